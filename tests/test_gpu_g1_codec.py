"""GPU: compressed G1 points and scalar bytes (zkp_g1_decompress*, zkp_g1_compress*, zkp_g1_bases_create_compressed,
zkp_fr_from_bytes_dev, zkp_fr_to_bytes_dev, KzgCellVerifier.verify_bytes).  Every expectation -- status bytes, the report, the limbs
and the infinity flags -- comes from the big-integer model tests/model/g1_codec_model.py, never from the code under test: all-valid
arrays at the wave and block edges with infinities among them, every kind of fault on every lane position of the edges with and
without the subgroup flag, both round trips, the 2^18 upload seam of the host entry, a handle made from bytes, scalars in both byte
orders, and cells verified from their wire form.  No test provokes a fault: bad input here is a status, an error code or a rejected
batch."""
import numpy as np
import pytest

import bigmodel as bm
import g1_codec_model as cm

pytestmark = pytest.mark.gpu
P, R = bm.P, bm.R
FAULT_AT = [0, 63, 64, 128, 255, 256]
KINDS = ["c-clear", "i+s", "i+low-bit", "x=p", "x=2^381-1", "x=1", "x=2", "x=3", "x=7", "x=0", "x=4", "s-flipped"]
# status with the subgroup flag, status without
WANT = {"c-clear": (4, 4), "i+s": (4, 4), "i+low-bit": (4, 4), "x=p": (1, 1), "x=2^381-1": (1, 1), "x=1": (2, 2), "x=2": (2, 2),
        "x=3": (2, 2), "x=7": (2, 2), "x=0": (3, 0), "x=4": (3, 0), "s-flipped": (0, 0)}
REPORT_KEYS = ["checked", "bad", "malformed", "non_canonical", "off_curve", "outside_subgroup", "first_bad", "first_status"]
SECRET = 0x1F2E3D4C5B6A7988


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


# ------------------------------------------------------------------------------------------------ the model's side
_decoded = {}


def model_decode(b, subgroup):
    """(status, twelve limbs, infinity flag) of one encoding, computed once per encoding and flag"""
    key = (bytes(b), subgroup)
    if key not in _decoded:
        st, pt = cm.decompress(key[0], subgroup)
        inf = st == 0 and pt is bm.INF
        _decoded[key] = (st, cm.abi_row(None if st or inf else pt), int(inf))
    return _decoded[key]


def expected(enc, subgroup):
    """enc: (n, 48) uint8 -> statuses, (n, 12) limbs, flags, report"""
    rows = [model_decode(enc[i].tobytes(), subgroup) for i in range(enc.shape[0])]
    status = np.array([r[0] for r in rows], dtype=np.uint8)
    xy = np.array([r[1] for r in rows], dtype=np.uint64).reshape(-1, 12)
    inf = np.array([r[2] for r in rows], dtype=np.uint8)
    bad = np.nonzero(status)[0]
    rep = dict(checked=len(status), bad=len(bad), malformed=int((status == 4).sum()), non_canonical=int((status == 1).sum()),
               off_curve=int((status == 2).sum()), outside_subgroup=int((status == 3).sum()),
               first_bad=int(bad[0]) if len(bad) else len(status), first_status=int(status[bad[0]]) if len(bad) else 0)
    return status, xy, inf, rep


def encode_rows(rows, inf=None):
    """the model's bytes of ABI limbs (no square root: cheap; limbs read as little-endian bytes, 2^18 rows in about a second)"""
    raw, out = np.ascontiguousarray(rows, dtype=np.uint64).tobytes(), bytearray()
    for i in range(len(rows)):
        if inf is not None and inf[i]:
            out += cm.INF_BYTES
            continue
        x, y = int.from_bytes(raw[96 * i:96 * i + 48], "little"), int.from_bytes(raw[96 * i + 48:96 * i + 96], "little")
        out += cm.compress((x * cm.RINV % P, y * cm.RINV % P))
    return np.frombuffer(bytes(out), dtype=np.uint8).reshape(len(rows), 48).copy()


def as_bytes(v):
    return np.frombuffer(v.to_bytes(48, "big"), dtype=np.uint8)


def fault_bytes(kind, b):
    """the 48 bytes that replace the valid encoding b for one kind of fault"""
    v = int.from_bytes(b.tobytes(), "big")
    c = 1 << 383
    return as_bytes({"c-clear": v & ~c, "i+s": 0xE0 << 376, "i+low-bit": 0xC0 << 376 | 1, "x=p": c | P, "x=2^381-1": c | ((1 << 381) - 1),
                     "x=1": c | 1, "x=2": c | 2 | 1 << 381, "x=3": c | 3, "x=7": c | 7 | 1 << 381, "x=0": c | 1 << 381, "x=4": c | 4 | 1 << 381,
                     "s-flipped": v ^ 1 << 381}[kind])


@pytest.fixture(scope="module")
def valid(orc):
    """300 points k_i G as limbs, and their encodings by the model; the model decodes every one of them back to the same limbs and finds
    it in G1 (computed once)"""
    rows, inf = orc.g1_fixed_base_mul(orc.rand_fr(0x61D0, 300))
    assert inf.sum() == 0
    enc = encode_rows(rows)
    st, xy, flags, rep = expected(enc, True)
    assert rep["bad"] == 0 and not flags.any() and np.array_equal(xy, rows)
    assert 100 < int((enc[:, 0] & 0x20 != 0).sum()) < 200          # both signs occur
    return rows, enc


def with_infinities(enc, n):
    a = enc[:n].copy()
    for i in {n // 3, (2 * n) // 3} if n > 2 else set():
        a[i] = np.frombuffer(cm.INF_BYTES, dtype=np.uint8)
    return a


def faulted(enc, shift):
    a = enc[:257].copy()
    for i in (5, 100):
        a[i] = np.frombuffer(cm.INF_BYTES, dtype=np.uint8)
    kinds = [KINDS[(j + shift) % len(KINDS)] for j in range(len(FAULT_AT))]
    for at, kind in zip(FAULT_AT, kinds):
        a[at] = fault_bytes(kind, a[at])
    return a, kinds


def device_decode(zkp, enc, subgroup, want_status=True):
    import torch
    n = enc.shape[0]
    xy = torch.full((n * 12,), -1, dtype=torch.int64, device="cuda")
    inf = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda") if want_status else None
    rep = zkp.g1_decompress_dev(dev(enc), n, xy, inf, check_subgroup=subgroup, status_tensor=st)
    return xy.cpu().numpy().view(np.uint64).reshape(n, 12), inf.cpu().numpy(), rep, st.cpu().numpy() if want_status else None


def check_both_entries(zkp, enc, subgroup, note=None):
    status, xy, inf, rep = expected(enc, subgroup)
    got_xy, got_inf, got_rep, got_status = zkp.g1_decompress(enc, check_subgroup=subgroup, want_status=True)
    assert got_status.tobytes() == status.tobytes(), (note, "host", got_status[status != got_status])
    assert got_rep == rep and np.array_equal(got_xy, xy) and got_inf.tobytes() == inf.tobytes(), (note, "host")
    got_xy, got_inf, got_rep, got_status = device_decode(zkp, enc, subgroup)
    assert got_status.tobytes() == status.tobytes(), (note, "device")
    assert got_rep == rep and np.array_equal(got_xy, xy) and got_inf.tobytes() == inf.tobytes(), (note, "device")
    got_xy, got_inf, got_rep, _ = device_decode(zkp, enc, subgroup, want_status=False)      # no status array
    assert got_rep == rep and np.array_equal(got_xy, xy) and got_inf.tobytes() == inf.tobytes(), (note, "device, no status")
    got_xy, got_inf, got_rep = zkp.g1_decompress(enc, check_subgroup=subgroup)
    assert got_rep == rep and np.array_equal(got_xy, xy) and got_inf.tobytes() == inf.tobytes(), (note, "host, no status")
    return status, xy, inf


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 300])
def test_all_valid_and_both_round_trips(zkp, valid, n):
    import torch
    rows, enc = valid
    a = with_infinities(enc, n)
    for subgroup in (True, False):
        status, xy, inf = check_both_entries(zkp, a, subgroup, n)
        assert not status.any() and inf.sum() == (2 if n > 2 else 0)
    finite = inf == 0
    assert np.array_equal(xy[finite], rows[:n][finite])                               # the limbs the points were made from
    # compress(decompress(b)) == b, through both entries
    assert zkp.g1_compress(xy, inf).tobytes() == a.tobytes()
    out = torch.full((n * 48,), 0xEE, dtype=torch.uint8, device="cuda")
    zkp.g1_compress_dev(dev(xy), n, out, is_inf_tensor=dev(inf))
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == a.tobytes()
    # decompress(compress(P)) == P, and without flags every point is finite
    b = zkp.g1_compress(rows[:n])
    assert b.tobytes() == enc[:n].tobytes()
    back, back_inf, rep = zkp.g1_decompress(b)
    assert np.array_equal(back, rows[:n]) and not back_inf.any() and rep["bad"] == 0


@pytest.mark.parametrize("shift", range(len(KINDS)))
def test_injected_faults_lane_by_lane(zkp, valid, shift):
    """over the twelve shifts every kind of fault sits once on every one of the six positions"""
    rows, enc = valid
    a, kinds = faulted(enc, shift)
    for col, subgroup in enumerate((True, False)):
        status, xy, inf = check_both_entries(zkp, a, subgroup, kinds)
        assert [int(status[at]) for at in FAULT_AT] == [WANT[k][col] for k in kinds]       # the model agrees with what each fault is meant to be
        assert inf[5] == 1 and inf[100] == 1 and inf.sum() == 2
        for at, kind in zip(FAULT_AT, kinds):
            if status[at]:
                assert not xy[at].any() and inf[at] == 0                                    # a bad point is (0, 0), not flagged
            elif kind == "s-flipped":
                assert np.array_equal(xy[at][:6], rows[at][:6]) and cm.point_of_row(xy[at]) == bm.g1_neg(cm.point_of_row(rows[at]))
            else:                                                                           # x = 0 or 4 without the flag: the model's point
                pt = cm.point_of_row(xy[at])
                assert pt[0] == int(kind[2:]) and bm.g1_on_curve(pt) and pt[1] > cm.HALF


def test_compress_of_an_srs_is_the_models_bytes(zkp, orc):
    pts = zkp.srs_g1(orc.fr_from_ints([SECRET])[0], 67)
    want = np.stack([np.frombuffer(cm.compress(bm.g1_mul(bm.G1, pow(SECRET, i, R))), dtype=np.uint8) for i in range(67)])
    got = zkp.g1_compress(pts)
    assert got.tobytes() == want.tobytes() and got[0].tobytes() == cm.compress(bm.G1) and got[0, 0] == 0x97
    back, inf, rep = zkp.g1_decompress(got)
    assert np.array_equal(back, pts) and not inf.any() and rep["bad"] == 0 and rep["checked"] == 67
    # limbs that are no point give bytes that are no encoding, never a fault: all-ones limbs, and zeros without a flag
    junk = np.full((65, 12), 0xFFFFFFFFFFFFFFFF, dtype=np.uint64)
    junk[1::2] = 0
    out = zkp.g1_compress(junk)
    assert out.shape == (65, 48) and out[1].tobytes() == bytes([0x80]) + bytes(47)           # x = 0, y = 0: c set, s clear


def test_chunk_seam_of_the_host_entry(zkp, orc):
    import torch
    seam = 1 << 18
    n = seam + 3
    t_pts = torch.zeros(n * 12, dtype=torch.int64, device="cuda")
    zkp.g1_fixed_base_mul_dev(dev(orc.rand_fr(0x61D1, n)), n, t_pts)
    torch.cuda.synchronize()
    pts = t_pts.cpu().numpy().view(np.uint64).reshape(n, 12).copy()
    enc = encode_rows(pts)                                                            # by the model
    xy, inf, rep = zkp.g1_decompress(enc, check_subgroup=False)
    assert rep == dict(checked=n, bad=0, malformed=0, non_canonical=0, off_curve=0, outside_subgroup=0, first_bad=n, first_status=0)
    assert np.array_equal(xy, pts) and not inf.any()
    # the device's own encoding of the same points, in one call
    out = torch.zeros(n * 48, dtype=torch.uint8, device="cuda")
    zkp.g1_compress_dev(t_pts, n, out)
    torch.cuda.synchronize()
    assert out.cpu().numpy().tobytes() == enc.tobytes()
    want_status = np.zeros(n, dtype=np.uint8)
    for at, kind in ((seam - 1, "c-clear"), (seam, "x=p"), (seam + 1, "x=1")):        # the last point of the first upload, the first two of the second
        enc[at] = fault_bytes(kind, enc[at])
        want_status[at] = WANT[kind][1]
        pts[at] = 0
    xy, inf, rep, status = zkp.g1_decompress(enc, check_subgroup=False, want_status=True)
    assert rep == dict(checked=n, bad=3, malformed=1, non_canonical=1, off_curve=1, outside_subgroup=0, first_bad=seam - 1, first_status=4)
    assert status.tobytes() == want_status.tobytes() and np.array_equal(xy, pts) and not inf.any()
    enc[seam - 1] = enc[0]                                                            # now the first bad point lies in the second upload
    rep = zkp.g1_decompress(enc, check_subgroup=False)[2]
    assert (rep["bad"], rep["first_bad"], rep["first_status"]) == (2, seam, 1)
    enc[seam] = enc[1]
    rep = zkp.g1_decompress(enc, check_subgroup=False)[2]
    assert (rep["bad"], rep["first_bad"], rep["first_status"]) == (1, seam + 1, 2)


def test_bases_from_compressed(zkp, orc):
    pts = zkp.srs_g1(orc.fr_from_ints([SECRET])[0], 67)
    enc = encode_rows(pts)
    coeffs = orc.rand_fr(0x61D2, 67)
    ref = zkp.G1Bases.from_host(pts)
    want = zkp.kzg_commit(ref, coeffs)
    for subgroup in (True, False):
        h = zkp.G1Bases.from_compressed(enc, check_subgroup=subgroup)
        assert len(h) == 67
        got = zkp.kzg_commit(h, coeffs)
        assert np.array_equal(np.asarray(got[0]), np.asarray(want[0])) and int(got[1]) == int(want[1])
        h.close()
    h = zkp.G1Bases.from_compressed(enc.tobytes())                                    # plain bytes
    assert h.validate()["bad"] == 0
    h.close()
    for at, kind, word, subgroup in ((40, "x=1", "curve", True), (66, "c-clear", "encoding", False), (0, "x=p", "canonical", True),
                                     (3, "x=4", "subgroup", True)):
        bad = enc.copy()
        bad[at] = fault_bytes(kind, bad[at])
        with pytest.raises(zkp.ZkpError) as ei:
            zkp.G1Bases.from_compressed(bad, check_subgroup=subgroup)
        assert ei.value.code == zkp.ZKP_E_ARG and "point %d " % at in str(ei.value) and word in str(ei.value), str(ei.value)
        assert ei.value.report["first_bad"] == at and ei.value.report["bad"] == 1 and ei.value.report["checked"] == 67
    bad = enc.copy()
    bad[3] = fault_bytes("x=4", bad[3])                                               # on the curve, outside G1: taken when nobody asks
    h = zkp.G1Bases.from_compressed(bad, check_subgroup=False)
    rep = h.validate()
    assert (rep["bad"], rep["first_bad"], rep["first_status"]) == (1, 3, 3)
    h.close()
    ref.close()


@pytest.mark.parametrize("big_endian", [True, False])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_scalars(zkp, n, big_endian):
    import torch
    special = [0, 1, R - 1, R, (1 << 256) - 1]
    vals = [R - 1] if n == 1 else (special + bm.rand_fr_list(0x61D3 + n, n))[:n]
    if n > 200:
        vals[200] = R + 1
    raw = np.frombuffer(b"".join(cm.fr_to_bytes(v, big_endian) for v in vals), dtype=np.uint8).copy()
    decoded = [cm.fr_from_bytes(raw[32 * i:32 * i + 32].tobytes(), big_endian) for i in range(n)]
    bad_at = [i for i, (ok, _) in enumerate(decoded) if not ok]
    assert len(bad_at) == (0 if n == 1 else 3)
    want = np.array([bm.to_limbs(bm.fr_to_mont(v), 4) for _, v in decoded], dtype=np.uint64).reshape(n, 4)
    out = torch.full((n * 4,), -1, dtype=torch.int64, device="cuda")
    bad, first = zkp.fr_from_bytes_dev(dev(raw), n, out, big_endian=big_endian)
    assert (bad, first) == (len(bad_at), bad_at[0] if bad_at else n)
    assert np.array_equal(out.cpu().numpy().view(np.uint64).reshape(n, 4), want)
    back = torch.full((n * 32,), 0xEE, dtype=torch.uint8, device="cuda")
    zkp.fr_to_bytes_dev(out, n, back, big_endian=big_endian)
    torch.cuda.synchronize()
    back = back.cpu().numpy()
    for i, (ok, v) in enumerate(decoded):                                              # to_bytes(from_bytes(b)) == b; a refused value is zero
        assert back[32 * i:32 * i + 32].tobytes() == (raw[32 * i:32 * i + 32].tobytes() if ok else bytes(32)), i


def test_verify_bytes_end_to_end(zkp, orc):
    log_n, log_l = 6, 2
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    pts = zkp.srs_g1(orc.fr_from_ints([SECRET])[0], n)
    bases = zkp.G1Bases.from_compressed(encode_rows(pts))
    g2_sl = zkp.g2_mul(zkp.g2_generator(), orc.fr_from_ints([pow(SECRET, l, R)])[0])[0]
    polys = [orc.rand_fr(0x61D4, n), orc.rand_fr(0x61D5, n - 5), orc.rand_fr(0x61D6, l)]    # the last one: every proof is the identity
    opener = zkp.KzgOpener(bases, log_n, log_l)
    commits, proofs, cell_bytes, ci, ki = [], [], [], [], []
    for m, f in enumerate(polys):
        (xy, inf), ev = opener.open_cosets(f, evals=True)
        c, cinf = zkp.kzg_commit(bases, f)
        commits.append(cm.compress(bm.INF if cinf else cm.point_of_row(np.asarray(c))))
        ev_int = orc.fr_to_ints(ev)
        for k in range(r):
            proofs.append(cm.compress(bm.INF if inf[k] else cm.point_of_row(xy[k])))
            cell_bytes.append(b"".join(cm.fr_to_bytes(int(v), True) for v in ev_int[k::r]))
            ci.append(m)
            ki.append(k)
    opener.close()
    assert proofs[2 * r] == cm.INF_BYTES and commits[2] != cm.INF_BYTES
    cells = len(ci)
    weights = orc.fr_from_ints([(0x9E3779B97F4A7C15 * (i + 1)) % (1 << 128) for i in range(cells)])
    ver = zkp.KzgCellVerifier(bases, g2_sl, log_n, log_l, cells, len(polys))
    c48, p48, sb = b"".join(commits), b"".join(proofs), b"".join(cell_bytes)
    assert ver.verify_bytes(c48, ci, ki, sb, p48, weights) is True
    le = b"".join(cell_bytes[i][32 * j:32 * j + 32][::-1] for i in range(cells) for j in range(l))
    assert ver.verify_bytes(c48, ci, ki, le, p48, weights, big_endian=False) is True
    at = 5
    flipped = bytearray(p48)
    flipped[48 * at] ^= 0x20                                                          # the other root: still a point of G1, a wrong proof
    assert ver.verify_bytes(c48, ci, ki, sb, bytes(flipped), weights) is False
    broken = bytearray(p48)
    broken[48 * at:48 * at + 48] = (1 << 383 | 1).to_bytes(48, "big")                 # x = 1: x^3 + 4 is no square
    with pytest.raises(zkp.ZkpError) as ei:
        ver.verify_bytes(c48, ci, ki, sb, bytes(broken), weights)
    assert ei.value.code == zkp.ZKP_E_ARG and "proofs" in str(ei.value) and "[5]" in str(ei.value) and "curve" in str(ei.value)
    worse = bytearray(c48)
    worse[48] &= 0x7F
    with pytest.raises(zkp.ZkpError) as ei:
        ver.verify_bytes(bytes(worse), ci, ki, sb, p48, weights)
    assert ei.value.code == zkp.ZKP_E_ARG and "commitments[1]" in str(ei.value) and "encoding" in str(ei.value)
    big = bytearray(sb)
    big[32 * 7:32 * 7 + 32] = cm.fr_to_bytes(R, True)
    with pytest.raises(zkp.ZkpError) as ei:
        ver.verify_bytes(c48, ci, ki, bytes(big), p48, weights)
    assert ei.value.code == zkp.ZKP_E_ARG and "cell_bytes[7]" in str(ei.value) and "canonical" in str(ei.value)
    ver.close()
    bases.close()
