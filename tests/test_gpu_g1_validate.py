"""GPU: zkp_g1_validate / zkp_g1_validate_dev / zkp_g1_bases_validate / zkp_srs_check.  The expected status of every point comes from a
big-integer model in this file (canonical limbs, then the curve equation, then [r]P = O by an unreduced double-and-add), never from
the code under test: all-valid arrays at the wave and block edges, faults of every kind on every lane position of the edges, the same
faults through a handle (plain and both expansions), the 2^18 upload seam of the host entry, a sharded handle in a child process, and
the SRS structure check against SRSs that are right, tampered with, scaled, or paired with the wrong [s]_2."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bigmodel as bm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, R = bm.P, bm.R
RINV = pow(1 << 384, -1, P)
ONES = (1 << 384) - 1
FAULT_AT = [0, 63, 64, 128, 255, 256]
KINDS = ["x+p", "y+p", "x=p", "all-ones", "y+1", "(0,0)", "small-x", "(0,2)", "G+(0,2)", "[r]Q", "x+p,y+1"]
REPORT_KEYS = ["checked", "bad", "non_canonical", "off_curve", "outside_subgroup", "first_bad", "first_status"]


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def dev(a, dtype=np.int64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dtype)).cuda()


# ------------------------------------------------------------------------------------------------ the model
def mul_unreduced(pt, k):
    """bm.g1_mul reduces its scalar mod r; [r]P needs the scalar as it is"""
    acc = bm.INF
    for i in range(k.bit_length() - 1, -1, -1):
        acc = bm.g1_add(acc, acc)
        if (k >> i) & 1:
            acc = bm.g1_add(acc, pt)
    return acc


def raw_ints(row):
    return (sum(int(v) << (64 * k) for k, v in enumerate(row[:6])), sum(int(v) << (64 * k) for k, v in enumerate(row[6:])))


def raw_row(x, y):
    return [(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)] + [(y >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]


_status_cache = {}


def model_status(row, flagged=0):
    """the status the header defines, for 12 raw limbs (Montgomery residues as stored)"""
    if flagged:
        return 0
    x, y = raw_ints(row)
    if (x, y) not in _status_cache:
        if x >= P or y >= P:
            s = 1
        else:
            pt = (x * RINV % P, y * RINV % P)
            s = 2 if not bm.g1_on_curve(pt) else 0 if mul_unreduced(pt, R) is bm.INF else 3
        _status_cache[(x, y)] = s
    return _status_cache[(x, y)]


def expected_report(status):
    bad = np.nonzero(status)[0]
    return dict(checked=len(status), bad=len(bad), non_canonical=int((status == 1).sum()), off_curve=int((status == 2).sum()),
                outside_subgroup=int((status == 3).sum()), first_bad=int(bad[0]) if len(bad) else len(status),
                first_status=int(status[bad[0]]) if len(bad) else 0)


def mont(v):
    return v * (1 << 384) % P


def fault_row(kind, row):
    """the 12 raw limbs that replace `row` (a valid point) for one kind of fault"""
    x, y = raw_ints(row)
    q = (4, pow(4 ** 3 + 4, (P + 1) // 4, P))            # a curve point outside G1
    pt = lambda p: raw_row(mont(p[0]), mont(p[1]))
    return {"x+p": lambda: raw_row(x + P, y), "y+p": lambda: raw_row(x, y + P), "x=p": lambda: raw_row(P, y),
            "all-ones": lambda: raw_row(ONES, ONES), "y+1": lambda: raw_row(x, y + 1), "(0,0)": lambda: raw_row(0, 0),
            "small-x": lambda: pt(q), "(0,2)": lambda: pt((0, 2)), "G+(0,2)": lambda: pt(bm.g1_add(bm.G1, (0, 2))),
            "[r]Q": lambda: pt(mul_unreduced(q, R)), "x+p,y+1": lambda: raw_row(x + P, y + 1)}[kind]()


@pytest.fixture(scope="module")
def valid(orc):
    """1000 points k_i G, all finite, and the model's verdict on the first 257 of them (computed once)"""
    pts, inf = orc.g1_fixed_base_mul(orc.rand_fr(0x61C7, 1000))
    assert inf.sum() == 0
    assert all(model_status(pts[i]) == 0 for i in range(257))
    return pts


def with_infinities(pts, n):
    """the first n points; two of them (one when n == 1) flagged as infinity with their coordinates overwritten by 0xff bytes"""
    a, inf = pts[:n].copy(), np.zeros(n, dtype=np.uint8)
    for i in {0, n // 2} if n > 1 else {0}:
        inf[i] = 1
        a[i] = 0xFFFFFFFFFFFFFFFF
    return a, inf


def faulted(pts, shift):
    """257 points with fault kind (j + shift) mod 11 at the j-th of FAULT_AT, flagged infinities at 5 and 100; -> points, flags, statuses"""
    a, inf = pts[:257].copy(), np.zeros(257, dtype=np.uint8)
    for i in (5, 100):
        inf[i] = 1
        a[i] = 0xFFFFFFFFFFFFFFFF
    for j, at in enumerate(FAULT_AT):
        a[at] = fault_row(KINDS[(j + shift) % len(KINDS)], a[at])
    # (the other 249 finite points are the valid fixture's, whose verdict the model has given once)
    return a, inf, np.array([model_status(a[i], inf[i]) if i in FAULT_AT else 0 for i in range(257)], dtype=np.uint8)


def device_entry(zkp, a, inf, n):
    import torch
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    rep = zkp.g1_validate_dev(dev(a), n, dev(inf, np.uint8), st)
    return rep, st.cpu().numpy()


# ------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1000])
def test_all_valid(zkp, valid, n):
    a, inf = with_infinities(valid, n)
    exp = expected_report(np.zeros(n, dtype=np.uint8))
    rep, status = zkp.g1_validate(a, inf, want_status=True)
    assert rep == exp and not status.any()
    assert zkp.g1_validate(a, inf) == exp                      # no status array
    rep, status = device_entry(zkp, a, inf, n)
    assert rep == exp and not status.any()
    for expand in (None, False, True):
        h = zkp.G1Bases.from_host(a, inf)
        if expand is not None:
            h.precompute(12, glv=expand)
        rep, status = h.validate(want_status=True)
        assert rep == exp and not status.any(), expand
        assert h.validate() == exp
        h.close()
    if n > 1:  # the same coordinates without their flags are no points at all: 0xff bytes in every limb
        rep, status = zkp.g1_validate(a, None, want_status=True)
        assert rep["non_canonical"] == 2 and rep["bad"] == 2 and rep["first_bad"] == 0 and rep["first_status"] == 1
        assert status[0] == 1 and status[n // 2] == 1 and status.sum() == 2


def test_empty_and_null_arguments(zkp):
    import ctypes as C
    zero = dict.fromkeys(REPORT_KEYS, 0)
    assert zkp.g1_validate(np.zeros((0, 12), dtype=np.uint64)) == zero
    h = zkp.G1Bases.from_host(np.zeros((0, 12), dtype=np.uint64))
    assert h.validate() == zero
    assert zkp.lib().zkp_g1_validate(None, None, 3, None, None) == zkp.ZKP_E_ARG
    v = zkp._G1Validation()
    assert zkp.lib().zkp_g1_validate(None, None, 3, None, C.byref(v)) == zkp.ZKP_E_ARG
    assert zkp.lib().zkp_g1_validate_dev(None, None, 3, None, None, C.byref(v)) == zkp.ZKP_E_ARG
    assert zkp.lib().zkp_g1_bases_validate(None, None, C.byref(v)) == zkp.ZKP_E_ARG
    assert zkp.lib().zkp_g1_bases_validate(h._h, None, None) == zkp.ZKP_E_ARG


@pytest.mark.parametrize("shift", range(len(KINDS)))
def test_injected_faults_lane_by_lane(zkp, valid, shift):
    """over the eleven shifts every kind of fault sits once on every one of the six positions"""
    a, inf, exp_status = faulted(valid, shift)
    kinds = [KINDS[(j + shift) % len(KINDS)] for j in range(len(FAULT_AT))]
    want = {"x+p": 1, "y+p": 1, "x=p": 1, "all-ones": 1, "y+1": 2, "(0,0)": 2, "small-x": 3, "(0,2)": 3, "G+(0,2)": 3, "[r]Q": 3, "x+p,y+1": 1}
    assert [int(exp_status[at]) for at in FAULT_AT] == [want[k] for k in kinds]   # the model agrees with what each fault is meant to be
    exp = expected_report(exp_status)
    rep, status = zkp.g1_validate(a, inf, want_status=True)
    assert status.tobytes() == exp_status.tobytes(), (kinds, status[FAULT_AT])
    assert rep == exp
    rep, status = device_entry(zkp, a, inf, 257)
    assert status.tobytes() == exp_status.tobytes() and rep == exp
    assert zkp.g1_validate(a, inf) == exp                      # the report alone


@pytest.mark.parametrize("shift", [4, 5, 8])
def test_handle_form_on_the_same_faults(zkp, valid, shift):
    """the internal form has lost the raw limbs: the non-canonical entries are left out, statuses 2 and 3 must come back unchanged"""
    a, inf, exp_status = faulted(valid, shift)
    keep = exp_status != 1
    a, inf, exp_status = a[keep], inf[keep], exp_status[keep]
    assert (exp_status == 2).sum() + (exp_status == 3).sum() >= 2
    exp = expected_report(exp_status)
    for expand in (None, False, True):
        h = zkp.G1Bases.from_host(a, inf)
        if expand is not None:
            h.precompute(12, glv=expand)
        rep, status = h.validate(want_status=True)
        assert status.tobytes() == exp_status.tobytes(), (expand, status[exp_status != 0])
        assert rep == exp
        h.close()


def test_chunk_seam_of_the_host_entry(zkp, orc):
    import torch
    n = (1 << 18) + 1
    t_pts = torch.zeros(n * 12, dtype=torch.int64, device="cuda")
    zkp.g1_fixed_base_mul_dev(dev(orc.rand_fr(0x61C8, n)), n, t_pts)
    torch.cuda.synchronize()
    pts = t_pts.cpu().numpy().view(np.uint64).reshape(n, 12).copy()
    clean = expected_report(np.zeros(n, dtype=np.uint8))
    assert zkp.g1_validate_dev(t_pts, n) == clean
    exp_status = np.zeros(n, dtype=np.uint8)
    seam = 1 << 18                                              # index n - 1: the only point of the second upload
    for at, kind in ((seam - 2, "x+p"), (seam - 1, "y+1"), (seam, "(0,2)")):
        pts[at] = fault_row(kind, pts[at])
        exp_status[at] = model_status(pts[at])
    assert exp_status[[seam - 2, seam - 1, seam]].tolist() == [1, 2, 3]
    rep, status = zkp.g1_validate(pts, None, want_status=True)
    assert rep == expected_report(exp_status) and rep["first_bad"] == seam - 2 and rep["first_status"] == 1
    assert (rep["non_canonical"], rep["off_curve"], rep["outside_subgroup"]) == (1, 1, 1)
    assert status.tobytes() == exp_status.tobytes()
    pts[seam - 2], pts[seam - 1] = pts[0], pts[1]               # now the first bad point lies in the second upload
    exp_status[seam - 2:seam] = 0
    rep = zkp.g1_validate(pts)
    assert rep == expected_report(exp_status) and rep["first_bad"] == seam and rep["first_status"] == 3


def test_sharded_handle_in_a_child_process():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "g1_validate_worker.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "OK g1_validate slots" in p.stdout


@pytest.fixture(scope="module")
def srs257(zkp, orc):
    secret, other = orc.fr_from_ints([0x1F2E3D4C5B6A7988])[0], orc.fr_from_ints([0x1F2E3D4C5B6A7989])[0]
    pts = zkp.srs_g1(secret, 257)
    g2 = zkp.g2_generator()
    g2s, _ = zkp.g2_mul(g2, secret)
    g2o, _ = zkp.g2_mul(g2, other)
    r = orc.rand_fr(0x61C9, 256)
    r[:, 2:] = 0                                                # 128-bit scalars, as Fr::from(rng.gen::<u128>())
    r = orc.fr_from_ints([v & ((1 << 128) - 1) for v in orc.limbs_to_ints(r)])
    decoys, _ = orc.g1_fixed_base_mul(orc.rand_fr(0x61CA, 3))   # other multiples of G
    return pts, g2s, g2o, r, decoys


@pytest.mark.parametrize("n", [1, 2, 3, 64, 257])
def test_srs_check(zkp, orc, srs257, n):
    pts, g2s, g2o, r, decoys = srs257
    pts = pts[:n]
    plain = zkp.G1Bases.from_host(pts)
    assert plain.validate()["bad"] == 0
    assert zkp.srs_check(plain, g2s, n, r) == 1
    assert zkp.srs_check(zkp.G1Bases.from_host(pts).precompute(12), g2s, n, r) == 1
    assert zkp.srs_check(zkp.G1Bases.from_host(pts).precompute(12, glv=True), g2s, n, r) == 1
    for k, at in enumerate(sorted({0, n // 2, n - 1})):
        bad = pts.copy()
        bad[at] = decoys[k]
        assert zkp.srs_check(zkp.G1Bases.from_host(bad), g2s, n, r) == 0, at
    if n > 1:
        assert zkp.srs_check(plain, g2o, n, r) == 0             # the [s]_2 of another secret (n == 1 looks at P_0 only)
    two = orc.fr_from_ints([2])[0]
    scaled = np.stack([orc.g1_mul(p, 0, two)[0] for p in pts[:min(n, 3)]])
    if n <= 3:  # [2 s^i]G: the chain holds, P_0 is not the generator
        h = zkp.G1Bases.from_host(scaled)
        assert h.validate()["bad"] == 0 and zkp.srs_check(h, g2s, n, r) == 0
    else:
        bad = pts.copy()
        bad[0] = scaled[0]
        assert zkp.srs_check(zkp.G1Bases.from_host(bad), g2s, n, r) == 0
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.srs_check(plain, g2s, n + 1, np.concatenate([r, r]))
    assert ei.value.code == zkp.ZKP_E_SIZE
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.srs_check(plain, g2s, 0, r)
    assert ei.value.code == zkp.ZKP_E_ARG
    off = g2s.copy()
    off[12] ^= 1                                                # y.c0 changed: off the twist
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.srs_check(plain, off, n, r)
    assert ei.value.code == zkp.ZKP_E_ARG


def test_scaled_srs_is_rejected_for_p0(zkp, orc, srs257):
    """the SRS of the same secret scaled by 2, whole: consistent with [s]_2 along the chain, refused for P_0"""
    pts, g2s, _, r, _ = srs257
    n = 64
    ks = orc.fr_from_ints([2 * pow(0x1F2E3D4C5B6A7988, i, R) % R for i in range(n)])
    scaled, inf = orc.g1_fixed_base_mul(ks)
    assert inf.sum() == 0
    h = zkp.G1Bases.from_host(scaled)
    assert h.validate()["bad"] == 0
    assert zkp.srs_check(h, g2s, n, r) == 0
    fixed = scaled.copy()
    fixed[0] = pts[0]                                           # P_0 put right: now the chain breaks between P_0 and P_1
    assert zkp.srs_check(zkp.G1Bases.from_host(fixed), g2s, n, r) == 0
