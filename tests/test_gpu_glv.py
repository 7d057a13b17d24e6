"""GPU: the endomorphism-split MSM (zkp_g1_bases_precompute_glv).  Every result is compared bit for bit with the oracle's naive MSM and
with the same call over a plain expansion of the same points: the scalar split itself (zkp_selftest_glv_split_dev against divmod),
MSMs at the sizes and scalars where the split, the recoding or the two-set tail can go wrong, scalar ranges, batches, the handle's
bookkeeping, a sharded handle, and the users of the MSM (KZG open, PLONK prove / verify, one Nova fold)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bigmodel as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R
LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF
SPECIAL = [R - 1, LAMBDA, LAMBDA - 1, LAMBDA + 1, 0, 1]  # r - 1 = (lambda + 1) lambda: k1 = 0 and the largest k2
EDGES = [0, 1] + [m * LAMBDA + d for m in (1, 2, 1 << 64, LAMBDA - 1, LAMBDA, LAMBDA + 1) for d in (-1, 0, 1) if m * LAMBDA + d < R] + [R - 1, R - 2]
NMAX = 4096


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


@pytest.fixture(scope="module")
def points(orc):
    """4096 points k_i G (k_i kept: the identity case needs them), two of them the point at infinity"""
    ks = orc.rand_fr(0x61C, NMAX)
    ks[0] = 0
    ks[17] = 0
    pts, inf = orc.g1_fixed_base_mul(ks)
    assert inf[0] == 1 and inf[17] == 1 and inf.sum() == 2
    return ks, pts, inf


_handles = {}


def handle(zkp, points, n, wb, glv, first=0):
    """an expanded handle over points [first, first + n), made once per (n, width, mode)"""
    key = (first, n, wb, glv)
    if key not in _handles:
        _, pts, inf = points
        _handles[key] = zkp.G1Bases.from_host(pts[first:first + n], inf[first:first + n]).precompute(wb, glv=glv)
    return _handles[key]


def scalars_for(orc, n):
    sc = orc.rand_fr(0x5EED6100 + n, n)
    sc[:min(n, 6)] = orc.fr_from_ints(SPECIAL[:min(n, 6)])
    if n >= 63:
        sc[20:40] = sc[19]  # equal scalars: one crowded bucket per slice
    return sc


_refs = {}


def reference(orc, points, n, first=0):
    """(scalars, oracle's naive MSM) for size n, computed once"""
    if (n, first) not in _refs:
        _, pts, inf = points
        sc = scalars_for(orc, n)
        _refs[(n, first)] = (sc, orc.msm_naive(pts[first:first + n], inf[first:first + n], sc))
    return _refs[(n, first)]


def test_split_hook_matches_divmod(zkp, orc):
    import torch
    ks = EDGES + orc.fr_to_ints(orc.rand_fr(0x61C1, 4096))
    assert len(EDGES) == 21
    n = len(ks)
    out = torch.zeros(8 * n, dtype=torch.int32, device="cuda")
    zkp.selftest_glv_split_dev(dev(orc.fr_from_ints(ks)), n, out)
    torch.cuda.synchronize()
    w = out.cpu().numpy().view(np.uint32).reshape(n, 8)
    for k, row in zip(ks, w):
        k2, k1 = divmod(k, LAMBDA)
        exp = [(k1 >> (32 * j)) & 0xFFFFFFFF for j in range(4)] + [(k2 >> (32 * j)) & 0xFFFFFFFF for j in range(4)]
        assert row.tolist() == exp, hex(k)


@pytest.mark.parametrize("wb", [9, 12, 16, 0])
def test_msm_sizes_and_edge_scalars(zkp, orc, points, wb):
    for n in (1, 2, 63, 64, 65, 300, NMAX):
        first = 1 if n <= 2 else 0  # (point 0 is the point at infinity: the smallest cases take finite bases)
        if wb == 0 and n < 64:
            continue  # the automatic width leaves fewer than 64 points unexpanded
        sc, (exp, einf) = reference(orc, points, n, first)
        split, plain = handle(zkp, points, n, wb, True, first), handle(zkp, points, n, wb, False, first)
        assert split.expansion()["glv"] == 1 and plain.expansion()["glv"] == 0
        got, ref = zkp.msm_g1_dev(split, dev(sc), n), zkp.msm_g1_dev(plain, dev(sc), n)
        assert got[1] == einf and np.array_equal(got[0], exp), (n, wb)
        assert ref[1] == einf and np.array_equal(ref[0], exp), (n, wb)
        got = zkp.msm_g1(split, sc)  # host scalars
        assert got[1] == einf and np.array_equal(got[0], exp), (n, wb)
        if n == 300:  # a prefix of the bases
            expm = orc.msm_naive(points[1][:77], points[2][:77], sc[:77])
            got = zkp.msm_g1_dev(split, dev(sc), 77)
            assert got[1] == expm[1] and np.array_equal(got[0], expm[0])


@pytest.mark.parametrize("wb", [12, 0])
@pytest.mark.parametrize("what", ["k2_zero", "k1_zero", "identity", "all_equal", "all_r_minus_1"])
def test_msm_degenerate_halves(zkp, orc, points, wb, what):
    """one of the two bucket sets sums to the identity, the whole sum is the identity, every point of a slice in one bucket"""
    n = 300
    ks, pts, inf = points
    small = [v % LAMBDA for v in orc.fr_to_ints(orc.rand_fr(0x61C2, n))]
    if what == "k2_zero":
        vals = small                                 # below lambda: the second total is the identity
    elif what == "k1_zero":
        vals = [v * LAMBDA for v in small]           # multiples of lambda (< r): the first total is the identity
        vals[5] = 0
    elif what == "identity":
        vals = orc.fr_to_ints(orc.rand_fr(0x61C3, n))
        kk = orc.fr_to_ints(ks[:n])
        vals[n - 1] = -sum(v * k for v, k in zip(vals[:n - 1], kk[:n - 1])) * pow(kk[n - 1], -1, R) % R
    elif what == "all_equal":
        vals = [0x1234567 * LAMBDA + 0x89ABCDEF] * n
    else:
        vals = [R - 1] * n
    sc = orc.fr_from_ints(vals)
    exp, einf = orc.msm_naive(pts[:n], inf[:n], sc)
    assert einf == (1 if what == "identity" else 0)
    for glv in (True, False):
        got = zkp.msm_g1_dev(handle(zkp, points, n, wb, glv), dev(sc), n)
        assert got[1] == einf and np.array_equal(got[0], exp), (what, glv)


@pytest.mark.parametrize("mode", ["ranges", "slots"])
def test_ranges_and_sharded_handle_in_a_child_process(mode):
    """ranges: ZKP_MSM_RANGE_LOG=10, 4096 scalars in four ranges (resume, hand-over array, two bucket sets), resident and host scalars;
    slots: two slots on one GPU, a sharded split handle, n = 300"""
    env = dict(os.environ)
    if mode == "ranges":
        env["ZKP_MSM_RANGE_LOG"] = "10"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "glv_worker.py"), mode], capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "OK glv " + mode in p.stdout


def test_batches(zkp, orc, points):
    n, wb = 300, 12
    _, pts, inf = points
    split, plain = handle(zkp, points, n, wb, True), handle(zkp, points, n, wb, False)
    vecs = [orc.rand_fr(0x5EED6200 + i, n) for i in range(33)]
    vecs[1][:] = 0                                   # the identity in the middle of a batch
    vecs[2][:6] = orc.fr_from_ints(SPECIAL)
    d = [dev(v) for v in vecs]
    singles = [zkp.msm_g1_dev(split, t, n) for t in d[:32]]
    for v, (xy, i) in list(zip(vecs, singles))[:4]:
        exp, einf = orc.msm_naive(pts[:n], inf[:n], v)
        assert i == einf and np.array_equal(xy, exp)
    for count in (3, 32):
        got, ref = zkp.msm_g1_batch_dev(split, d[:count], n), zkp.msm_g1_batch_dev(plain, d[:count], n)
        for k in range(count):
            assert got[k][1] == singles[k][1] and np.array_equal(got[k][0], singles[k][0]), (count, k)
            assert ref[k][1] == singles[k][1] and np.array_equal(ref[k][0], singles[k][0]), (count, k)
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.msm_g1_batch_dev(split, d, n)            # 33: two bucket sets per MSM, 64 per pass
    assert ei.value.code == zkp.ZKP_E_ARG and "32 MSMs" in str(ei.value)
    assert len(zkp.msm_g1_batch_dev(plain, d, n)) == 33
    part = zkp.msm_g1_partial_dev(split, d[0], n)
    xy, i = zkp.g1_xyzz_sum(part.reshape(1, 24))
    assert i == singles[0][1] and np.array_equal(xy, singles[0][0])


def test_handle_bookkeeping(zkp, orc, points, monkeypatch):
    _, pts, inf = points
    n = 300
    for wb in (9, 12, 16, 20, 22):
        planes, full = -(-129 // wb), -(-256 // wb)
        s, p = handle(zkp, points, n, wb, True), handle(zkp, points, n, wb, False)
        e, f = s.expansion(), p.expansion()
        assert (e["window_bits"], e["planes"], e["slices"], e["glv"], e["bytes"]) == (wb, planes, 2 * planes, 1, 128 * planes * n)
        assert (f["window_bits"], f["planes"], f["slices"], f["glv"], f["bytes"]) == (wb, full, full, 0, 128 * full * n)
        assert e["bytes"] * full <= f["bytes"] * planes
        assert e["widest_slice_bits"] == -(-129 // planes) and s.info() == (wb, 2 * planes) and p.info() == (wb, full)
    s, p = handle(zkp, points, n, 12, True), handle(zkp, points, n, 12, False)
    s.precompute(12, glv=True)  # the same mode and width again
    p.precompute(12)
    for h, glv, wb in ((s, False, 12), (p, True, 12), (s, False, 0), (p, True, 0), (s, True, 16)):
        with pytest.raises(zkp.ZkpError) as ei:
            h.precompute(wb, glv=glv)
        assert ei.value.code == zkp.ZKP_E_ARG
    assert s.expansion()["glv"] == 1 and p.expansion()["glv"] == 0
    fresh = zkp.G1Bases.from_host(pts[:n], inf[:n])
    assert fresh.expansion() == dict(window_bits=0, slices=0, planes=0, glv=0, widest_slice_bits=0, bytes=0)
    # a budget between the two sizes: the split expansion fits where the plain one is refused
    monkeypatch.setenv("ZKP_SRS_EXPAND_MAX_BYTES", str(128 * 7 * n))
    with pytest.raises(zkp.ZkpError) as ei:
        fresh.precompute(20)
    assert ei.value.code == zkp.ZKP_E_NOMEM and "13 planes x 300 points" in str(ei.value)
    assert fresh.info() == (0, 0)
    fresh.precompute(20, glv=True)
    assert fresh.info() == (20, 14) and fresh.expansion()["bytes"] == 128 * 7 * n
    monkeypatch.setenv("ZKP_SRS_EXPAND_MAX_BYTES", str(128 * 7 * n - 1))
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.G1Bases.from_host(pts[:n], inf[:n]).precompute(20, glv=True)
    assert ei.value.code == zkp.ZKP_E_NOMEM and "7 planes x 300 points" in str(ei.value)
    sc, (exp, einf) = reference(orc, points, n)
    got = zkp.msm_g1(fresh, sc)
    assert got[1] == einf and np.array_equal(got[0], exp)


def test_kzg_open_over_a_split_srs(zkp, orc):
    n = 300
    secret = orc.fr_from_ints([0x1F2E3D4C5B6A7988])[0]
    coeffs, z = orc.rand_fr(0x61C4, n), orc.rand_fr(0x61C5, 1)[0]
    a, b = zkp.Srs.new_from_secret(secret, n), zkp.Srs.new_from_secret(secret, n)
    a.bases.precompute(12, glv=True)
    b.bases.precompute(12)
    (xa, ia), eva = zkp.kzg_open(a.bases, coeffs, z)
    (xb, ib), evb = zkp.kzg_open(b.bases, coeffs, z)
    assert ia == ib == 0 and np.array_equal(xa, xb) and np.array_equal(eva, evb)
    ca, cb = zkp.kzg_commit(a.bases, coeffs), zkp.kzg_commit(b.bases, coeffs)
    exp, einf = orc.msm_naive(a.g1_points_xy[:n], None, coeffs)
    assert ca[1] == cb[1] == einf and np.array_equal(ca[0], exp) and np.array_equal(cb[0], exp)


def test_plonk_proof_over_a_split_srs_is_byte_identical(zkp, orc):
    import pairing_model as PairM
    import plonk_model as PM
    from test_pairing_cpu import g2_from_ints
    from test_plonk_model import challenges
    cc = PM.reference_test_circuit_03().compile()  # n = 2: the smallest of the reference's circuits
    blinders, _ = challenges(7)
    secret = M.rand_fr_list(407, 1)[0]
    n = cc["n"]
    polys = {k: orc.fr_from_ints(cc[k]) if len(cc[k]) else np.zeros((0, 4), dtype=np.uint64) for k in zkp.CIRCUIT_POLYS}
    proofs = []
    for glv in (True, False):
        srs = zkp.Srs.new_from_secret(orc.fr_from_ints([secret])[0], n)
        srs.bases.precompute(9, glv=glv)
        assert srs.bases.expansion()["glv"] == int(glv)
        pr = zkp.PlonkProver(srs.bases, n.bit_length() - 1, polys, orc.fr_from_ints([cc["k1"]])[0], orc.fr_from_ints([cc["k2"]])[0])
        proof = pr.prove(orc.fr_from_ints(blinders))
        assert pr.verify(g2_from_ints(PairM.g2_mul(PairM.G2, secret)), proof) == 1
        proofs.append(proof)
        pr.close()
    a, b = proofs
    assert a["degree"] == b["degree"] and np.array_equal(a["u"], b["u"]) and np.array_equal(a["bars"], b["bars"])
    for k in a["commits"]:
        assert a["commits"][k][1] == b["commits"][k][1] and np.array_equal(a["commits"][k][0], b["commits"][k][0]), k


def test_nova_fold_over_a_split_srs(zkp):
    import nova_model as NM
    r1cs_m, ws, xs = NM.gen_test_values([3, 4])
    fr = lambda rows: [NM.fr_limbs(r) for r in rows]
    res = []
    for glv in (True, False):
        srs = zkp.Srs.new_from_secret(NM.fr_limbs([0x1F2E3D4C5B6A7988])[0], 4 + 1 + 1)
        srs.bases.precompute(9, glv=glv)
        scheme = zkp.KzgScheme(srs, expand_bases=False)
        r1cs = zkp.NovaR1CS.from_dense(scheme, fr(r1cs_m["a"]), fr(r1cs_m["b"]), fr(r1cs_m["c"]), 4, 1)
        fw = [zkp.FWitness.new(dev(np.asarray(NM.fr_limbs(w), dtype=np.uint64)), 4) for w in ws]
        fi = [f.commit(scheme, NM.fr_limbs(x)) for f, x in zip(fw, xs)]
        fw3, fi3, com_t, r = zkp.nifs_prover(r1cs, fw[0], fw[1], fi[0], fi[1], zkp.NovaTranscript())
        res.append([fi[0].com_w, fi[1].com_w, fi[0].com_e, com_t, fi3.com_w, fi3.com_e, (np.asarray(r), 0)])
    for a, b in zip(*res):
        assert a[1] == b[1] and np.array_equal(np.asarray(a[0], dtype=np.uint64), np.asarray(b[0], dtype=np.uint64))
    assert res[0][3][1] == 0 and res[0][4][1] == 0  # the cross term and the folded witness commit to finite points
