"""GPU: Nova folding (zkp_nova_*) against the big-int model of nova/src (tests/model/nova_model.py): the reference's own example
(test_one_fold, test_prover_folding), the cross-term kernel on random sparse R1CS that exercise both row paths and their boundary,
an 8-fold chain folded in place, the device openings against zkp_kzg_open, and one 2^20-row fold checked through the SRS trapdoor."""
import numpy as np
import pytest

import bigmodel as M
import nova_model as NM

pytestmark = pytest.mark.gpu
R = M.R
SECRET = 0x1F2E3D4C5B6A7988
_RINV = pow(1 << 256, -1, R)


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available()
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


def ints(a):
    """(n, 4) uint64 Montgomery limbs -> canonical ints (vectorised enough for 2^20 elements)."""
    b = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") * _RINV % R for i in range(0, len(b), 32)]


def dlog_of(vec_limbs):
    """commit_vector in the exponent: v(s) for the SRS secret."""
    return M.poly_eval(ints(vec_limbs), SECRET, R)


def same_point(zkp, got, dlog):
    exp = zkp.g1_mul(NM.g1_abi(M.G1)[0], 0, NM.fr_limbs([dlog])[0])
    assert got[1] == exp[1] and (exp[1] or np.array_equal(np.asarray(got[0], dtype=np.uint64), exp[0]))


def make_scheme(zkp, n):
    return zkp.KzgScheme(zkp.Srs.new_from_secret(NM.fr_limbs([SECRET])[0], n))


def g2s(zkp):
    return zkp.g2_mul(zkp.g2_generator(), NM.fr_limbs([SECRET])[0])[0]


# ----------------------------------------------------------------------------- the reference's example
def test_reference_one_fold(zkp):
    r1cs_m, ws, xs = NM.gen_test_values([3, 4])
    scheme = make_scheme(zkp, 4 + 1 + 1)  # domain_size = |W| + |x| + 1 (nifs_verifier.rs:162)
    fr = lambda rows: [NM.fr_limbs(r) for r in rows]
    r1cs = zkp.NovaR1CS.from_dense(scheme, fr(r1cs_m["a"]), fr(r1cs_m["b"]), fr(r1cs_m["c"]), 4, 1)
    fw = [zkp.FWitness.new(dev(NM.fr_limbs(w)), 4) for w in ws]
    fi = [f.commit(scheme, NM.fr_limbs(x)) for f, x in zip(fw, xs)]
    mfw = [{"e": [0] * 4, "w": w} for w in ws]
    mfi = [NM.instance(f, x, SECRET) for f, x in zip(mfw, xs)]
    for k in range(2):
        same_point(zkp, fi[k].com_e, mfi[k]["com_e"])
        same_point(zkp, fi[k].com_w, mfi[k]["com_w"])
        assert zkp.is_r1cs_satisfied(r1cs, fi[k], fw[k], scheme)

    # T alone, bit-exact
    t = dev(np.zeros((4, 4), dtype=np.uint64))
    r1cs.cross_term_dev(fw[0].w, fi[0].x, fi[0].u, fw[1].w, fi[1].x, fi[1].u, t)
    z1, z2 = NM.z_vector(ws[0], xs[0], 1), NM.z_vector(ws[1], xs[1], 1)
    assert ints(host(t)) == NM.compute_t(r1cs_m, 1, 1, z1, z2)

    # NIFS::prover on the device against the model
    mtr = NM.Transcript()
    mfw3, mfi3, mcom_t, mr, _ = NM.prover(r1cs_m, mfw[0], mfw[1], mfi[0], mfi[1], SECRET, mtr)
    tr = zkp.NovaTranscript()
    fw3, fi3, com_t, r = zkp.nifs_prover(r1cs, fw[0], fw[1], fi[0], fi[1], tr)
    assert ints([r])[0] == mr
    same_point(zkp, com_t, mcom_t)
    same_point(zkp, fi3.com_e, mfi3["com_e"])
    same_point(zkp, fi3.com_w, mfi3["com_w"])
    assert ints(host(fw3.e)) == mfw3["e"] and ints(host(fw3.w)) == mfw3["w"]
    assert ints([fi3.u])[0] == mfi3["u"] and ints(fi3.x) == mfi3["x"]
    assert r1cs.relaxed_residual(fw3.w, fi3.x, fi3.u, fw3.e) == 0
    assert NM.residual_rows(r1cs_m, mfw3["w"], mfi3["x"], mfi3["u"], mfw3["e"]) == 0
    assert zkp.is_r1cs_satisfied(r1cs, fi3, fw3, scheme)

    # NIFS::prove + NIFS::verify
    proof = zkp.nifs_prove(r1cs, r, fw3, fi3, tr)
    mproof = NM.prove(mr, mfw3, mfi3, SECRET, mtr)
    assert ints([proof.opening_point])[0] == mproof["opening_point"]
    assert ints([proof.opening_e[1]])[0] == mproof["opening_e"][1] and ints([proof.opening_w[1]])[0] == mproof["opening_w"][1]
    same_point(zkp, proof.opening_e[0], mproof["opening_e"][0])
    same_point(zkp, proof.opening_w[0], mproof["opening_w"][0])
    assert zkp.nifs_verify(g2s(zkp), proof, fi[0], fi[1], fi3, com_t, zkp.NovaTranscript()) == 1

    # the host-pointer forms give the same
    htr = zkp.NovaTranscript()
    hfw = [zkp.FWitness(host(f.e), host(f.w)) for f in fw]
    hfw3, hfi3, hcom_t, hr = zkp.nifs_prover(r1cs, hfw[0], hfw[1], fi[0], fi[1], htr)
    assert np.array_equal(hr, r) and np.array_equal(hcom_t[0], com_t[0]) and np.array_equal(hfi3.com_e[0], fi3.com_e[0])
    assert np.array_equal(hfw3.e, host(fw3.e)) and np.array_equal(hfw3.w, host(fw3.w))
    hproof = zkp.nifs_prove(r1cs, hr, hfw3, hfi3, htr)
    assert np.array_equal(hproof.opening_e[0][0], proof.opening_e[0][0]) and np.array_equal(hproof.opening_w[1], proof.opening_w[1])


# ----------------------------------------------------------------------------- random sparse R1CS
def random_r1cs(orc, rows, nv, nio, seed):
    """Three CSR matrices, about one entry per row each, with: empty rows, rows of 1, 4, 63, 64, 65 and 2048 / 3000 entries in all
    (both kernels and their boundary at NOVA_LONG_ROW = 64), duplicate (row, column) entries, and columns on the x and u slots."""
    rng = np.random.default_rng(seed)
    ncols = nv + nio + 1
    lens = [rng.integers(0, 3, rows) for _ in range(3)]  # 0..2 per matrix: ~3 per row
    special = {3: (1, 0, 0), 5: (0, 4, 0), 7: (63, 0, 0), 9: (0, 0, 64), 11: (65, 0, 0), 13: (30, 20, 15), 17: (2048, 0, 0),
               19: (1000, 1000, 1000), 21: (0, 0, 0), 23: (0, 0, 0)}
    for i, ls in special.items():
        for k in range(3):
            lens[k][i] = ls[k]
    mats = []
    for k in range(3):
        rp = np.zeros(rows + 1, dtype=np.uint64)
        rp[1:] = np.cumsum(lens[k])
        nnz = int(rp[-1])
        cols = rng.integers(0, ncols, nnz).astype(np.uint32)
        starts = rp[:-1][lens[k] >= 2].astype(np.int64)
        dup = starts[rng.random(len(starts)) < 0.3]
        cols[dup + 1] = cols[dup]                               # duplicate entries
        hit = rng.choice(nnz, size=min(nnz, 64), replace=False)
        cols[hit[:32]] = nv + rng.integers(0, nio, 32)          # x slots
        cols[hit[32:]] = nv + nio                               # u slot
        vals = orc.rand_fr(seed * 7 + k, nnz)
        vals[rng.random(nnz) < 0.02] = 0                        # explicit zeros
        mats.append((rp, cols, vals))
    return mats


def model_mats(mats):
    return [(list(map(int, rp)), list(map(int, cols)), ints(vals)) for rp, cols, vals in mats]


@pytest.mark.parametrize("log_rows", [10, 16])
def test_cross_term_random_sparse_bit_exact(zkp, orc, log_rows):
    rows = nv = 1 << log_rows
    nio = 3
    mats = random_r1cs(orc, rows, nv, nio, log_rows)
    scheme = make_scheme(zkp, 16)
    r1cs = zkp.NovaR1CS(scheme, rows, nv, nio, *mats)
    w1, w2 = orc.rand_fr(1, nv), orc.rand_fr(2, nv)
    x1, x2 = orc.rand_fr(3, nio), orc.rand_fr(4, nio)
    u1, u2 = orc.rand_fr(5, 1)[0], orc.rand_fr(6, 1)[0]
    t = dev(np.zeros((rows, 4), dtype=np.uint64))
    r1cs.cross_term_dev(dev(w1), x1, u1, dev(w2), x2, u2, t)
    mm = model_mats(mats)
    z1 = NM.z_vector(ints(w1), ints(x1), ints([u1])[0])
    z2 = NM.z_vector(ints(w2), ints(x2), ints([u2])[0])
    exp = NM.compute_t_csr(mm, ints([u1])[0], ints([u2])[0], z1, z2)
    got = ints(host(t))
    bad = [i for i in range(rows) if got[i] != exp[i]]
    assert not bad, f"{len(bad)} rows differ, first {bad[:8]}"
    # the residual kernel on an instance satisfied by construction (E = A z o B z - u C z), then with one row broken per path
    e = [(a * b - ints([u1])[0] * c) % R for a, b, c in zip(*(NM.csr_matvec(m, z1) for m in mm))]
    e_l = NM.fr_limbs(e)
    assert r1cs.relaxed_residual(dev(w1), x1, u1, dev(e_l)) == 0
    e_l[7] = NM.fr_limbs([e[7] + 1])[0]     # a short row
    e_l[19] = NM.fr_limbs([e[19] + 1])[0]   # a long row
    assert r1cs.relaxed_residual(dev(w1), x1, u1, dev(e_l)) == 2


# ----------------------------------------------------------------------------- folding chains
HALF = NM.fr_limbs([pow(2, -1, R)])[0]


def satisfied_pair(zkp, r1cs, scheme, w, x, u):
    """A relaxed instance satisfied by construction, built on the device: T(z, z, u, u) = 2 (A z o B z - u C z), so
    E = fold(0, T, 0; r = 1/2) = A z o B z - u C z."""
    import torch
    rows = r1cs.rows
    t = torch.zeros(rows * 4, dtype=torch.int64, device="cuda")
    r1cs.cross_term_dev(w, x, u, w, x, u, t)
    zero_e = torch.zeros_like(t)
    e = torch.zeros_like(t)
    w_copy = torch.empty_like(w)
    r1cs.fold_witness_dev(HALF, zero_e, w, zero_e, torch.zeros_like(w), t, e, w_copy)
    fw = zkp.FWitness(e, w_copy)
    fi = fw.commit(scheme, x)
    fi.u = np.asarray(u, dtype=np.uint64).copy()
    return fw, fi


def test_fold_chain_in_place_stays_satisfied(zkp, orc):
    rows = nv = 1 << 12
    nio = 2
    mats = random_r1cs(orc, rows, nv, nio, 12)
    scheme = make_scheme(zkp, rows)
    r1cs = zkp.NovaR1CS(scheme, rows, nv, nio, *mats)
    run_w, run_i = satisfied_pair(zkp, r1cs, scheme, dev(orc.rand_fr(100, nv)), orc.rand_fr(101, nio), orc.rand_fr(102, 1)[0])
    assert zkp.is_r1cs_satisfied(r1cs, run_i, run_w, scheme)
    e_ptr = run_w.e.data_ptr()
    tr = zkp.NovaTranscript()
    for k in range(8):
        w_k, i_k = satisfied_pair(zkp, r1cs, scheme, dev(orc.rand_fr(200 + k, nv)), orc.rand_fr(300 + k, nio), orc.rand_fr(400 + k, 1)[0])
        run_w, run_i, com_t, r = zkp.nifs_prover(r1cs, run_w, w_k, run_i, i_k, tr, inplace=True)
        assert run_w.e.data_ptr() == e_ptr  # the running instance's buffers were the kernel's output
        assert r1cs.relaxed_residual(run_w.w, run_i.x, run_i.u, run_w.e) == 0, f"fold {k}"
    assert zkp.is_r1cs_satisfied(r1cs, run_i, run_w, scheme)
    # prove: the openings are zkp_kzg_open's on the same vectors (E: the device path of kzg_open, len >= 4096)
    proof = zkp.nifs_prove(r1cs, r, run_w, run_i, tr)
    for vec, (pt, ev) in ((host(run_w.e), proof.opening_e), (host(run_w.w), proof.opening_w)):
        kpt, kev = zkp.kzg_open(scheme.srs.bases, vec, proof.opening_point)
        assert kpt[1] == pt[1] and np.array_equal(kpt[0], pt[0]) and np.array_equal(kev, ev)
    # a broken entry of E is seen by the residual
    bad = run_w.e.clone()
    bad[4 * 1000] += 1
    assert r1cs.relaxed_residual(run_w.w, run_i.x, run_i.u, bad) == 1


def test_open_of_zero_e_matches_kzg_open(zkp, orc):
    rows = nv = 256
    mats = random_r1cs(orc, rows, nv, 1, 3)
    scheme = make_scheme(zkp, rows)
    r1cs = zkp.NovaR1CS(scheme, rows, nv, 1, *mats)
    fw = zkp.FWitness.new(dev(orc.rand_fr(9, nv)), rows)  # E = 0: the trimmed E is empty
    fi = fw.commit(scheme, orc.rand_fr(10, 1))
    assert fi.com_e[1] == 1
    tr = zkp.NovaTranscript()
    tr.feed_scalar_num(orc.rand_fr(11, 1)[0])
    proof = zkp.nifs_prove(r1cs, orc.rand_fr(12, 1)[0], fw, fi, tr)
    kpt, kev = zkp.kzg_open(scheme.srs.bases, host(fw.e), proof.opening_point)
    assert proof.opening_e[0][1] == kpt[1] == 1 and np.array_equal(proof.opening_e[1], kev) and not kev.any()
    wpt, wev = zkp.kzg_open(scheme.srs.bases, host(fw.w), proof.opening_point)
    assert np.array_equal(proof.opening_w[0][0], wpt[0]) and np.array_equal(proof.opening_w[1], wev)


def test_fold_2e20_rows(zkp, orc):
    rows = nv = 1 << 20
    nio = 2
    rng = np.random.default_rng(20)
    mats = []
    for k in range(3):  # one entry per row in each matrix, plus a few rows of 1024 entries in A
        lens = np.ones(rows, dtype=np.int64)
        if k == 0:
            lens[rng.choice(rows, 8, replace=False)] = 1024
        rp = np.zeros(rows + 1, dtype=np.uint64)
        rp[1:] = np.cumsum(lens)
        nnz = int(rp[-1])
        mats.append((rp, rng.integers(0, nv + nio + 1, nnz).astype(np.uint32), orc.rand_fr(50 + k, nnz)))
    scheme = make_scheme(zkp, rows)
    r1cs = zkp.NovaR1CS(scheme, rows, nv, nio, *mats)
    fw1, fi1 = satisfied_pair(zkp, r1cs, scheme, dev(orc.rand_fr(60, nv)), orc.rand_fr(61, nio), orc.rand_fr(62, 1)[0])
    fw2, fi2 = satisfied_pair(zkp, r1cs, scheme, dev(orc.rand_fr(63, nv)), orc.rand_fr(64, nio), orc.rand_fr(65, 1)[0])
    tr = zkp.NovaTranscript()
    fw3, fi3, com_t, r = zkp.nifs_prover(r1cs, fw1, fw2, fi1, fi2, tr)
    assert r1cs.relaxed_residual(fw3.w, fi3.x, fi3.u, fw3.e) == 0
    same_point(zkp, fi3.com_e, dlog_of(host(fw3.e)))
    same_point(zkp, fi3.com_w, dlog_of(host(fw3.w)))
    proof = zkp.nifs_prove(r1cs, r, fw3, fi3, tr)
    assert zkp.nifs_verify(g2s(zkp), proof, fi1, fi2, fi3, com_t, zkp.NovaTranscript()) == 1
