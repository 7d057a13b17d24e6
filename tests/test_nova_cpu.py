"""CPU: the host half of Nova folding -- the transcript (nova/src/transcript.rs), NIFS::verify (nifs_verifier.rs:22-91) on proofs made
by the big-int model with a known SRS secret, the R1CS matrix validation of zkp_nova_r1cs_create, and the dense -> CSR conversion of
the Python layer.  No device is used: these entries are host code."""
import os

import numpy as np
import pytest

import bigmodel as M
import nova_model as NM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R


@pytest.fixture(scope="module")
def zkp():
    import importlib.util
    spec = importlib.util.spec_from_file_location("zkp_build", os.path.join(ROOT, "zkp-implementation_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    import zkp_hip
    return zkp_hip


def test_transcript_matches_model_on_mixed_feeds(zkp):
    pts = [NM.point(d) for d in (1, 2, 0xC0FFEE)] + [None]
    scalars = [0, 1, 15, 20, R - 1, 0x1234567890ABCDEF1234567890ABCDEF]
    t, m = zkp.NovaTranscript(), NM.Transcript()
    order = [("s", 0), ("p", 0), ("s", 1), ("s", 2), ("p", 3), ("p", 1), ("s", 4), ("s", 5), ("p", 2)]
    for i, (kind, k) in enumerate(order):
        if kind == "s":
            t.feed_scalar_num(NM.fr_limbs([scalars[k]])[0])
            m.feed_scalar_num(scalars[k])
        else:
            t.feed(NM.g1_abi(pts[k]))
            m.feed(pts[k])
        if i in (2, 5, 8):
            n = 1 + i // 3
            assert NM.fr_ints(t.generate_challenges(n)) == m.generate_challenges(n)


def test_transcript_refuses_to_draw_twice(zkp):
    t = zkp.NovaTranscript()
    with pytest.raises(zkp.ZkpError) as e:
        t.generate_challenges(1)  # nothing fed yet
    assert e.value.code == zkp.ZKP_E_ARG
    t.feed_scalar_num(NM.fr_limbs([15])[0])
    t.generate_challenges(3)
    with pytest.raises(zkp.ZkpError) as e:
        t.generate_challenges(1)
    assert e.value.code == zkp.ZKP_E_ARG and "hungry" in str(e.value)
    t.feed(NM.g1_abi(NM.point(7)))
    assert t.generate_challenges(1).shape == (1, 4)


def _abi_instance(zkp, fi):
    return zkp.FInstance(NM.g1_abi(NM.point(fi["com_e"])), NM.fr_limbs([fi["u"]])[0], NM.g1_abi(NM.point(fi["com_w"])),
                         NM.fr_limbs(fi["x"]))


def _abi_proof(zkp, p):
    return zkp.NifsProof(NM.fr_limbs([p["r"]])[0], NM.fr_limbs([p["opening_point"]])[0],
                         (NM.g1_abi(NM.point(p["opening_e"][0])), NM.fr_limbs([p["opening_e"][1]])[0]),
                         (NM.g1_abi(NM.point(p["opening_w"][0])), NM.fr_limbs([p["opening_w"][1]])[0]))


@pytest.fixture(scope="module")
def model_fold():
    """test_one_fold (nifs_verifier.rs:150-200) in the model, SRS secret s known."""
    s = 0x5EC12E7
    r1cs, ws, xs = NM.gen_test_values([3, 4])
    fw = [{"e": [0] * 4, "w": w} for w in ws]
    fi = [NM.instance(f, x, s) for f, x in zip(fw, xs)]
    tr = NM.Transcript()
    fw3, fi3, com_t, r, _t = NM.prover(r1cs, fw[0], fw[1], fi[0], fi[1], s, tr)
    proof = NM.prove(r, fw3, fi3, s, tr)
    assert NM.is_r1cs_satisfied(r1cs, fi3, fw3, s)
    return dict(s=s, fi1=fi[0], fi2=fi[1], fi3=fi3, com_t=com_t, proof=proof)


def _verify(zkp, mf, proof=None, com_t=None, fi3=None):
    g2s = zkp.g2_mul(zkp.g2_generator(), NM.fr_limbs([mf["s"]])[0])[0]
    return zkp.nifs_verify(g2s, _abi_proof(zkp, proof or mf["proof"]), _abi_instance(zkp, mf["fi1"]), _abi_instance(zkp, mf["fi2"]),
                           _abi_instance(zkp, fi3 or mf["fi3"]), NM.g1_abi(NM.point(mf["com_t"] if com_t is None else com_t)),
                           zkp.NovaTranscript())


def test_verify_accepts_model_proof(zkp, model_fold):
    assert _verify(zkp, model_fold) == 1


def test_verify_rejects_each_change_with_its_reason(zkp, model_fold):
    mf = model_fold
    p = dict(mf["proof"])
    assert _verify(zkp, mf, proof=dict(p, r=(p["r"] + 1) % R)) == -1                           # random r
    assert _verify(zkp, mf, com_t=(mf["com_t"] + 1) % R) == -1                                 # com_T changes r
    assert _verify(zkp, mf, proof=dict(p, opening_point=(p["opening_point"] + 1) % R)) == -2   # opening point
    ow, ew = p["opening_w"]
    assert _verify(zkp, mf, proof=dict(p, opening_w=(ow, (ew + 1) % R))) == 0                  # folding wrong at W
    oe, ee = p["opening_e"]
    assert _verify(zkp, mf, proof=dict(p, opening_e=((oe + 1) % R, ee))) == -3                 # folding wrong at E
    assert zkp.nova.VERIFY_RESULTS[-3] == "Verify: Folding wrong at E"


def zkp_csr_from(rows, entries):
    """(row, column) entries -> CSR with value 1 each"""
    from zkp_hip import nova
    ones = NM.fr_limbs([1] * len(entries))
    return nova.csr_from_triplets(rows, [e[0] for e in entries], [e[1] for e in entries], ones)


def _create_error(zkp, a, b, c, rows=3, nv=2, nio=1):
    with pytest.raises(zkp.ZkpError) as e:
        zkp.NovaR1CS(None, rows, nv, nio, a, b, c)
    assert e.value.code == zkp.ZKP_E_ARG
    return str(e.value)


def test_r1cs_validation_errors(zkp):
    good = zkp_csr_from(3, [(0, 0), (1, 3), (2, 1)])  # column 3 = u (num_vars 2 + num_io 1)
    bad_col = zkp_csr_from(3, [(0, 0), (1, 4)])
    assert "column 4" in _create_error(zkp, good, bad_col, good) and "matrix B" in _create_error(zkp, good, bad_col, good)
    rp, cl, vl = good
    down = (np.array([0, 2, 1, 3], dtype=np.uint64), cl, vl)
    assert "decreases" in _create_error(zkp, good, good, down)
    shifted = (np.array([1, 2, 3, 3], dtype=np.uint64), cl, vl)
    assert "row_ptr[0]" in _create_error(zkp, shifted, good, good)
    assert "null argument (matrix A)" in _create_error(zkp, (rp, None, None), good, good)
    assert "at least one row" in _create_error(zkp, good, good, good, nv=0)
    # a valid R1CS gets past validation and stops at the missing SRS (the handle itself needs a device)
    assert "null argument (srs)" in _create_error(zkp, good, good, good)


def test_dense_to_csr_handles_ragged_rows_zeros_and_duplicates(zkp):
    from zkp_hip import nova
    dense = [[1, 0, 5], [], [0, 0, 0, 7], [2, 3, 0, 0, 0, 0, 9]]  # ragged; the last row reaches past z (6 columns)
    ncols = 6
    rp, cols, vals = nova.csr_from_dense([NM.fr_limbs(r) for r in dense], ncols)
    assert list(rp) == [0, 2, 2, 3, 5] and list(cols) == [0, 2, 3, 0, 1]
    assert NM.fr_ints(vals) == [1, 5, 7, 2, 3]
    z = [11, 12, 13, 14, 15, 16]
    assert NM.csr_matvec((list(map(int, rp)), list(map(int, cols)), NM.fr_ints(vals)), z) == NM.matrix_vector_product(dense, z)
    # triplets: duplicates and explicit zeros are kept and add up as the dense sum would
    rp, cols, vals = nova.csr_from_triplets(3, [2, 0, 2, 0, 1], [1, 0, 1, 2, 0], NM.fr_limbs([4, 1, 6, 0, 8]))
    assert list(rp) == [0, 2, 3, 5] and list(cols) == [0, 2, 0, 1, 1]
    got = NM.csr_matvec((list(map(int, rp)), list(map(int, cols)), NM.fr_ints(vals)), [3, 5, 7])
    assert got == [3, 24, 50]
