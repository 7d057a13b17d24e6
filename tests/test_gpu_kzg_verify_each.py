"""GPU: a verdict per opening on the point verifier (zkp_kzg_verify_points_each / _dev, KzgPointVerifier.verify_each,
KzgScheme.verify_points_each).  70 openings over 3 commitments from the big-int model's kzg_open, the openings {0, 5, 64, 69} made
wrong three different ways (y, z, W): the verdict bytes equal the expected vector index by index (the second wave holds six live
lanes, two of them wrong), n_bad = 4, and the lowest zero is what zkp_kzg_verify_points_find_bad returns for the same batch.  An
all-good batch gives all ones; the identity proof of a constant polynomial is accepted.  No test provokes a fault."""
import random

import numpy as np
import pytest

import bigmodel as M
import pairing_model as PM

pytestmark = pytest.mark.gpu
R = M.R
SECRET = 0x1F2E3D4C5B6A7988
N, POLYS, DEGREE = 70, 3, 4
WRONG = {0: "y", 5: "z", 64: "w", 69: "y"}


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).cuda()


@pytest.fixture(scope="module")
def batch(orc):
    """The honest batch, computed once by the model and left unchanged: opening i is of polynomial i mod 3"""
    rng = random.Random(0xEAC4)
    pts = M.srs(SECRET, DEGREE)
    polys = [[rng.randrange(R) for _ in range(DEGREE)] for _ in range(POLYS)]
    index = [i % POLYS for i in range(N)]
    zs = [rng.randrange(R) for _ in range(N)]
    ws, ys = zip(*(M.kzg_open(polys[m], z, pts) for m, z in zip(index, zs)))
    assert all(w is not None for w in ws)
    commits, cinf = orc.points_from_ints([M.msm_naive(f, pts) for f in polys])
    proofs, pinf = orc.points_from_ints(list(ws))
    assert not cinf.any() and not pinf.any()
    return {"commits": commits, "proofs": proofs, "ws": list(ws), "zs": zs, "ys": list(ys), "index": np.array(index, dtype=np.uint32)}


def tampered(orc, batch):
    zs, ys, proofs = list(batch["zs"]), list(batch["ys"]), batch["proofs"].copy()
    for i, how in WRONG.items():
        if how == "y":
            ys[i] = (ys[i] + 1) % R
        elif how == "z":
            zs[i] = (zs[i] + 1) % R
        else:
            proofs[i] = orc.points_from_ints([M.g1_mul(batch["ws"][i], 2)])[0][0]   # a point of G1, not the proof
    return orc.fr_from_ints(zs), orc.fr_from_ints(ys), proofs


@pytest.fixture(scope="module")
def verifier(zkp, orc):
    import zkp_hip.kzg_points as kp
    g2s = zkp.g2_mul(zkp.g2_generator(), orc.fr_from_ints([SECRET])[0])[0]
    v = kp.KzgPointVerifier(g2s, 128, 128)
    yield v
    v.close()


def test_wrong_openings_are_named_index_by_index(zkp, orc, batch, verifier):
    import torch
    zs, ys, proofs = tampered(orc, batch)
    want = [0 if i in WRONG else 1 for i in range(N)]
    ok, n_bad = verifier.verify_each(batch["commits"], zs, ys, proofs, commit_index=batch["index"])
    assert ok.tolist() == want and n_bad == 4
    d_ok = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
    n_bad = verifier.verify_each_dev(dev(batch["commits"]), POLYS, N, dev(zs), dev(ys), dev(proofs), d_ok, commit_index=batch["index"])
    assert d_ok.cpu().numpy().tolist() == want and n_bad == 4
    weights = orc.fr_from_ints([random.Random(50 + i).randrange(1, 1 << 128) for i in range(N)])
    assert verifier.find_bad(batch["commits"], zs, ys, proofs, weights, commit_index=batch["index"]) == want.index(0) == 0
    # with opening 0 honest the lowest failing opening moves to 5 in both
    ys2 = ys.copy()
    ys2[0] = orc.fr_from_ints([batch["ys"][0]])[0]
    ok, n_bad = verifier.verify_each(batch["commits"], zs, ys2, proofs, commit_index=batch["index"])
    assert n_bad == 3 and ok.tolist().index(0) == 5 == verifier.find_bad(batch["commits"], zs, ys2, proofs, weights, commit_index=batch["index"])


def test_all_good_batch_and_the_identity_index(zkp, orc, batch, verifier):
    zs, ys = orc.fr_from_ints(batch["zs"]), orc.fr_from_ints(batch["ys"])
    ok, n_bad = verifier.verify_each(batch["commits"], zs, ys, batch["proofs"], commit_index=batch["index"])
    assert ok.tolist() == [1] * N and n_bad == 0
    # no index: opening i against its own copy of its commitment, 65 of them (a second wave of one lane)
    own = np.ascontiguousarray(batch["commits"][batch["index"][:65]])
    ys_bad = ys[:65].copy()
    ys_bad[64] = orc.fr_from_ints([(batch["ys"][64] + 1) % R])[0]
    ok, n_bad = verifier.verify_each(own, zs[:65], ys_bad, batch["proofs"][:65])
    assert ok.tolist() == [1] * 64 + [0] and n_bad == 1


def test_identity_proof_of_a_constant_polynomial(zkp, orc, verifier):
    """f = c: the commitment is [c]G, every value is c and the proof is the identity, at any z; z = 0 and y = 0 take the lanes'
    short cuts"""
    c = 0xC0175A17
    commits, _ = orc.points_from_ints([M.g1_mul(M.G1, c), M.g1_mul(M.G1, 5)])
    proofs = np.zeros((4, 12), dtype=np.uint64)
    pinf = np.array([1, 1, 1, 0], dtype=np.uint8)
    # opening 3: the constant 5 at z = 0 with y = 5 but a finite point, G, where the identity proof belongs
    proofs[3] = orc.points_from_ints([M.G1])[0][0]
    zs = orc.fr_from_ints([12345, 0, 99, 0])
    ys = orc.fr_from_ints([c, c, (c + 1) % R, 5])
    ok, n_bad = verifier.verify_each((commits, np.zeros(2, dtype=np.uint8)), zs, ys, (proofs, pinf), commit_index=np.array([0, 0, 0, 1], dtype=np.uint32))
    # 2: the wrong value; 3: the left point is C - [5]G = O, but e(-G, [s]_2) != 1
    assert ok.tolist() == [1, 1, 0, 0] and n_bad == 2
    # the identity as a commitment: f = 0, y = 0, W = O
    ok, n_bad = verifier.verify_each((commits[:1], np.ones(1, dtype=np.uint8)), orc.fr_from_ints([7]), orc.fr_from_ints([0]),
                                     (np.zeros((1, 12), dtype=np.uint64), np.ones(1, dtype=np.uint8)))
    assert ok.tolist() == [1] and n_bad == 0


def test_scheme_method_and_refusals(zkp, orc, batch, verifier):
    zs, ys, proofs = tampered(orc, batch)
    scheme = zkp.KzgScheme.__new__(zkp.KzgScheme)     # the method needs no SRS
    g2s = zkp.g2_mul(zkp.g2_generator(), orc.fr_from_ints([SECRET])[0])[0]
    ok, n_bad = scheme.verify_points_each(g2s, batch["commits"], zs[:6], ys[:6], proofs[:6], commit_index=batch["index"][:6])
    assert ok.tolist() == [0, 1, 1, 1, 1, 0] and n_bad == 2
    scheme._point_verifier[1].close()
    assert verifier.verify_each(batch["commits"], zs[:0], ys[:0], proofs[:0], commit_index=batch["index"][:0])[1] == 0
    with pytest.raises(zkp.ZkpError) as ei:   # a commitment index out of range, before anything is launched
        verifier.verify_each(batch["commits"], zs[:2], ys[:2], proofs[:2], commit_index=np.array([0, 3], dtype=np.uint32))
    assert ei.value.code == zkp.ZKP_E_ARG
    with pytest.raises(zkp.ZkpError) as ei:   # more openings than the verifier was made for
        verifier.verify_each(np.zeros((129, 12), dtype=np.uint64), np.zeros((129, 4), dtype=np.uint64), np.zeros((129, 4), dtype=np.uint64),
                             np.zeros((129, 12), dtype=np.uint64))
    assert ei.value.code == zkp.ZKP_E_SIZE
    off = proofs.copy()
    off[3, 6] ^= np.uint64(1)
    with pytest.raises(zkp.ZkpError) as ei:   # validated as zkp_kzg_verify_points validates
        verifier.verify_each(batch["commits"], zs, ys, off, commit_index=batch["index"])
    assert ei.value.code == zkp.ZKP_E_ARG and "proofs[3]" in str(ei.value)
