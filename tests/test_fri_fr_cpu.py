"""Host-only pieces of FRI over BLS12-381 Fr (no GPU needed): transcript replay and verifier against the independent
big-int model, the reference's field-independent known answers restated in Fr, and the device entries' ZKP_E_DEVICE."""
import numpy as np
import pytest

import bigmodel as M
import fri_fr_model as F

R = M.R


@pytest.fixture(scope="module")
def zkp():
    import zkp_hip
    zkp_hip.lib()
    return zkp_hip


def mem(vals):
    return np.array(F.to_mem(vals), dtype=np.uint64).reshape(-1, 4)


def test_display_boundaries(zkp):
    """Display of 0, r - 1 (77 digits), 10^76 and the 55/56-digit block boundary, as digested by the library's transcript"""
    assert F.display(0) == b"" and F.display(0, True) == b"0"
    assert len(F.display(R - 1)) == 77 and F.display(10 ** 76) == b"1" + b"0" * 76
    for v in (0, 1, R - 1, 10 ** 76, 10 ** 15 - 1, 10 ** 15, 10 ** 54, 10 ** 55):
        r, q = zkp.fri_challenges_fr(mem([v]), F.limbs(v), 2)
        t = F.FriTranscript()
        t.digest(v)
        want = t.challenge()
        t.digest(v)
        assert F.from_mem(r) == [want] and [int(x) for x in q] == t.challenge_list_usize(2)


def test_challenges_match_model(zkp):
    roots = [5, 0, R - 1, 10 ** 76, 123456789]
    const = 77
    r, q = zkp.fri_challenges_fr(mem(roots), F.limbs(const), 6)
    t = F.FriTranscript()
    want_r = []
    for x in roots:
        t.digest(x)
        want_r.append(t.challenge())
    t.digest(const)
    assert F.from_mem(r) == want_r
    assert [int(v) for v in q] == t.challenge_list_usize(6)


@pytest.mark.parametrize("coeffs,blowup,nq", [([1, 2, 3, 4], 2, 2), ([1, 2, 3, 4, 5, 6], 2, 2), ([5], 1, 3), ([5], 2, 1),
                                              (list(range(1, 40)), 4, 5), ([R - 1, 0, 10 ** 76, 3], 2, 3)])
def test_verify_accepts_model_proofs_and_rejects_tampering(zkp, coeffs, blowup, nq):
    proof = np.array(F.fri_flatten(F.fri_prove(coeffs, blowup, nq)), dtype=np.uint64)
    assert zkp.fri_verify_fr(proof)
    L = int(proof[1])
    with pytest.raises(zkp.ZkpError):
        zkp.fri_verify_fr(proof[:-1])  # truncated
    with pytest.raises(zkp.ZkpError):
        zkp.fri_verify_fr(proof[:2])
    if L == 0:
        return
    rec0 = 3 + 4 * (L + 2)  # first query record
    bad = proof.copy()
    bad[rec0] += np.uint64(1)  # its index
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.fri_verify_fr(bad)
    assert "wrong index!" in str(ei.value)
    bad = proof.copy()
    bad[-4:] = F.limbs((F.from_mem([proof[-4:]])[0] + 1) % R)  # last sibling hash of the last record
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.fri_verify_fr(bad)
    assert "verify Merkle path failed!" in str(ei.value)
    bad = proof.copy()
    bad[3 + 4:3 + 8] = F.limbs((F.from_mem([proof[3 + 4:3 + 8]])[0] + 1) % R)  # layer-0 root: it also moves the queries
    with pytest.raises(zkp.ZkpError):
        zkp.fri_verify_fr(bad)
    if len(coeffs) == 1:
        return  # a constant folds to itself on any coset
    # a coset the proof was not made for: every path still verifies, the fold check does not
    bad = proof.copy()
    bad[3:7] = F.limbs(11)
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.fri_verify_fr(bad)
    assert "folding wrong!" in str(ei.value)


def test_reference_kats_in_fr(zkp):
    """prover.rs:180-205 restated in Fr: fold([1,2,3,4], r=1) = [3,7]; the layer-1 coset of a 4-point domain is 7^2 = 49.
    The library's verifier squares the coset per layer: it accepts the model's proof and rejects it on the coset 7 sent as 49."""
    assert M.fri_fold([1, 2, 3, 4], 1, mod=R) == [3, 7]
    p = F.fri_prove([1, 2, 3, 4], 1, 1)
    assert p["domain_size"] == 4 and len(p["roots"]) == 2
    ev = F.layer_eval([3, 7], 49, 2)
    assert ev == [(3 + 7 * 49) % R, (3 - 7 * 49) % R]
    proof = np.array(F.fri_flatten(p), dtype=np.uint64)
    assert zkp.fri_verify_fr(proof)
    bad = proof.copy()
    bad[3:7] = F.limbs(49)
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.fri_verify_fr(bad)
    assert "folding wrong!" in str(ei.value)


def test_sym_index_is_index_plus_half_domain(zkp):
    """prover.rs:208-222: the sym index of a query is index + D/2 (mod D).  The library's verifier checks the sym path at
    that index: a proof whose sym evaluation and path belong to index + 1 instead is refused."""
    p = F.fri_prove([1, 2, 3, 4], 1, 1)
    flat = F.fri_flatten(p)
    L = flat[1]
    rec0 = 3 + 4 * (L + 2)
    idx = flat[rec0]
    evals = F.layer_eval([1, 2, 3, 4], 7, 4)
    levels = F.merkle_levels(evals)
    assert p["queries"][0][0][4] == F.merkle_path(levels, (idx + 2) % 4)
    assert zkp.fri_verify_fr(np.array(flat, dtype=np.uint64))
    wrong = (idx + 1) % 4
    bad = list(flat)
    bad[rec0 + 5:rec0 + 9] = F.limbs(evals[wrong])
    bad[rec0 + 9 + 4 * L:rec0 + 9 + 8 * L] = [w for x in F.merkle_path(levels, wrong) for w in F.limbs(x)]
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.fri_verify_fr(np.array(bad, dtype=np.uint64))
    assert "verify Merkle path failed!" in str(ei.value)


def test_device_entries_need_a_device(zkp):
    """Without a GPU every device entry fails with ZKP_E_DEVICE (no CPU fallback)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the device entries run (tests/test_gpu_fri_fr.py)")
    c = mem([1, 2, 3, 4])
    calls = [lambda: zkp.fri_prove_fr(c, 2, 1), lambda: zkp.fri_merkle_tree_fr(c), lambda: zkp.fri_fold_fr(c, F.limbs(1)),
             lambda: zkp.fri_layer_eval_fr(c, F.limbs(7), 3)]
    for f in calls:
        with pytest.raises(zkp.ZkpError) as ei:
            f()
        assert ei.value.code == zkp.ZKP_E_DEVICE


def test_argument_errors_before_the_device(zkp):
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.fri_prove_fr(np.zeros((4, 4), dtype=np.uint64), 2, 1)
    assert ei.value.code == zkp.ZKP_E_ARG
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.fri_prove_fr(mem([1]), 0, 1)
    assert ei.value.code == zkp.ZKP_E_ARG
