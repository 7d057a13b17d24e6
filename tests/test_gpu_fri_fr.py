"""GPU FRI over BLS12-381 Fr (Merkle trees, layer evaluation, fold, generate_proof) against the independent big-int +
hashlib model (tests/model/fri_fr_model.py), through the C ABI."""
import random

import numpy as np
import pytest

import bigmodel as M
import fri_fr_model as F

pytestmark = pytest.mark.gpu
R = M.R


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def mem(vals):
    return np.array(F.to_mem(vals), dtype=np.uint64).reshape(-1, 4)


def canon(rows):
    return F.from_mem(np.asarray(rows).reshape(-1, 4))


# Display lengths at the SHA-256 block boundaries of a leaf message: 55 bytes = 1 block, 56 = 2; r - 1 has 77 digits
SPECIAL = [0, 1, R - 1, 10 ** 76, 10 ** 54, 10 ** 55, 10 ** 54 - 1, 10 ** 55 - 1, 10 ** 19, 10 ** 18 - 1, 2 ** 64, 9]


def leaves_for(n, seed):
    rnd = random.Random(seed)
    vals = [rnd.randrange(R) for _ in range(n)]
    for i, v in enumerate(SPECIAL[:n]):
        vals[(i * 7) % n] = v
    return vals


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 255, 256, 257, 1000, 4096])
def test_merkle_tree_vs_model(zkp, n):
    vals = leaves_for(n, 0x3E2C + n)
    got = zkp.fri_merkle_tree_fr(mem(vals))
    assert got.shape == (zkp.fri_merkle_node_count(n), 4)
    assert canon(got) == [v for lvl in F.merkle_levels(vals) for v in lvl]


def test_zero_display_switch(zkp, monkeypatch):
    """ZKP_FRI_ZERO_AS_0=1 switches Display(0) to "0" for Fr as for Goldilocks."""
    vals = [0, 1, 2, 0, 5]
    default = canon(zkp.fri_merkle_tree_fr(mem(vals)))
    assert default == [v for lvl in F.merkle_levels(vals) for v in lvl]
    coeffs = [0, 0, 3, 0, 7]
    p_default = zkp.fri_prove_fr(mem(coeffs), 2, 2)
    monkeypatch.setenv("ZKP_FRI_ZERO_AS_0", "1")
    switched = canon(zkp.fri_merkle_tree_fr(mem(vals)))
    assert switched == [v for lvl in F.merkle_levels(vals, True) for v in lvl] and switched != default
    p_switched = zkp.fri_prove_fr(mem(coeffs), 2, 2)
    assert [int(x) for x in p_switched] == F.fri_flatten(F.fri_prove(coeffs, 2, 2, zero_as_0=True))
    assert zkp.fri_verify_fr(p_switched)
    with pytest.raises(zkp.ZkpError):
        zkp.fri_verify_fr(p_default)  # made under the other convention


@pytest.mark.parametrize("d,log_d", [(1, 0), (3, 2), (5, 3), (100, 8), (1000, 12)])
def test_layer_eval_and_fold_vs_model(zkp, d, log_d):
    rnd = random.Random(d)
    coeffs = [rnd.randrange(R) for _ in range(d)]
    coset = rnd.randrange(1, R)
    got = canon(zkp.fri_layer_eval_fr(mem(coeffs), F.limbs(coset), log_d))
    assert got == F.layer_eval(coeffs, coset, 1 << log_d)
    r = rnd.randrange(R)
    want = M.fri_fold(coeffs, r, mod=R)
    got = canon(zkp.fri_fold_fr(mem(coeffs), F.limbs(r)))
    assert got[:len(want)] == want and all(v == 0 for v in got[len(want):])


@pytest.mark.parametrize("d,blowup,nq", [(4, 2, 2), (6, 2, 2), (1, 1, 3), (1, 2, 1), (39, 4, 5), (300, 2, 8), (1024, 4, 4),
                                         (600, 4, 3), (1000, 2, 3), (500, 2, 3)])
def test_fri_prove_vs_model(zkp, d, blowup, nq):
    """(500, 2): a 1024-point domain, one layer above the 512-point tail threshold, the 512-point layer first in the tail kernel.
    (600, 4) and (1024, 4): 4096 points, three large layers (the 4096- and 2048-point trees in two Merkle launches each)."""
    coeffs = list(range(1, d + 1)) if d <= 6 else leaves_for(d, 0xF21 + d)
    got = zkp.fri_prove_fr(mem(coeffs), blowup, nq)
    want = F.fri_flatten(F.fri_prove(coeffs, blowup, nq))
    assert [int(x) for x in got] == want
    assert zkp.fri_verify_fr(got)


def test_fri_prove_trailing_zeros_and_zero_polynomial(zkp):
    c = leaves_for(10, 5)
    padded = np.concatenate([mem(c), np.zeros((6, 4), dtype=np.uint64)])
    assert np.array_equal(zkp.fri_prove_fr(padded, 2, 3), zkp.fri_prove_fr(mem(c), 2, 3))
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.fri_prove_fr(np.zeros((4, 4), dtype=np.uint64), 2, 1)
    assert ei.value.code == zkp.ZKP_E_ARG


def test_merkle_tree_dev_large_property(zkp, orc):
    """2^21 leaves (a 2^20-coefficient polynomial at blowup 2): three launches.  Random paths verify with the model's hash, and
    level 11 equals the model's hash_slice over the GPU's level 10."""
    import torch
    n = 1 << 21
    leaves = orc.rand_fr(77, n)
    d_leaves = torch.from_numpy(leaves.view(np.int64)).cuda()
    d_nodes = torch.zeros(zkp.fri_merkle_node_count(n) * 4, dtype=torch.int64, device="cuda")
    zkp.fri_merkle_tree_fr_dev(d_leaves, n, d_nodes)
    torch.cuda.synchronize()
    nodes = d_nodes.cpu().numpy().view(np.uint64).reshape(-1, 4)
    off = [0]
    for l in range(22):
        off.append(off[-1] + (n >> l))
    assert off[22] == nodes.shape[0]
    rnd = np.random.default_rng(3)
    for idx in rnd.integers(0, n, 4):
        cur = int(idx)
        h = F.hash_slice(canon(leaves[cur:cur + 1]))
        for l in range(21):
            assert canon(nodes[off[l] + cur:off[l] + cur + 1])[0] == h
            sib = canon(nodes[off[l] + (cur ^ 1):off[l] + (cur ^ 1) + 1])[0]
            h = F.hash_slice([h, sib] if cur % 2 == 0 else [sib, h])
            cur //= 2
        assert canon(nodes[off[21]:off[21] + 1])[0] == h
    lvl10 = canon(nodes[off[10]:off[11]])
    assert [F.hash_slice(lvl10[2 * j:2 * j + 2]) for j in range(1024)] == canon(nodes[off[11]:off[12]])


def test_fri_prove_large_verifies(zkp, orc):
    """2^20 coefficients at blowup 2 with 32 queries: accepted by fri_verify_fr, rejected once a layer-0 evaluation changes, and
    its layer-0 query evaluations equal the oracle's coset NTT (the oracle is a checker only)."""
    L = 21
    coeffs = orc.rand_fr(0xB16, 1 << 20)
    proof = zkp.fri_prove_fr(coeffs, 2, 32)
    assert int(proof[0]) == 1 << L and int(proof[1]) == L and int(proof[2]) == 32
    assert zkp.fri_verify_fr(proof)
    evals = orc.ntt_fr(np.concatenate([coeffs, np.zeros_like(coeffs)]), coset=np.array(F.limbs(7), dtype=np.uint64))
    p = 3 + 4 * (L + 2)
    for q in range(32):
        idx = int(proof[p])
        assert np.array_equal(proof[p + 1:p + 5], evals[idx])
        assert np.array_equal(proof[p + 5:p + 9], evals[(idx + (1 << 20)) % (1 << 21)])
        for l in range(L):
            p += 1 + 4 * (2 + 2 * (L - l))
    assert p == proof.size
    bad = proof.copy()
    bad[3 + 4 * (L + 2) + 1] ^= np.uint64(1)
    with pytest.raises(zkp.ZkpError):
        zkp.fri_verify_fr(bad)


@pytest.mark.parametrize("tail_log", ["0", "1", "9"])
@pytest.mark.parametrize("d,blowup", [(1000, 2), (39, 4), (3, 2)])
def test_tail_threshold_does_not_change_the_proof(zkp, monkeypatch, d, blowup, tail_log):
    """The tail kernel and the large-layer launches compute the same layers: moving the threshold (0 = no tail) changes
    nothing in the proof."""
    coeffs = leaves_for(d, 0x7A11 + d)
    default = zkp.fri_prove_fr(mem(coeffs), blowup, 3)
    monkeypatch.setenv("ZKP_FRI_FR_TAIL_LOG", tail_log)
    assert np.array_equal(zkp.fri_prove_fr(mem(coeffs), blowup, 3), default)
    assert [int(x) for x in default] == F.fri_flatten(F.fri_prove(coeffs, blowup, 3))


def test_reference_kats_through_the_library(zkp):
    """prover.rs:180-222 restated in Fr, on the library's output: fold([1,2,3,4], r=1) = [3,7]; layer 1 of the 4-point proof
    lives on the coset 7^2 = 49; the sym index of a query is index + D/2, with the evaluation and path of that index."""
    assert canon(zkp.fri_fold_fr(mem([1, 2, 3, 4]), F.limbs(1))) == [3, 7]
    coeffs = [1, 2, 3, 4]
    proof = [int(x) for x in zkp.fri_prove_fr(mem(coeffs), 1, 1)]
    D, L = proof[0], proof[1]
    assert D == 4 and L == 2
    roots = np.array(proof[7:7 + 4 * L], dtype=np.uint64).reshape(-1, 4)
    r, _ = zkp.fri_challenges_fr(roots, np.array(proof[7 + 4 * L:11 + 4 * L], dtype=np.uint64), 1)
    folded = canon(zkp.fri_fold_fr(mem(coeffs), r[0]))
    rec0 = 3 + 4 * (L + 2)
    idx = proof[rec0]
    rec1 = rec0 + 1 + 4 * (2 + 2 * L)  # layer-1 record of the same query
    w2 = M.root_of_unity(1, R)
    x = 49 * pow(w2, proof[rec1], R) % R
    assert F.from_mem([proof[rec1 + 1:rec1 + 5]])[0] == (folded[0] + folded[1] * x) % R
    evals = canon(zkp.fri_layer_eval_fr(mem(coeffs), F.limbs(7), 2))
    sym = (idx + 2) % 4
    assert F.from_mem([proof[rec0 + 5:rec0 + 9]])[0] == evals[sym]
    levels = F.merkle_levels(evals)
    assert F.from_mem(np.array(proof[rec0 + 9 + 8:rec0 + 9 + 16], dtype=np.uint64).reshape(-1, 4)) == F.merkle_path(levels, sym)
