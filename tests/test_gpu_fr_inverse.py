"""GPU: the two device inversions of Fr lane by lane (zkp_selftest_fr_inverse_dev): the division steps of csrc/fr_inv.hpp and the
Fermat power of csrc/plonk.hpp on the inputs the Python model of tests/test_fr_safegcd_model.py walks -- 0, 1, r - 1, the
non-canonical r, r + 5, 2r - 1, powers of two +- 1, r >> k, Fibonacci-ratio values (the longest division-step chains) -- and a few
hundred random ones.  Every output word is the model's."""
import random

import numpy as np
import pytest

import fr_safegcd_model as G

pytestmark = pytest.mark.gpu
R = G.R


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def invert(zkp, xs, method):
    import torch
    n = len(xs)
    words = np.array([[(x >> (32 * w)) & 0xffffffff for w in range(8)] for x in xs], dtype=np.uint32)
    d_in = torch.from_numpy(words.view(np.int32).reshape(-1)).cuda()
    d_out = torch.full_like(d_in, 0x5a5a5a5a)
    zkp.selftest_fr_inverse_dev(d_in, n, method, d_out)
    torch.cuda.synchronize()
    out = d_out.cpu().numpy().view(np.uint32).reshape(n, 8)
    return [sum(int(out[i, w]) << (32 * w) for w in range(8)) for i in range(n)]


_expected = {}


def expected(xs):
    """the model's words for each input (the memory form: a R in, the canonical a^-1 R out), computed once"""
    for x in xs:
        if x not in _expected:
            _expected[x] = G.inverse_words(x)
    return [_expected[x] for x in xs]


def inputs():
    rnd = random.Random(0xF5AFE)
    return G.edge_inputs() + [rnd.randrange(1, R) for _ in range(300)] + [rnd.randrange(R, 2 * R) for _ in range(60)]


def test_division_steps_give_the_models_words(zkp):
    xs = inputs()
    got = invert(zkp, xs, 0)
    exp = expected(xs)
    for i, x in enumerate(xs):
        assert got[i] == exp[i], (i, hex(x))
        assert got[i] < R and (got[i] * x - pow(2, 512, R)) % R == 0 if x % R else got[i] == 0   # a R * a^-1 R = R^2; 0 and r -> 0


def test_fermat_power_gives_the_same_words(zkp):
    """fr_inverse takes canonical residues (and maps 0 to 0): the inputs below r, word for word the model's and the division steps'"""
    xs = [x for x in inputs() if x < R]
    got = invert(zkp, xs, 1)
    assert got == expected(xs)
    assert got == invert(zkp, xs, 0)


def test_lanes_of_one_wave_finish_at_different_rounds(zkp):
    """The early exit is wave-uniform: a wave leaves when its slowest lane has finished, and the lanes that finished before it keep
    running rounds that must change nothing.  Non-zero inputs need 17 to 19 rounds of the 25, zero (and r) one.  The first wave of 64
    lanes mixes all of these; then come a wave of zeros alone (it leaves after the first round), a wave of 17-round inputs alone and
    one of the slowest the model knows."""
    rounds = {x: G.modinv(x)[1] for x in G.edge_inputs()}
    by = {}
    for x in sorted(rounds):
        by.setdefault(rounds[x], []).append(x)
    assert by[1] == [0, R] and min(k for k in by if k > 1) < max(by) <= G.ROUNDS
    lo, hi = min(k for k in by if k > 1), max(by)
    fill = lambda pool, count: [pool[i % len(pool)] for i in range(count)]
    mixed = [v for quad in zip(fill(by[1], 16), fill(by[lo], 16), fill(by[hi], 16), fill(by[hi - 1], 16)) for v in quad]
    xs = mixed + fill(by[1], 64) + fill(by[lo], 64) + fill(by[hi], 64)
    assert len(mixed) == 64 and len(xs) == 256
    assert invert(zkp, xs, 0) == expected(xs)


def test_refusals(zkp):
    import torch
    t = torch.zeros(16, dtype=torch.int32, device="cuda")
    o = torch.full((16,), 7, dtype=torch.int32, device="cuda")
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.selftest_fr_inverse_dev(t, 2, 2, o)
    assert ei.value.code == zkp.ZKP_E_ARG and "method" in str(ei.value)
    zkp.selftest_fr_inverse_dev(t, 0, 0, o)
    torch.cuda.synchronize()
    assert (o.cpu() == 7).all()
