"""The Fr transform's lazy reduction driven to its bound on the device: the adversarial vectors of tests/ntt_adversarial.py (built and
proved in contract by tests/model/ntt_fr_model.py, tests/test_ntt_fr_model_cpu.py) through every radix and every plan class, and
edge-valued data through every plan class of both fields.  Every output word against the CPU oracle, bit for bit.

The kernels never reduce inside a tile: a value grows by up to 4r per stage (csrc/fr29.hpp, csrc/ntt.hpp).  Random data stays 5 to 8r
under the ceiling that the design's margins are spent on; these vectors come within 2r of it."""
import os

import numpy as np
import pytest

import bigmodel as M
import ntt_adversarial as A

pytestmark = pytest.mark.gpu
DIRECTIONS = pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    yield zkp_hip
    zkp_hip.shutdown()


class knob:
    """The environment variable for the calls inside, and fresh plans on both sides when the knob is one that plans keep
    (as in tests/test_gpu_ntt_plan_edges.py)."""

    def __init__(self, zkp, name, value, fresh_plans=False):
        self.zkp, self.name, self.value, self.fresh = zkp, name, value, fresh_plans

    def __enter__(self):
        assert self.name not in os.environ
        if self.fresh:
            self.zkp.shutdown()
        os.environ[self.name] = self.value

    def __exit__(self, *exc):
        del os.environ[self.name]
        if self.fresh:
            self.zkp.shutdown()


def run_fr(zkp, a, log_n, batch=1, inverse=False, coset=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    zkp.ntt_fr_dev(t, log_n, batch, inverse=inverse, coset=coset)
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


# ------------------------------------------------------------------------------------------------------------- a single pass
@DIRECTIONS
@pytest.mark.parametrize("log_n", range(1, 12))
def test_single_pass_every_radix(zkp, orc, log_n, inverse):
    """2^1 .. 2^3: no round, one round, one round and a trailing stage; the inverse multiplies the grown values by 1/n (SCALE_CONST)"""
    a = A.to_array(A.single(log_n, inverse)[0])
    assert np.array_equal(run_fr(zkp, a, log_n, inverse=inverse), orc.ntt_fr(a, inverse=inverse))


@pytest.mark.parametrize("log_n", [8, 11])
def test_single_pass_behind_and_before_the_coset_table(zkp, orc, log_n):
    """forward: the tile's inputs are the pre-scale's tight products; inverse: the coset table times 1/n multiplies the grown values"""
    a = A.to_array(A.single_coset(log_n)[0])
    assert np.array_equal(run_fr(zkp, a, log_n, coset=A.COSET_ARRAY), orc.ntt_fr(a, coset=A.COSET_ARRAY))
    a = A.to_array(A.single(log_n, True)[0])
    assert np.array_equal(run_fr(zkp, a, log_n, inverse=True, coset=A.COSET_ARRAY), orc.ntt_fr(a, inverse=True, coset=A.COSET_ARRAY))


# ------------------------------------------------------------------------------------------------------------- pass 0 of every multi-pass class
@DIRECTIONS
@pytest.mark.parametrize("name", list(A.PLANTED))
def test_pass0_of_every_plan_class(zkp, orc, name, inverse):
    """Adversarial columns at the first, second, last column of a tile, the last column of the pass and some between, random words
    elsewhere: radix 2^6 with the twiddle matrix and with powtab_get's product, 2^8, 2^6 ahead of a middle pass, 2^9 (two-column
    tiles, a batch that crosses the wide threshold), 2^10 (single-column tiles) ahead of 2^9 and of 2^10."""
    c = A.PLANTED[name]
    a, _ = A.planted(name, inverse)
    n = 1 << c["log_n"]
    if c["matrix"]:
        got = run_fr(zkp, a, c["log_n"], c["batch"], inverse=inverse)
    else:
        with knob(zkp, "ZKP_NTT_TW_MATRIX_MAX_LOG", "0"):
            got = run_fr(zkp, a, c["log_n"], c["batch"], inverse=inverse)
    for b in range(c["batch"]):
        assert np.array_equal(got[b * n:(b + 1) * n], orc.ntt_fr(a[b * n:(b + 1) * n], inverse=inverse))


# ------------------------------------------------------------------------------------------------------------- a last-pass tile
@pytest.mark.parametrize("log_n", [12, 16])
def test_last_pass_tile(zkp, orc, log_n):
    """a pre-image through pass 0 aimed at one last-pass tile (radix 2^6 and 2^8): its inputs are what store_tight wrote"""
    a = A.last_pass(log_n)[0]
    assert np.array_equal(run_fr(zkp, a, log_n), orc.ntt_fr(a))


# ------------------------------------------------------------------------------------------------------------- edge values, both fields
def fr_edge(pattern, n):
    i = np.arange(n)
    return A.to_array([0, 1, M.R - 1])[{"r-1": i * 0 + 2, "zero": i * 0, "mix": (i * 7 + (i >> 5)) % 3}[pattern]]


@pytest.mark.parametrize("pattern", ["r-1", "zero", "mix"])
@pytest.mark.parametrize("log_n", [11, 12, 17, 19])
def test_fr_edge_values_through_every_plan_class(zkp, orc, log_n, pattern):
    """one pass, two, three, and two wide ones"""
    a = fr_edge(pattern, 1 << log_n)
    fwd = run_fr(zkp, a, log_n)
    assert np.array_equal(fwd, orc.ntt_fr(a))
    assert np.array_equal(run_fr(zkp, fwd, log_n, inverse=True), a)


def gl_edge(pattern, n):
    p, i = M.GL, np.arange(n)
    vals = np.array([0, 1, (1 << 32) - 1, 1 << 32, p - (1 << 32), p - 1], dtype=np.uint64)
    return vals[i * 0 + 5 if pattern == "p-1" else (i * 5 + (i >> 4)) % 6]


@pytest.mark.parametrize("pattern", ["p-1", "mix"])
@pytest.mark.parametrize("log_n", [13, 14, 19])
def test_goldilocks_edge_values_through_every_plan_class(zkp, orc, log_n, pattern):
    """one pass, two and three; the words around 2^32 and p - 2^32 are where the special-form reduction wraps"""
    a = gl_edge(pattern, 1 << log_n)
    fwd = zkp.ntt_goldilocks(a)
    assert np.array_equal(fwd, orc.ntt_gl(a))
    assert np.array_equal(zkp.ntt_goldilocks(fwd, inverse=True), a)
