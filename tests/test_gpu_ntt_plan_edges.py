"""The smallest transform of every plan class (csrc/ntt_plan.hpp: pass count, radices, direct tables, the pass-0 matrix, where 1/n
rides), every output word against the CPU oracle: forward, then the inverse back to the input.

A plan is cached per (size, direction, allow_wide) until zkp_shutdown, and ZKP_NTT_NO_WIDE_PASS acts on plans built from then on: the
cases that set it shut the library down around the variant, so that each variant builds its own plan and no plan built under a knob
outlives this module."""
import os

import numpy as np
import pytest

import bigmodel as M

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    yield zkp_hip
    zkp_hip.shutdown()


class knob:
    """The environment variable for the calls inside, and fresh plans on both sides when the knob is one that plans keep."""

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


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def host(t, cols=None):
    a = t.cpu().numpy().view(np.uint64)
    return a.reshape(-1, cols) if cols else a


def fr_pair(zkp, a, log_n, batch=1, coset=None):
    """(forward, inverse of the forward) of `batch` transforms on the device."""
    t = dev(a)
    zkp.ntt_fr_dev(t, log_n, batch, coset=coset)
    fwd = host(t, 4).copy()
    zkp.ntt_fr_dev(t, log_n, batch, inverse=True, coset=coset)
    return fwd, host(t, 4)


# 2^11 largest single pass, 2^12 first and 2^16 last two-pass, 2^17 first three-pass (direct middle table), 2^19 and 2^20 radix 2^10
# (single-column tiles), 2^21 three passes that wide passes cannot shorten
@pytest.mark.parametrize("log_n", [11, 12, 16, 17, 19, 20, 21])
def test_fr_plan_classes(zkp, orc, log_n):
    a = orc.rand_fr(0x9E0000 + log_n, 1 << log_n)
    fwd, back = fr_pair(zkp, a, log_n)
    assert np.array_equal(fwd, orc.ntt_fr(a))
    assert np.array_equal(back, a)


# from 2^19 elements per launch the radix-2^9 two-pass plan; without wide passes the same data gives the same words
@pytest.mark.parametrize("log_n,batch", [(17, 4), (18, 2)])
def test_fr_batches_across_the_wide_threshold(zkp, orc, log_n, batch):
    n = 1 << log_n
    a = orc.rand_fr(0x9E1000 + log_n, batch * n)
    fwd, back = fr_pair(zkp, a, log_n, batch)
    for b in range(batch):
        assert np.array_equal(fwd[b * n:(b + 1) * n], orc.ntt_fr(a[b * n:(b + 1) * n]))
    assert np.array_equal(back, a)
    with knob(zkp, "ZKP_NTT_NO_WIDE_PASS", "1", fresh_plans=True):
        narrow_fwd, narrow_back = fr_pair(zkp, a, log_n, batch)
    assert np.array_equal(narrow_fwd, fwd)
    assert np.array_equal(narrow_back, a)


@pytest.mark.parametrize("log_n", [12, 17])
def test_fr_coset(zkp, orc, log_n):
    """The inverse carries 1/n on the coset table."""
    a = orc.rand_fr(0x9E2000 + log_n, 1 << log_n)
    g = orc.rand_fr(97, 1)[0]
    fwd, back = fr_pair(zkp, a, log_n, coset=g)
    assert np.array_equal(fwd, orc.ntt_fr(a, coset=g))
    assert np.array_equal(back, a)
    assert np.array_equal(zkp.ntt_fr(a, inverse=True, coset=g), orc.ntt_fr(a, inverse=True, coset=g))


def test_fr_inverse_scaling_on_pass0_by_table_and_by_matrix(zkp, orc):
    """The two routes by which 1/n rides on pass 0: the two-level table times 1/n, and the twiddle matrix made from it."""
    a = orc.rand_fr(0x9E3012, 1 << 12)
    with knob(zkp, "ZKP_NTT_TW_MATRIX_MAX_LOG", "0"):
        by_table = zkp.ntt_fr(a, inverse=True)
    by_matrix = zkp.ntt_fr(a, inverse=True)
    assert np.array_equal(by_table, orc.ntt_fr(a, inverse=True))
    assert np.array_equal(by_matrix, by_table)


# 2^13 largest single pass, 2^14 first and 2^18 last two-pass, 2^19 first three-pass
@pytest.mark.parametrize("log_n", [13, 14, 18, 19])
def test_goldilocks_plan_classes(zkp, orc, log_n):
    a = orc.rand_gl(0x9E4000 + log_n, 1 << log_n)
    fwd = zkp.ntt_goldilocks(a)
    assert np.array_equal(fwd, orc.ntt_gl(a))
    assert np.array_equal(zkp.ntt_goldilocks(fwd, inverse=True), a)


def test_fr_four_passes_with_a_middle_pass_on_the_two_level_table(zkp, orc):
    """2^25 without wide passes: the smallest transform in four passes, whose pass 1 (sub-problems of 2^18) has no direct table.
    Round trip, linearity, and three outputs against the definition X[k] = sum_j a_j w^(jk) (Horner on the oracle)."""
    import torch
    log_n = 25
    n = 1 << log_n
    a = orc.rand_fr(0x9E5019, n)
    b = np.roll(a, 1, axis=0)
    with knob(zkp, "ZKP_NTT_NO_WIDE_PASS", "1", fresh_plans=True):
        t = dev(a)
        zkp.ntt_fr_dev(t, log_n)
        fa = host(t, 4).copy()
        zkp.ntt_fr_dev(t, log_n, inverse=True)
        torch.cuda.synchronize()
        assert np.array_equal(host(t, 4), a)
        t.copy_(dev(b))
        zkp.ntt_fr_dev(t, log_n)
        fb = host(t, 4).copy()
        t.copy_(dev(orc.fr_add(a, b)))
        zkp.ntt_fr_dev(t, log_n)
        assert np.array_equal(host(t, 4), orc.fr_add(fa, fb))
        del t
        torch.cuda.empty_cache()
    w = orc.fr_root_of_unity(log_n)
    for k in (1, 12345, n - 1):
        wk = orc.fr_from_ints([pow(orc.fr_to_ints(w.reshape(1, 4))[0], k, M.R)])[0]
        assert np.array_equal(orc.poly_eval_fr(a, wk), fa[k])
