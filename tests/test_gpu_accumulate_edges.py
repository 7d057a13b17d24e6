"""Edges of one insertion of msm_accumulate_kernel (csrc/msm.hpp: msm_accumulate_run; csrc/g1_28.hpp: g1_28_madd, g1_28_mmadd), at the
smallest shape that reaches the lane kernel and not the quad one: 2^17 + 5 points expanded at 16 bits -- 16 planes, more than 2^20
entries.  The bases are P_i = k_i G with known k_i, so every MSM has the known answer (sum s_i k_i) G (zkp_hip/trapdoor.py); each
case is also run with the scalars beyond the first 4 096 terms zeroed, at the same shape, against the oracle's Pippenger over that prefix.

What the k_i and the scalars are arranged to reach:
  plane boundaries   scalars at indices 0, 1, n - 2, n - 1 only: a wrong plane or point of locate() changes the sum
  extreme digits     all scalars r - 1, all 1, and scalars whose slices are the most negative digit (0x8000 with and without a carry in)
  exceptional adds   64 copies of one point under one scalar (a doubling at the second insertion); Q, R, Q + R, -2(Q + R) and two more
                     points under one scalar (a doubling inside the loop, infinity mid-run, insertions into it); P, -P, and two more;
                     runs of length 0, 1, 2 and 3 (the peeled iterations)
  oversized buckets  one scalar shared by n / 2 terms: the pieces path and msm_combine
  host-fed ranges    a batch of three resident vectors and a host-scalar call, two ranges each: resume / more and the hand-over array
Run on an MI355X with `pytest -m gpu`."""
import numpy as np
import pytest

import bigmodel as M

pytestmark = pytest.mark.gpu

N = (1 << 17) + 5
PREFIX = 4096
REP = range(1000, 1064)          # one point 64 times
NEG = 2000                       # P, -P, then two ordinary points
SUM = 3000                       # Q, R, Q + R, -2 (Q + R), then two ordinary points


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


class Setup:
    pass


@pytest.fixture(scope="module")
def env(orc):
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    from zkp_hip import trapdoor
    zkp_hip.init()
    s = Setup()
    s.zkp, s.trapdoor = zkp_hip, trapdoor
    ks = orc.rand_fr(0xACC0ED6E, N)
    k = orc.fr_to_ints(ks[[REP[0], NEG, SUM, SUM + 1]])
    special = {i: k[0] for i in REP}
    special.update({NEG + 1: M.R - k[1], SUM + 2: k[2] + k[3], SUM + 3: M.R - 2 * (k[2] + k[3])})
    idx = sorted(special)
    ks[idx] = orc.fr_from_ints([special[i] for i in idx])
    s.ks = ks
    s.d_ks = dev(ks)
    t_pts = torch.zeros(N * 12, dtype=torch.int64, device="cuda")
    zkp_hip.g1_fixed_base_mul_dev(s.d_ks, N, t_pts)
    s.pts_prefix = t_pts[: PREFIX * 12].cpu().numpy().view(np.uint64).reshape(PREFIX, 12)
    s.bases = zkp_hip.G1Bases.from_device(t_pts, N)
    s.bases.precompute(16)
    e = s.bases.expansion()
    assert e["planes"] == 16 and e["planes"] * N > 1 << 20, e   # the shape this file is about
    s.rnd = orc.rand_fr(0xACC05EED, N)
    return s


def expected(s, sc):
    return s.trapdoor.expected_msm(s.zkp, s.trapdoor.fr_inner_product(dev(sc), s.d_ks))


def check(s, orc, sc, what):
    """the resident-scalar MSM against the trapdoor value, and its 4 096-term prefix (same shape, zeros behind) against Pippenger"""
    exp, einf = expected(s, sc)
    out, inf = s.zkp.msm_g1_dev(s.bases, dev(sc), N)
    assert inf == einf and (inf or np.array_equal(out, exp)), what   # (the coordinates of infinity are not compared)
    head = np.zeros_like(sc)
    head[:PREFIX] = sc[:PREFIX]
    exp, einf = orc.msm_pippenger(s.pts_prefix, None, sc[:PREFIX])
    out, inf = s.zkp.msm_g1_dev(s.bases, dev(head), N)
    assert inf == einf and (inf or np.array_equal(out, exp)), what + " (prefix)"


def sparse(orc, values):
    """{index: scalar as int} -> (N, 4) Montgomery scalars, zero elsewhere"""
    sc = np.zeros((N, 4), dtype=np.uint64)
    idx = sorted(values)
    sc[idx] = orc.fr_from_ints([values[i] for i in idx])
    return sc


def test_plane_boundaries(env, orc):
    v = orc.fr_to_ints(env.rnd[:4])
    check(env, orc, sparse(orc, {0: v[0], 1: v[1], N - 2: v[2], N - 1: v[3]}), "first and last two points of every plane")
    check(env, orc, sparse(orc, {0: M.R - 1, N - 1: M.R - 1}), "first and last point, every digit signed")


def all_slices(lowest, others, top):
    return lowest | sum(others << (16 * j) for j in range(1, 15)) | (top << 240)


@pytest.mark.parametrize("name", ["r_minus_1", "one", "most_negative"])
def test_extreme_digits(env, orc, name):
    if name == "most_negative":
        # slices of 0x8000: the most negative digit where a slice of 2^15 is recoded as -2^15 with a carry out -- then every later slice
        # is 0x7fff + carry -- and the pattern without carries for a recoding that keeps +2^15; the top slice stays below r >> 240 = 0x73ed
        a = all_slices(0x8000, 0x7FFF, 0x73EC)
        b = all_slices(0x8000, 0x8000, 0x7000)
        assert a < M.R and b < M.R
        sc = np.tile(orc.fr_from_ints([a, b]), (N // 2 + 1, 1))[:N]
    else:
        sc = np.tile(orc.fr_from_ints([M.R - 1 if name == "r_minus_1" else 1]), (N, 1))
    check(env, orc, np.ascontiguousarray(sc), name)


def test_exceptional_insertions(env, orc):
    v = orc.fr_to_ints(env.rnd[:8])
    rep = {i: v[0] for i in REP}
    check(env, orc, sparse(orc, rep), "one point 64 times: doubling at the second insertion")
    chain = {SUM + j: v[1] for j in range(6)}
    check(env, orc, sparse(orc, chain), "Q, R, Q + R, -2 (Q + R), two more: doubling in the loop, infinity, insertions into it")
    check(env, orc, sparse(orc, {SUM + j: v[1] for j in range(4)}), "a run that ends at infinity")
    pair = {NEG + j: v[2] for j in range(4)}
    check(env, orc, sparse(orc, pair), "P, -P, two more: infinity at the second insertion")
    check(env, orc, sparse(orc, {NEG: M.R - 1, NEG + 1: M.R - 1}), "P, -P alone, negative digits: the whole sum is infinity")
    both = dict(rep)
    both.update(chain)
    both.update(pair)
    check(env, orc, sparse(orc, both), "all three together")
    short = {10: v[3], 20: v[4], 21: v[4], 30: v[5], 31: v[5], 32: v[5]}
    check(env, orc, sparse(orc, short), "runs of length 0, 1, 2 and 3")
    dense = env.rnd.copy()   # the same specials inside full buckets
    idx = sorted(both)
    dense[idx] = orc.fr_from_ints([both[i] for i in idx])
    check(env, orc, dense, "exceptional points inside random runs")


def test_oversized_buckets(env, orc):
    sc = env.rnd.copy()
    sc[0::2] = orc.fr_from_ints([orc.fr_to_ints(env.rnd[:1])[0]])[0]   # n / 2 terms share every digit: the pieces path, msm_combine
    check(env, orc, sc, "one scalar shared by n / 2 terms")


def test_host_fed_and_batched_ranges(env, orc, monkeypatch):
    s = env
    vecs = [s.rnd, np.roll(s.rnd, 1, axis=0), np.ascontiguousarray(s.rnd[::-1])]
    want = [expected(s, sc) for sc in vecs]
    monkeypatch.setenv("ZKP_MSM_RANGE_LOG", "17")   # 2^17 + 5 terms: a range of 2^17 and one of 5
    got = s.zkp.msm_g1_batch_dev(s.bases, [dev(sc) for sc in vecs], N)
    for (out, inf), (exp, einf) in zip(got, want):
        assert inf == einf and np.array_equal(out, exp)
    monkeypatch.delenv("ZKP_MSM_RANGE_LOG")
    monkeypatch.setenv("ZKP_MSM_FEED_RANGES", "2")
    out, inf = s.zkp.msm_g1(s.bases, vecs[0])
    assert inf == want[0][1] and np.array_equal(out, want[0][0])
