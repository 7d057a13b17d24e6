"""The MSM's bucket reduction stage by stage (csrc/msm.hpp: msm_combine, msm_fold_parts, msm_fold_parts_lane, msm_pyramid,
msm_pyramid_quad, msm_pyramid_tail, msm_collect; launched by MsmPass::launch_combine / launch_fold / reduce of csrc/msm_host.inc).
zkp_selftest_msm_reduce_dev runs them on bucket contents of the test's: every bucket is a pool entry k G of known discrete log
(tests/model/msm_reduce_model.py), so each of the c results of each bucket set, each folded and each combined bucket has ONE expected
point, and a failure names the window and the result ("sum", or "U_j: odd half of level j") or the bucket.  Every device point is also
held to the stored-point invariant; the hook fills what the reduction may read without having written it with 0xFF bytes, which is no
stored point.  Every case asserts from the geometry the hook reports that it is on the path it is named for
(tests/test_msm_reduce_model_cpu.py shows that the checker rejects single corruptions).  Run on an MI355X with `pytest -m gpu`."""
import time

import numpy as np
import pytest

import msm_reduce_model as RM

pytestmark = pytest.mark.gpu

KNOBS = ("ZKP_PYR_TAIL_THREADS", "ZKP_PYR_TAIL_BLOCKS", "ZKP_PYR_TAIL_HALF", "ZKP_FOLD_LANE_MIN")


class Setup:
    pass


@pytest.fixture(scope="module")
def env(orc):
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    s = Setup()
    s.zkp, s.orc, s.torch = zkp_hip, orc, torch
    s.pool = RM.Pool(orc)
    return s


@pytest.fixture(autouse=True)
def default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def dev(s, a):
    return s.torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint32)


# ---- bucket sets: index maps over the pool, in logical order (i = bucket - 1) ------------------------------------------------
def set_random(pool, nb, seed):
    return np.random.RandomState(seed).randint(0, len(pool), nb)


def set_same_point(pool, nb, j=1):
    """one point under varying z and representatives: every add at every level and in every O_j is a doubling"""
    return np.array([pool.idx(j, (RM.ONE, RM.Z, RM.WORST, RM.Z2)[(i * 7 // 3) % 4]) for i in range(nb)])


def set_alternating(pool, nb, j=2):
    """P, -P, P, -P: level 0 cancels everywhere, infinity meets infinity above; O_0 is all -P: doublings"""
    return np.array([pool.idx(j, RM.NEG if i & 1 else RM.Z) for i in range(nb)])


def set_infinity(pool, nb):
    return np.full(nb, pool.INF)


def set_one_live(pool, nb, at, j=3):
    m = np.full(nb, pool.INF)
    m[at] = pool.idx(j, RM.WORST)
    return m


def set_pqqp(pool, nb, j=4):
    """blocks (P, Q, Q, P): the equal sums P + Q and Q + P meet at level 1"""
    blk = [pool.idx(j, RM.Z), pool.idx(j + 1, RM.ONE), pool.idx(j + 1, RM.Z2), pool.idx(j, RM.WORST)]
    return np.array([blk[i & 3] for i in range(nb)])


def all_sets(pool, nb, seed=11):
    return [set_random(pool, nb, seed), set_same_point(pool, nb), set_alternating(pool, nb), set_infinity(pool, nb),
            set_one_live(pool, nb, 0), set_one_live(pool, nb, nb - 1), set_one_live(pool, nb, nb // 2 + nb // 8 + 1), set_pqqp(pool, nb),
            set_random(pool, nb, seed + 1)]


_want_cache = {}


def expected_results(s, bucket_logs, key=None):
    """(W, nb) discrete logs -> W rows of c expected points; cases that differ only in the launch shape share them (key)"""
    if key is None or key not in _want_cache:
        logs = RM.result_logs(bucket_logs)
        c = len(logs[0])
        flat = RM.points_of_logs(s.orc, [k for row in logs for k in row])
        _want_cache[key] = [flat[w * c:(w + 1) * c] for w in range(len(logs))]
    return _want_cache[key]


def reduce_sets(s, c, maps, key=None, want_geometry=None):
    """run the hook over the bucket sets `maps` (W, nb) and check the W x c results; -> (geometry, results)"""
    maps = np.asarray(maps)
    W, nb = maps.shape
    assert nb == 1 << (c - 1)
    g, res, flags = s.zkp.selftest_msm_reduce_dev(c, W, buckets=dev(s, RM.pack_planes(s.pool.gather(maps))))
    if want_geometry:
        want_geometry(g)
    assert (g["c"], g["nwin"], g["nb"], g["cap"], g["result_words"]) == (c, W, nb, W * nb, 64 * W * c)
    check_flags(g, flags)
    RM.check_results(res, expected_results(s, s.pool.logs(maps), key))
    return g, res


def check_flags(g, flags):
    """a set's flag word is its barrier counter as the last-levels launch left it: every workgroup arrived once per level -- which also
    says that the hook zeroed the counters -- and nobody gave up (top bit), nothing is pending (bit 30); msm_collect writes 0"""
    arrivals = g["tail_blocks"] * (g["c"] - 1 - g["nlevel"])
    assert flags.tolist() == [arrivals] * g["nwin"], (flags, arrivals, g)


def triples(sets):
    return [sets[k:k + 3] for k in range(0, len(sets), 3)]


# ---- the pyramid: c = 8, three bucket sets per call, every launch shape -----------------------------------------------------
def tail_only(threads, min_quads=1, blocks=None):
    """every level inside the last-levels launch, of `threads` threads per workgroup and at least min_quads quads per bucket set"""
    def want(g):
        assert g["nlevel"] == 0 and g["tail_threads"] == threads and g["tail_blocks"] * threads // 4 >= min_quads, g
        assert blocks is None or g["tail_blocks"] == blocks, g
    return want


def own_quad_levels_then_tail(g):
    assert [(v["level"], v["quad"]) for v in g["level"]] == [(l, 1) for l in range(6)] and g["tail_blocks"] >= 1, g


SHAPES = {   # a level of c = 8 has 64 items at most
    "default": ({}, tail_only(256)),
    "tail_half_1": ({"ZKP_PYR_TAIL_HALF": "1"}, own_quad_levels_then_tail),   # levels 0..5 as their own quad launches, the tail does the last
    "one_wave": ({"ZKP_PYR_TAIL_THREADS": "64", "ZKP_PYR_TAIL_BLOCKS": "1"}, tail_only(64, blocks=1)),   # 16 quads walk every item: the stride loop
    "idle_workgroups": ({"ZKP_PYR_TAIL_THREADS": "64", "ZKP_PYR_TAIL_BLOCKS": "256"}, tail_only(64, min_quads=65)),  # they must still arrive
    "eight_waves": ({"ZKP_PYR_TAIL_THREADS": "512", "ZKP_PYR_TAIL_BLOCKS": "8"}, tail_only(512, min_quads=65)),
}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_c8_three_sets(env, monkeypatch, shape):
    knobs, want = SHAPES[shape]
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    for t, maps in enumerate(triples(all_sets(env.pool, 128))):
        reduce_sets(env, 8, maps, key=("c8", t), want_geometry=want)


def test_c9_the_other_buffer_parity(env):
    """c - 1 even: the final and the previous pyramid buffer swap in pyr_result; level 0 is its own launch"""
    def want(g):
        assert g["nlevel"] == 1 and g["level"][0]["quad"] == 1 and g["tail_blocks"] >= 1, g
    for maps in triples(all_sets(env.pool, 256)):
        reduce_sets(env, 9, maps, want_geometry=want)


def test_c16_production_depth(env):
    """32768 buckets per set: quad levels down to the last-levels launch"""
    def want(g):
        assert g["nlevel"] == 8 and all(v["quad"] for v in g["level"]) and g["tail_blocks"] >= 1, g
    pool, nb = env.pool, 1 << 15
    sets = [set_random(pool, nb, 5), set_same_point(pool, nb), set_alternating(pool, nb), set_pqqp(pool, nb),
            set_one_live(pool, nb, nb // 2 + 12345), set_one_live(pool, nb, nb - 1)]
    for k in range(0, len(sets), 2):
        reduce_sets(env, 16, sets[k:k + 2], want_geometry=want)


def test_lane_levels_and_collect(env):
    """so many bucket sets that one workgroup per set would not be resident: every level its own launch, the widest ones one lane per
    add with all three kinds of item (kind 0; kind == level, reading pyr_out; kind < level, reading odd_in), then msm_collect_kernel"""
    s = env
    g0, _, _ = s.zkp.selftest_msm_reduce_dev(8, 3, run=False)
    nwin = max(1366, g0["tail_max_waves"] // 4 + 1)   # 48 adds per set at level 2: above 2^16 adds per launch from 1366 sets on

    def want(g):
        assert g["tail_blocks"] == 0 and g["nlevel"] == 7, g
        assert [v["quad"] for v in g["level"][:3]] == [0, 0, 0] and any(v["quad"] for v in g["level"][3:]), g

    pool = s.pool
    special = all_sets(pool, 128)
    rnd = np.random.RandomState(99)
    maps = rnd.randint(0, len(pool), (nwin, 128))
    for k, m in enumerate(special):                  # the arranged sets at the front, in the middle and at the end
        maps[k] = maps[nwin // 2 + k] = maps[nwin - 1 - k] = m
    t0 = time.time()
    reduce_sets(s, 8, maps, want_geometry=want)
    print(f"lane shape: {nwin} bucket sets, {time.time() - t0:.2f} s")


# ---- fold ------------------------------------------------------------------------------------------------------------------------
def part_tuple(pool, kind, nparts, rnd, j):
    inf, p, neg = pool.INF, pool.idx(j, RM.Z), pool.idx(j, RM.NEG)
    return [[inf] * (nparts - 1) + [p], [p] + [inf] * (nparts - 1), [pool.idx(j, (RM.Z, RM.Z2, RM.WORST, RM.ONE)[k]) for k in range(nparts)],
            [neg if k & 1 else p for k in range(nparts)], [inf] * nparts, rnd.randint(0, len(pool), nparts).tolist()][kind]


@pytest.mark.parametrize("form", ["lane", "quad"])
@pytest.mark.parametrize("split_log", [1, 2])
def test_fold_parts(env, monkeypatch, split_log, form):
    s, c, W, nb = env, 8, 3, 128
    monkeypatch.setenv("ZKP_FOLD_LANE_MIN", "1" if form == "lane" else str(1 << 40))
    nparts = 1 << split_log
    rnd = np.random.RandomState(split_log)
    maps = np.array([[part_tuple(s.pool, (i + w) % 6, nparts, rnd, i + w) for i in range(nb)] for w in range(W)])   # (W, nb, parts)
    maps = maps.transpose(2, 0, 1)                                                                                # (parts, W, nb)
    arrays = [RM.pack_planes(s.pool.gather(m)) for m in maps]
    out = s.torch.full((16 * W * nb * 4,), -1, dtype=s.torch.int32, device="cuda")
    g, res, flags = s.zkp.selftest_msm_reduce_dev(c, W, split_log, dev(s, arrays[0]), dev(s, np.stack(arrays[1:])), out_buckets=out)
    assert [(v["lane"], v["pairs"]) for v in g["fold"]] == [(int(form == "lane"), 1 << (split_log - 1 - t)) for t in range(split_log)], g
    assert g["parts_words"] == (nparts - 1) * g["bucket_words"]
    check_flags(g, flags)
    logs = RM.fold_logs(s.pool.logs(maps))
    want = RM.points_of_logs(s.orc, logs.reshape(-1).tolist())
    RM.check_buckets(RM.unpack_planes(host(out), W, nb), [want[w * nb:(w + 1) * nb] for w in range(W)], kind="folded bucket")
    RM.check_results(res, expected_results(s, logs))


# ---- combine ---------------------------------------------------------------------------------------------------------------------
class CombineCase:
    """c = 8, two bucket sets.  Set 0 has 70 candidates -- more than the combine grid's 64 workgroups per set, so the first six take
    a second turn of the `r += gridDim.x` walk -- with 0, 1, 2, 63, 64, 65 and 129 pieces among them (64 / 65: the LDS tree with
    every lane holding one piece, and one lane two); bucket ids 1, nb and in between; set 1 has a candidate with no piece next to
    one with 129."""
    c, W, nb, over_cap = 8, 2, 128, 72

    def __init__(self, s):
        pool = s.pool
        rnd = np.random.RandomState(42)
        counts0 = [129, 0, 65, 1, 64, 2, 63, 0] + [int(x) for x in rnd.randint(0, 5, 62)]
        ids0 = [1, 50, self.nb, 64, 65] + [int(x) for x in rnd.permutation(np.arange(2, 128))[:70] if x not in (50, 64, 65)][:65]
        self.cand = [list(zip(ids0, counts0)), [(77, 0), (78, 129), (1, 3)]]
        assert len(self.cand[0]) == 70 and len(set(ids0)) == 70
        self.pieces = []            # per set: the pool entries of its pieces, candidate after candidate
        for w, cand in enumerate(self.cand):
            row = []
            for r, (b, n) in enumerate(cand):
                if n == 64:         # all equal: the tree is six rounds of doublings
                    row += [pool.idx(20, (RM.Z, RM.Z2)[k & 1]) for k in range(n)]
                elif n == 65:       # pairs of opposites and one point left
                    row += [pool.idx(21, RM.NEG if k & 1 else RM.Z) for k in range(n)]
                else:
                    row += rnd.randint(0, len(pool), n).tolist()
            self.pieces.append(row)
        self.desc_cap = max(len(p) for p in self.pieces) + 3
        self.base = np.stack([set_random(pool, self.nb, 70), set_random(pool, self.nb, 71)])
        self.carry = rnd.randint(0, len(pool), (self.W, self.nb))
        over = np.zeros((self.W, 2), dtype=np.uint32)
        over_b = np.full((self.W, self.over_cap), 0xFFFFFFFF, dtype=np.uint32)
        over_off = np.full((self.W, self.over_cap + 1), 0xFFFFFFFF, dtype=np.uint32)
        pieces = np.full((self.W, self.desc_cap, 64), 0xFFFFFFFF, dtype=np.uint32)
        for w, cand in enumerate(self.cand):
            over[w] = (len(cand), len(self.pieces[w]))
            over_b[w, :len(cand)] = [b for b, _ in cand]
            over_off[w, :len(cand) + 1] = np.concatenate([[0], np.cumsum([n for _, n in cand])])
            pieces[w, :len(self.pieces[w])] = pool.gather(self.pieces[w])
        self.tables = dict(over=over, over_b=over_b, over_off=over_off, pieces=pieces)

    def combined(self, pool, resume):
        """{(w, i): expected log} of the buckets the combine writes"""
        out = {}
        for w, cand in enumerate(self.cand):
            p = 0
            for b, n in cand:
                if n:
                    out[(w, b - 1)] = RM.combine_log([pool.k[m] for m in self.pieces[w][p:p + n]], pool.k[self.carry[w, b - 1]] if resume else 0)
                p += n
        return out


@pytest.fixture(scope="module")
def combine_case(env):
    return CombineCase(env)


@pytest.mark.parametrize("mode", ["plain", "resume", "more", "resume_more"])
def test_combine(env, combine_case, mode):
    s, cc, pool, torch = env, combine_case, env.pool, env.torch
    W, nb = cc.W, cc.nb
    resume, more = "resume" in mode, "more" in mode
    base_words = pool.gather(cc.base)
    carry_words = RM.to_physical(pool.gather(cc.carry))
    comb = dict(over_cap=cc.over_cap, desc_cap=cc.desc_cap, more=more, **{k: dev(s, v) for k, v in cc.tables.items()})
    if resume:
        comb["carry"] = dev(s, carry_words)
    if more:
        comb["out_carry"] = torch.full((W * nb * 64,), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
    out = torch.full((W * nb * 64,), -1, dtype=torch.int32, device="cuda")
    g, res, flags = s.zkp.selftest_msm_reduce_dev(cc.c, W, buckets=dev(s, RM.pack_planes(base_words)), combine=comb, out_buckets=out)
    assert g["combine_x"] == 64 and g["over_cap"] >= 70 and len(cc.cand[0]) > g["combine_x"], g
    got = RM.unpack_planes(host(out), W, nb)
    comb_logs = cc.combined(pool, resume)
    keys = sorted(comb_logs)
    comb_pts = dict(zip(keys, RM.points_of_logs(s.orc, [comb_logs[k] for k in keys])))
    want = [[comb_pts.get((w, i)) for i in range(nb)] for w in range(W)]
    written = np.zeros((W, nb), dtype=bool)
    for w, i in keys:
        written[w, i] = True
    assert written[0, 0] and written[0, nb - 1] and not written[0, 50 - 1]    # buckets 1 and nb combined, bucket 50 a candidate with no piece
    if more:   # the sums went to the hand-over array; the buckets, the results and the flags are as they were
        assert np.array_equal(got, base_words), "the combine wrote a bucket although another range follows"
        assert (res == 0xFFFFFFFF).all() and (flags == 0xFFFFFFFF).all()
        carry = RM.from_physical(host(comb["out_carry"]), W, nb)
        RM.check_buckets(carry, want, kind="hand-over entry of bucket", only=keys)
        rest = pool.gather(cc.carry) if resume else np.full((W, nb, 64), 0xFFFFFFFF, dtype=np.uint32)   # (the hook's fill)
        assert np.array_equal(carry[~written], rest[~written]), "a hand-over entry of a bucket that was not combined changed"
        return
    check_flags(g, flags)
    RM.check_buckets(got, want, kind="combined bucket", only=keys)
    assert np.array_equal(got[~written], base_words[~written]), "a bucket without pieces did not come back untouched"
    logs = pool.logs(cc.base)
    for (w, i), k in comb_logs.items():
        logs[w, i] = k
    RM.check_results(res, expected_results(s, logs))


# ---- housekeeping ----------------------------------------------------------------------------------------------------------------
def test_twice_the_same_words_and_geometry_without_a_launch(env):
    s = env
    maps = np.stack(all_sets(s.pool, 128, seed=31)[:3])
    g1, r1 = reduce_sets(s, 8, maps)
    g2, r2 = reduce_sets(s, 8, maps)
    g0, none_r, none_f = s.zkp.selftest_msm_reduce_dev(8, 3, run=False)
    assert g1 == g2 == g0 and none_r is None and none_f is None
    assert np.array_equal(r1, r2)


def test_an_msm_right_after_the_hook_is_exact(env):
    s, n = env, 4096
    orc, zkp, torch = s.orc, s.zkp, s.torch
    ks, sc = orc.rand_fr(0xBA5E, n), orc.rand_fr(0x5EED, n)
    t_pts = torch.zeros(n * 12, dtype=torch.int64, device="cuda")
    zkp.g1_fixed_base_mul_dev(torch.from_numpy(ks.view(np.int64)).cuda(), n, t_pts)
    bases = zkp.G1Bases.from_device(t_pts, n)
    exp, einf = orc.g1_mul(orc.g1_generator(), 0, orc.fr_inner_product(sc, ks))
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    reduce_sets(s, 16, [set_random(s.pool, 1 << 15, 3)])    # the MSM below has c = 16 too: the same workspaces, 0xFF-filled by the hook
    out, inf = zkp.msm_g1_dev(bases, d_sc, n)
    assert inf == einf and np.array_equal(out, exp)
    reduce_sets(s, 8, np.stack(all_sets(s.pool, 128)[:3]), key=("c8", 0))
    out, inf = zkp.msm_g1_dev(bases, d_sc, n)
    assert inf == einf and np.array_equal(out, exp)


def test_refusals(env, monkeypatch):
    s = env
    zkp, torch = s.zkp, s.torch
    good = dev(s, RM.pack_planes(s.pool.gather(np.stack(all_sets(s.pool, 128)[:3]))))

    def refused(match, *a, **kw):
        with pytest.raises(zkp.ZkpError, match=match) as e:
            zkp.selftest_msm_reduce_dev(*a, **kw)
        assert e.value.code == zkp.ZKP_E_ARG

    refused("window width", 1, 3, buckets=good)
    refused("window width", 25, 3, buckets=good)
    refused("bucket sets", 8, 0, buckets=good)
    refused("split_log", 8, 3, 3, buckets=good)
    refused("null or too-small", 8, 3)                                    # no buckets
    refused("null or too-small", 8, 3, buckets=good[:-4])
    refused("null or too-small", 8, 3, 1, buckets=good)                   # split_log 1 without parts
    refused("null or too-small", 8, 3, buckets=good, out_buckets=torch.zeros(64, dtype=torch.int32, device="cuda"))
    z = torch.zeros(4096, dtype=torch.int32, device="cuda")
    block = dict(over=z, over_b=z, over_off=z, pieces=z)
    refused("combine block", 8, 3, buckets=good, combine=dict(over_cap=0, desc_cap=4, **block))
    refused("combine block", 8, 3, buckets=good, combine=dict(over_cap=4, desc_cap=4, **dict(block, pieces=z[:16])))
    refused("combine block", 8, 3, buckets=good, combine=dict(over_cap=4, desc_cap=4, more=True, **block))       # more without out_carry
    bad = z.clone()
    bad[0] = 5                                                            # five candidates, over_cap four
    refused("candidates", 8, 3, buckets=good, combine=dict(over_cap=4, desc_cap=4, **dict(block, over=bad)))
    bad[0] = 1                                                            # one candidate, bucket id 0
    refused("bucket id", 8, 3, buckets=good, combine=dict(over_cap=4, desc_cap=4, **dict(block, over=bad)))
    for knob, v in (("ZKP_PYR_TAIL_THREADS", "100"), ("ZKP_PYR_TAIL_BLOCKS", "0"), ("ZKP_PYR_TAIL_HALF", "0")):
        monkeypatch.setenv(knob, v)
        refused("ZKP_PYR_TAIL_THREADS must be", 8, 3, buckets=good)
        refused("ZKP_PYR_TAIL_THREADS must be", 8, 3, run=False)
        monkeypatch.delenv(knob)
    reduce_sets(s, 8, np.stack(all_sets(s.pool, 128)[:3]), key=("c8", 0))  # and the slot still works
