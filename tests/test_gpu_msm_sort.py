"""The MSM's digit recoding and counting sort, stage by stage (csrc/msm.hpp: msm_digits*, msm_parthist, msm_partprefix, msm_partstart,
msm_partscatter<TILE>, msm_binsort, msm_rank, msm_order; launched by MsmPass::launch_sort of csrc/msm_host.inc).  Every case runs the
production sort of one scalar range through zkp_selftest_msm_sort_dev, which hands back every stage's output and the geometry the kernels
were given; the case asserts that the geometry is the shape it is named for, compares the digits bit for bit with
msm_sort_model.reference_digits and hands the rest to msm_sort_model.check_sort_outputs (tests/test_msm_sort_model_cpu.py shows that
the checker rejects single corruptions).  The hook fills the outputs with 0xFF first, so a write outside a kernel's own slots shows.

The points are k_i G (irrelevant here: nothing is accumulated).  Every case carries the same mix of scalars: random ones, 0, 1, r - 1,
all-ones slices, slices of 2^(width - 1) and 2^(width - 1) + 1 with and without a carry coming in (msm_sort_model.edge_scalars, built
from the slice offsets the hook reports), and a few bases flagged infinity.  Run on an MI355X with `pytest -m gpu`."""
import random

import numpy as np
import pytest

import msm_sort_model as S

pytestmark = pytest.mark.gpu

NMAX = 40003
PS_TILE_BIG, PS_TILE_MID, PS_TILE_SMALL = 12288, 8192, 4096
INF_AT = (3, 64, 1023, 1024, 1499)  # bases flagged infinity (inside every handle and every range below)


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
    s.zkp, s.orc, s.torch, s.trapdoor = zkp_hip, orc, torch, trapdoor
    s.d_ks = torch.from_numpy(orc.rand_fr(0x50A7, NMAX).view(np.int64)).cuda()
    s.pts = torch.zeros(NMAX * 12, dtype=torch.int64, device="cuda")
    zkp_hip.g1_fixed_base_mul_dev(s.d_ks, NMAX, s.pts)
    s.handles = {}
    return s


class Bases:
    def __init__(self, handle, inf):
        self._h, self.handle, self.inf = handle._h, handle, inf  # (_h: what zkp_hip's entries read)


def bases(s, n, expand=None, glv=False, inf_at=INF_AT):
    """the first n points, those at inf_at flagged infinity; expand: window bits of the shared-bucket expansion"""
    key = (n, expand, glv, inf_at)
    if key not in s.handles:
        inf = np.zeros(n, dtype=np.uint8)
        inf[list(inf_at)] = 1
        h = s.zkp.G1Bases.from_device(s.pts[:12 * n], n, s.torch.from_numpy(inf).cuda())
        s.torch.cuda.synchronize()
        if expand:
            h.precompute(expand, glv=glv)
        s.handles[key] = Bases(h, inf)
    return s.handles[key]


def dev(s, ints):
    return s.torch.from_numpy(s.orc.fr_from_ints(ints).view(np.int64)).cuda()


def mixed_scalars(seed, n, geom):
    """random scalars with the edge scalars of this geometry at the front, in the middle and at the end"""
    rnd = random.Random(seed)
    sc = [rnd.randrange(S.R) for _ in range(n)]
    edge = S.edge_scalars(geom["off"], glv=bool(geom["glv"]))
    if n >= 3 * len(edge):
        sc[:len(edge)] = edge
        sc[n // 2:n // 2 + len(edge)] = edge
        sc[n - len(edge):] = edge
    return sc


def geometry(s, h, count, n, range_index=0):
    """the first call of the hook: null outputs, zero-filled scalars of the right size are enough to plan"""
    z = s.torch.zeros(4 * n, dtype=s.torch.int64, device="cuda")
    return s.zkp.selftest_msm_sort_dev(h, [z] * count, n, range_index)


def run_sort(s, h, vecs, n, range_index=0):
    """vecs: one list of n canonical integers per MSM.  -> (geometry, digits, outputs as uint32 arrays) of that range"""
    torch = s.torch
    tensors = [dev(s, v) for v in vecs]
    g = s.zkp.selftest_msm_sort_dev(h, tensors, n, range_index)
    out = {k: torch.empty(max(w, 1), dtype=torch.int32, device="cuda") for k, w in g["out_words"].items()}
    g2 = s.zkp.selftest_msm_sort_dev(h, tensors, n, range_index, out)
    torch.cuda.synchronize()
    assert g2 == g
    W = g["nwin"]
    shape = dict(digits=(W, g["n"]), entries=(W, g["n"], 2), desc=(W, g["desc_cap"], 4))
    host = {k: out[k].cpu().numpy().view(np.uint32)[:g["out_words"][k]].reshape(shape.get(k, (W, -1))) for k in out}
    return g, host.pop("digits"), host


_ref_cache = {}


def check(s, h, vecs, n, range_index=0, want=None, ref_key=None):
    """run the hook, assert the geometry `want`, compare the digits with the model and check every later stage against them.
    ref_key: cases that differ only in how the sort is cut up share one reference (the digits do not depend on it)"""
    g, digits, out = run_sort(s, h, vecs, n, range_index)
    for k, v in (want or {}).items():
        assert g[k] == v, f"geometry: {k} is {g[k]}, the case is about {v} ({g})"
    lo, ln = g["range_off"], g["range_len"]
    assert g["ns"] == ln and lo + ln <= n
    if ref_key is None or ref_key not in _ref_cache:
        _ref_cache[ref_key] = S.reference_digits(g, [v[lo:lo + ln] for v in vecs], h.inf[lo:lo + ln])
    ref = _ref_cache[ref_key]
    if not np.array_equal(digits, ref):
        w, i = (int(x[0]) for x in np.nonzero(digits != ref))
        raise AssertionError(f"window {w}, stage digits, index {i}: is {int(digits[w, i]):#x}, expected {int(ref[w, i]):#x}")
    S.check_sort_outputs(g, ref, out)
    return g, ref, out


def plan_only(s, h, count, n):
    return geometry(s, h, count, n)


# ------------------------------------------------------------------------------------------------------------------ cases
def test_one_partition_of_128_bins(env):
    """lo_n = 128 bins, fewer than the workgroup's threads, in one partition; nb = 128 is no multiple of msm_rank's 1024 buckets"""
    n = 2047
    h = bases(env, n)
    g = plan_only(env, h, 1, n)
    check(env, h, [mixed_scalars(1, n, g)], n, want=dict(c=8, nwin=32, nb=128, lo_bits=7, nhi=1, shared=0, nranges=1, n=n, ps_tile=PS_TILE_BIG))


def test_saturated_size_class_is_rechecked(env, monkeypatch):
    """run_limit = 512 > 255: every bucket of the saturated class is a candidate and msm_order re-checks its size.  Window 0 holds planted
    buckets of 255, run_limit, run_limit + 1 and 3 piece + 1 entries: all four are in the saturated class, three are candidates that must
    get no piece, one gets five"""
    monkeypatch.setenv("ZKP_MSM_C", "8")
    n = 1 << 14
    h = bases(env, n)
    g = plan_only(env, h, 1, n)
    rnd = random.Random(2)
    sc = S.plant_c8_buckets(g, [rnd.randrange(S.R) for _ in range(n)], S.edge_scalars(g["off"]), skip=INF_AT)
    g, ref, out = check(env, h, [sc], n, want=dict(c=8, nwin=32, nb=128, run_limit=512, piece=128, nhi=1, nchunk=4, nranges=1))
    assert list(np.bincount(ref[0] >> 1, minlength=129)[1:5]) == [255, 512, 513, 385]
    assert list(out["over"][0]) == [4, 5]  # buckets 1 to 4 are candidates, only bucket 3 has pieces: ceil(513 / 128)


@pytest.mark.parametrize("n", [4095, 4096, 4097])
def test_load_group_and_chunk_edges(env, monkeypatch, n):
    """one chunk of n digits: the four-loads-per-lane groups of msm_parthist and the tile loop of msm_partscatter end inside, at and
    one past a multiple of 4096"""
    monkeypatch.setenv("ZKP_MSM_NCHUNK", "1")
    h = bases(env, n)
    g = plan_only(env, h, 1, n)
    check(env, h, [mixed_scalars(3, n, g)], n, want=dict(c=16, nwin=16, nb=32768, lo_bits=8, nhi=128, nchunk=1, chunk=n, ps_tile=PS_TILE_BIG))


def test_three_partscatter_tiles(env, monkeypatch):
    """one chunk of 2 x 12288 + 1 digits: two full tiles of msm_partscatter and a third with one digit"""
    monkeypatch.setenv("ZKP_MSM_NCHUNK", "1")
    n = 2 * PS_TILE_BIG + 1
    h = bases(env, n)
    g = plan_only(env, h, 1, n)
    check(env, h, [mixed_scalars(4, n, g)], n, want=dict(c=16, nwin=16, nchunk=1, chunk=n, ps_tile=PS_TILE_BIG, nhi=128))


@pytest.mark.parametrize("nchunk,n", [(7, 40001), (17, 40001), (33, 40001), (17, 40003)])
def test_partprefix_chunk_groups(env, monkeypatch, nchunk, n):
    """msm_partprefix's 16 chunk groups own ceil(nchunk / 16) chunks each: fewer chunks than groups, one chunk more than 16, and three
    per group with groups left over.  40001 is no multiple of 7 or 33, so their last chunk is short; it is 17 x 2353, so 17 chunks are
    also run over 40003 digits, where the last one is short as well"""
    monkeypatch.setenv("ZKP_MSM_NCHUNK", str(nchunk))
    h = bases(env, n)
    g = plan_only(env, h, 1, n)
    assert (n % nchunk == 0) == ((nchunk, n) == (17, 40001))
    check(env, h, [mixed_scalars(5, n, g)], n, want=dict(c=16, nwin=16, nchunk=nchunk, chunk=-(-n // nchunk), nhi=128), ref_key=("partprefix", n))


def test_second_copy_out_tile_of_binsort(env):
    """window 0: partition 0 holds exactly one copy-out tile of msm_binsort (16 384 entries), partition 5 one entry more (a second tile
    of one entry), partitions 1 and 2 -- like every other -- are empty.  n = 2^15 + 3 leaves two terms over: they are this case's
    two bases flagged infinity (five flags would not leave 16 384 + 16 385 digits), and they carry the scalars 0 and r - 1.  The lowest 16
    bits of every other scalar are planted, the edge scalars' too: their patterns stay in windows 1 to 15."""
    n = (1 << 15) + 3
    flagged = (64, 1024)
    h = bases(env, n, inf_at=flagged)
    g = plan_only(env, h, 1, n)
    rnd = random.Random(6)
    sc = mixed_scalars(6, n, g)
    first = [i for i in range(n) if i not in flagged]
    assert len(first) == 16384 + 16385
    for j, i in enumerate(first):
        mag = (1 + rnd.randrange(256)) if j < 16384 else (5 * 256 + 1 + rnd.randrange(256))
        low = mag if rnd.randrange(2) else (1 << 16) - mag  # the digit +mag, or -mag with a carry into window 1
        sc[i] = (sc[i] & ~0xFFFF) | low
        if sc[i] >= S.R:  # (r - 1 with its lowest bits planted)
            sc[i] = (rnd.randrange(S.R >> 1) & ~0xFFFF) | low
    sc[flagged[0]], sc[flagged[1]] = 0, S.R - 1
    assert all(k < S.R for k in sc)
    g, ref, out = check(env, h, [sc], n, want=dict(c=16, nwin=16, lo_bits=8, nhi=128, n=n))
    assert list(out["pstart"][0][:7]) == [0, 16384, 16384, 16384, 16384, 16384, 16384 + 16385] and int(out["pstart"][0][128]) == 16384 + 16385


def test_every_thread_a_bin(env, monkeypatch):
    """lo_n = 1024 bins: every thread of msm_binsort owns one; nhi = 32 partitions, fewer than the 64 lanes msm_partprefix gives a row"""
    monkeypatch.setenv("ZKP_SORT_LO_BITS", "10")
    n = 3001
    h = bases(env, n)
    g = plan_only(env, h, 1, n)
    check(env, h, [mixed_scalars(7, n, g)], n, want=dict(c=16, nwin=16, lo_bits=10, nhi=32))


def test_lo_bits_9_and_uneven_slices(env):
    """bases expanded at 20 bits: 13 slices of 20 and 19 bits that straddle the 32-bit limbs, lo_bits = 9 by default, 1024 partitions"""
    n = 1500
    h = bases(env, n, expand=20)
    g = plan_only(env, h, 1, n)
    widths = {g["off"][k + 1] - g["off"][k] for k in range(g["nslice"])}
    assert widths == {19, 20} and any(a // 32 != (b - 1) // 32 for a, b in zip(g["off"], g["off"][1:]))
    check(env, h, [mixed_scalars(8, n, g)], n, want=dict(c=20, shared=1, nwin=1, nslice=13, nb=1 << 19, lo_bits=9, nhi=1024, n=13 * n, ps_tile=PS_TILE_BIG))


def test_partscatter_tile_mid(env, monkeypatch):
    """msm_partscatter<PS_TILE_MID>: 4096 partitions"""
    monkeypatch.setenv("ZKP_SORT_LO_BITS", "6")
    n = 1500
    h = bases(env, n, expand=19)
    g = plan_only(env, h, 1, n)
    check(env, h, [mixed_scalars(9, n, g)], n, want=dict(c=19, shared=1, nwin=1, nslice=14, lo_bits=6, nhi=4096, ps_tile=PS_TILE_MID))


def test_partscatter_tile_small(env, monkeypatch):
    """msm_partscatter<PS_TILE_SMALL>: 8192 partitions, the most the sort takes (SORT_MAX_PART)"""
    monkeypatch.setenv("ZKP_SORT_LO_BITS", "6")
    n = 1500
    h = bases(env, n, expand=20)
    g = plan_only(env, h, 1, n)
    check(env, h, [mixed_scalars(10, n, g)], n, want=dict(c=20, shared=1, nwin=1, nslice=13, lo_bits=6, nhi=8192, ps_tile=PS_TILE_SMALL))


def test_batch_layout_per_window(env):
    """digits [msm][slice][scalar]: three vectors, a different one per MSM, the middle one all zero"""
    n = 2100
    h = bases(env, n)
    g = plan_only(env, h, 3, n)
    vecs = [mixed_scalars(11, n, g), [0] * n, mixed_scalars(12, n, g)[::-1]]
    check(env, h, vecs, n, want=dict(c=16, shared=0, nwin=48, nslice=16, n=n))


def test_batch_layout_shared(env):
    """two vectors over expanded bases: one bucket set each; the second all zero"""
    n = 2100
    h = bases(env, 8192, expand=16)
    g = plan_only(env, h, 2, n)
    check(env, h, [mixed_scalars(13, n, g), [0] * n], n, want=dict(c=16, shared=1, glv=0, nwin=2, nslice=16, n=16 * n, nranges=1))


def test_endomorphism_split_groups(env):
    """endomorphism-split planes: MSM m fills digit groups 2m (k mod lambda) and 2m + 1 (k div lambda)"""
    n = 1500
    h = bases(env, n, expand=16, glv=True)
    g = plan_only(env, h, 2, n)
    assert g["off"][g["nslice"]] >= 129
    lam = [S.LAMBDA, S.LAMBDA - 1, S.LAMBDA + 1, (S.LAMBDA + 1) * S.LAMBDA - 1]
    a, b = mixed_scalars(14, n, g), mixed_scalars(15, n, g)
    a[100:100 + len(lam)] = lam
    check(env, h, [a, b], n, want=dict(shared=1, glv=1, nwin=4, n=g["nslice"] * n, nranges=1))


@pytest.mark.parametrize("range_index", [0, 1, 2])
def test_later_and_shorter_ranges(env, monkeypatch, range_index):
    """2500 scalars in ranges of at most 2^10: 834, 834 and 832 -- the scalars and infinity flags of a later range start at its offset,
    and the last range sorts with a narrower geometry inside workspaces sized for the longest"""
    monkeypatch.setenv("ZKP_MSM_RANGE_LOG", "10")
    n = 2500
    h = bases(env, 8192, expand=16)
    g = plan_only(env, h, 1, n)
    lens = [834, 834, 832]
    check(env, h, [mixed_scalars(16, n, g)], n, range_index,
          want=dict(shared=1, nwin=1, nranges=3, range_index=range_index, range_off=sum(lens[:range_index]), range_len=lens[range_index],
                    ns=lens[range_index], n=16 * lens[range_index]))


def test_oversized_bucket_and_pieces(env):
    """one scalar shared by n / 2 terms: every slice has a bucket of more than 2048 entries, cut into pieces of 32"""
    n = 4096
    h = bases(env, 8192, expand=16)
    g = plan_only(env, h, 1, n)
    sc = mixed_scalars(17, n, g)
    sc[0::2] = [0x1234567 * S.LAMBDA + 0x89ABCDEF] * (n // 2)
    g, ref, out = check(env, h, [sc], n, want=dict(c=16, shared=1, nwin=1, n=16 * n, run_limit=128, piece=32, nranges=1))
    assert int(out["over"][0][0]) >= 8 and int(out["over"][0][1]) >= 8 * (2040 // 32)


def test_production_default_shape_and_the_next_msm(env):
    """shared c = 16, 2^13 terms, no knob: the hook's outputs are valid, and the MSM that follows it on the same workspaces gives the
    trapdoor value (sum s_i k_i) G over the bases that are not flagged"""
    n = 1 << 13
    h = bases(env, 8192, expand=16)
    g = plan_only(env, h, 1, n)
    sc = mixed_scalars(18, n, g)
    check(env, h, [sc], n, want=dict(c=16, shared=1, nwin=1, nslice=16, nb=32768, lo_bits=8, nhi=128, n=16 * n, nranges=1, ps_tile=PS_TILE_BIG))
    live = [0 if h.inf[i] else k for i, k in enumerate(sc)]
    exp, einf = env.trapdoor.expected_msm(env.zkp, env.trapdoor.fr_inner_product(dev(env, live), env.d_ks[:n]))
    out, inf = env.zkp.msm_g1_dev(h.handle, dev(env, sc), n)
    assert inf == einf and np.array_equal(out, exp)


def test_refusals(env):
    zkp, torch = env.zkp, env.torch
    n = 2047
    h = bases(env, n)
    z = torch.zeros(4 * n, dtype=torch.int64, device="cuda")
    g = zkp.selftest_msm_sort_dev(h, [z], n)
    with pytest.raises(zkp.ZkpError, match="range index") as ei:
        zkp.selftest_msm_sort_dev(h, [z], n, g["nranges"])
    assert ei.value.code == zkp.ZKP_E_ARG
    with pytest.raises(zkp.ZkpError, match="more scalars than bases") as ei:
        zkp.selftest_msm_sort_dev(h, [torch.zeros(4 * (n + 1), dtype=torch.int64, device="cuda")], n + 1)
    assert ei.value.code == zkp.ZKP_E_SIZE
    with pytest.raises(zkp.ZkpError, match="null") as ei:
        zkp.selftest_msm_sort_dev(None, [z], n)
    assert ei.value.code == zkp.ZKP_E_ARG
    for short in zkp.MSM_SORT_OUTPUTS:
        out = {k: torch.empty(w - (1 if k == short else 0), dtype=torch.int32, device="cuda") for k, w in g["out_words"].items()}
        with pytest.raises(zkp.ZkpError, match="too small|null output") as ei:
            zkp.selftest_msm_sort_dev(h, [z], n, 0, out)
        assert ei.value.code == zkp.ZKP_E_ARG
