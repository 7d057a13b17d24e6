"""MSM over bounded scalars: zkp_msm_g1_bits, zkp_msm_g1_bits_dev, zkp_msm_g1_batch_bits_dev, zkp_selftest_msm_sort_bits_dev and
zkp_fr_bit_length_dev (include/zkp_hip.h; plan: csrc/msm_plan.hpp msm_bound_slices / plan_msm; kernels: csrc/msm.hpp
msm_digits_bits_kernel, fr_or_words_kernel).  The SRS is [s^i]G for a known s, so up to 65 terms the result is also compared with
[sum k_i s^i]G (zkp_hip.trapdoor); everywhere it is compared, byte for byte, with the unbounded entry on the same scalars and handle.
Two bases of every handle are flagged infinity.  Run on an MI355X with `pytest -m gpu`."""
import ctypes as C
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import msm_sort_model as S
from msm_bits_model import BITS_GLV_ONE_SET, BITS_WHOLE, R, bound_slices, edge_values, handle_table

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SECRET = 0x1F2E3D4C5B6A79881122334455667788
NPTS = 4096
INF_AT = (2, 37)  # bases flagged infinity
SIZES = (1, 65, 2047, 2048)  # 2047 / 2048: the automatic window goes from 8 to 16 bits
BITS = (1, 7, 8, 15, 16, 17, 64, 126, 127, 128, 129, 254, 255, 256)
# an unexpanded handle, expansions of 4096 points at 12 bits (22 slices of 11 / 12 bits) and at 20 (13 slices), split planes at 12
HANDLES = (None, 12, 20, ("glv", 12))
HANDLE_IDS = ["plain", "expand12", "expand20", "glv12"]


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
    s.srs = zkp_hip.srs_g1(orc.fr_from_ints([SECRET])[0], NPTS)
    s.inf = np.zeros(NPTS, dtype=np.uint8)
    s.inf[list(INF_AT)] = 1
    s.handles = {}
    return s


def handle(s, kind):
    if kind not in s.handles:
        h = s.zkp.G1Bases.from_host(s.srs, s.inf)
        if kind is not None:
            h.precompute(kind[1], glv=True) if isinstance(kind, tuple) else h.precompute(kind)
        s.handles[kind] = h
    return s.handles[kind]


def dev(s, ints):
    return s.torch.from_numpy(s.orc.fr_from_ints(ints).view(np.int64)).cuda()


def table_for(kind, n, bits):
    """(full offset table, slices the bound leaves, split flag the plan keeps)"""
    off = handle_table(kind, n)
    split = isinstance(kind, tuple)
    if bits >= BITS_WHOLE or (split and bits > BITS_GLV_ONE_SET):
        return off, len(off) - 1, split
    return off, bound_slices(off, bits), False


def bounded_scalars(seed, kind, n, bits):
    """random values below 2^bits (and below r); the edge values of the truncated table from index 0 upwards and, mirrored, from index
    n - 1 downwards, the largest value the bound allows at both ends"""
    rnd = random.Random(seed)
    top = min(1 << bits, R)
    sc = [rnd.randrange(top) for _ in range(n)]
    off, t, _ = table_for(kind, n, bits)
    zero, one, high, ones, half = (min(k, top - 1) for k in edge_values(off[:t + 1], bits))
    for j, k in enumerate((ones, zero, one, high, half)):
        if 2 * j < n:
            sc[j] = sc[n - 1 - j] = k
    return sc


def trapdoor_point(s, sc):
    e, p = 0, 1
    for i, k in enumerate(sc):
        if not s.inf[i]:
            e = (e + k * p) % R
        p = p * SECRET % R
    return s.trapdoor.expected_msm(s.zkp, e)


# ------------------------------------------------------------------------------------------------------------------ 1. parity
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", HANDLES, ids=HANDLE_IDS)
def test_parity_with_the_unbounded_entry(env, kind, n):
    h = handle(env, kind)
    for bits in BITS:
        sc = bounded_scalars(1000 * n + bits, kind, n, bits)
        assert max(sc) < min(1 << bits, R) and sc[0] == sc[n - 1] == min(1 << bits, R) - 1
        t = dev(env, sc)
        want, winf = env.zkp.msm_g1_dev(h, t, n)
        got, ginf = env.zkp.msm_g1_dev(h, t, n, bits=bits)
        assert ginf == winf and np.array_equal(got, want), (kind, n, bits)
        if n <= 65:
            exp, einf = trapdoor_point(env, sc)
            assert ginf == einf and np.array_equal(got, exp), (kind, n, bits, "trapdoor")


# ------------------------------------------------------------------------------------------------------------------ 2. geometry and stages
def run_sort(s, h, vecs, n, bits, range_index=0):
    torch = s.torch
    tensors = [dev(s, v) for v in vecs]
    g = s.zkp.selftest_msm_sort_dev(h, tensors, n, range_index, bits=bits)
    out = {k: torch.empty(max(w, 1), dtype=torch.int32, device="cuda") for k, w in g["out_words"].items()}
    g2 = s.zkp.selftest_msm_sort_dev(h, tensors, n, range_index, out, bits=bits)
    torch.cuda.synchronize()
    assert g2 == g
    W = g["nwin"]
    shape = dict(digits=(W, g["n"]), entries=(W, g["n"], 2), desc=(W, g["desc_cap"], 4))
    host = {k: out[k].cpu().numpy().view(np.uint32)[:g["out_words"][k]].reshape(shape.get(k, (W, -1))) for k in out}
    return g, host.pop("digits"), host


STAGE_CASES = [(kind, 1500, bits) for kind in HANDLES for bits in (1, 16, 64, 127, 128, 254)] + [(None, 2100, 64), (None, 2100, 17)]


@pytest.mark.parametrize("kind,n,bits", STAGE_CASES, ids=[f"{HANDLE_IDS[HANDLES.index(k)]}-{n}-{b}" for k, n, b in STAGE_CASES])
def test_geometry_and_every_sort_stage(env, kind, n, bits):
    """What a forward to the full MSM cannot pass: the plan keeps t slices, the digits are those of the truncated table"""
    h, count = handle(env, kind), 2
    off, t, split = table_for(kind, n, bits)
    vecs = [bounded_scalars(7 * bits + m, kind, n, bits) for m in range(count)]
    g, digits, out = run_sort(env, h, vecs, n, bits)
    assert g["nslice"] == t and g["off"] == off[:t + 1] and g["glv"] == int(split) and g["nranges"] == 1 and g["ns"] == n
    if kind is None:
        assert g["shared"] == 0 and g["n"] == n and g["nwin"] == t * count and g["c"] == (16 if n >= 2048 else 8)
    else:
        assert g["shared"] == 1 and g["n"] == t * n and g["nwin"] == (2 if split else 1) * count
    if isinstance(kind, tuple) and bits <= BITS_GLV_ONE_SET:
        assert g["glv"] == 0 and g["nwin"] == count
    model_geom = dict(g, off=off[:t + 1])
    ref = S.reference_digits(model_geom, vecs, env.inf[:n])
    if not np.array_equal(digits, ref):
        w, i = (int(x[0]) for x in np.nonzero(digits != ref))
        raise AssertionError(f"window {w}, stage digits, index {i}: is {int(digits[w, i]):#x}, expected {int(ref[w, i]):#x}")
    S.check_sort_outputs(g, ref, out)


@pytest.mark.parametrize("kind", HANDLES, ids=HANDLE_IDS)
def test_a_bound_of_255_is_the_unbounded_geometry(env, kind):
    n = 1500
    h = handle(env, kind)
    z = env.torch.zeros(4 * n, dtype=env.torch.int64, device="cuda")
    plain = env.zkp.selftest_msm_sort_dev(h, [z, z], n)
    assert env.zkp.selftest_msm_sort_dev(h, [z, z], n, bits=255) == plain == env.zkp.selftest_msm_sort_dev(h, [z, z], n, bits=256)
    assert env.zkp.selftest_msm_sort_dev(h, [z, z], n, bits=64)["nslice"] < plain["nslice"]


# ------------------------------------------------------------------------------------------------------------------ 3. ranges
@pytest.mark.parametrize("kind,bits", [(20, 64), (("glv", 12), 100)], ids=["expand20-64", "glv12-100"])
def test_four_scalar_ranges(env, monkeypatch, kind, bits):
    monkeypatch.setenv("ZKP_MSM_RANGE_LOG", "10")
    n = NPTS
    h = handle(env, kind)
    sc = bounded_scalars(31, kind, n, bits)
    t = dev(env, sc)
    g = env.zkp.selftest_msm_sort_dev(h, [t], n, bits=bits)
    assert g["nranges"] == 4 and g["range_len"] == 1024 and g["nslice"] == table_for(kind, n, bits)[1] and g["glv"] == 0
    got = env.zkp.msm_g1_dev(h, t, n, bits=bits)
    monkeypatch.delenv("ZKP_MSM_RANGE_LOG")
    want = env.zkp.msm_g1_dev(h, t, n)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])


# ------------------------------------------------------------------------------------------------------------------ 4. batches
@pytest.mark.parametrize("kind,count,bits", [(12, 3, 64), (20, 64, 64), (("glv", 12), 64, 127)], ids=["expand12-3", "expand20-64", "glv12-64-at-127"])
def test_batches(env, kind, count, bits):
    n = 65
    h = handle(env, kind)
    vecs = [bounded_scalars(500 + m, kind, n, bits) for m in range(count)]
    tensors = [dev(env, v) for v in vecs]
    got = env.zkp.msm_g1_batch_dev(h, tensors, n, bits=bits)
    want = [env.zkp.msm_g1_dev(h, t, n) for t in tensors]
    assert len(got) == count
    for m in range(count):
        assert got[m][1] == want[m][1] and np.array_equal(got[m][0], want[m][0]), m
    for m in (0, count - 1):
        exp, einf = trapdoor_point(env, vecs[m])
        assert got[m][1] == einf and np.array_equal(got[m][0], exp), m


def test_split_handle_keeps_its_batch_limit_from_128_bits(env):
    n = 65
    h = handle(env, ("glv", 12))
    tensors = [dev(env, bounded_scalars(600, ("glv", 12), n, 128))] * 33
    with pytest.raises(env.zkp.ZkpError, match="32 MSMs") as ei:
        env.zkp.msm_g1_batch_dev(h, tensors, n, bits=128)
    assert ei.value.code == env.zkp.ZKP_E_ARG
    got = env.zkp.msm_g1_batch_dev(h, tensors[:32], n, bits=128)
    want = env.zkp.msm_g1_dev(h, tensors[0], n)
    assert all(g[1] == want[1] and np.array_equal(g[0], want[0]) for g in got)


# ------------------------------------------------------------------------------------------------------------------ 5. refusals
SENTINEL = 0xABABABABABABABAB


def raw_bits_dev(s, h, t, n, bits):
    """zkp_msm_g1_bits_dev on sentinel-filled outputs -> (code, message, out, inf)"""
    out = np.full(12, SENTINEL, dtype=np.uint64)
    inf = C.c_uint8(0xAB)
    code = s.zkp.lib().zkp_msm_g1_bits_dev(h._h, C.c_void_p(t.data_ptr()), n, bits, None, out.ctypes.data_as(C.c_void_p), C.byref(inf))
    return code, s.zkp.lib().zkp_last_error().decode() if code else "", out, inf.value


@pytest.mark.parametrize("bits", [0, 257])
def test_bits_out_of_range(env, bits):
    h = handle(env, 12)
    t = dev(env, [1] * 65)
    code, msg, out, inf = raw_bits_dev(env, h, t, 65, bits)
    assert code == env.zkp.ZKP_E_ARG and "1..256" in msg and np.all(out == SENTINEL) and inf == 0xAB
    with pytest.raises(env.zkp.ZkpError) as ei:
        env.zkp.msm_g1_batch_dev(h, [t], 65, bits=bits)
    assert ei.value.code == env.zkp.ZKP_E_ARG
    with pytest.raises(env.zkp.ZkpError) as ei:
        env.zkp.msm_g1(h, env.orc.fr_from_ints([1] * 65), bits=bits)
    assert ei.value.code == env.zkp.ZKP_E_ARG
    with pytest.raises(env.zkp.ZkpError) as ei:
        env.zkp.selftest_msm_sort_dev(h, [t], 65, bits=bits)
    assert ei.value.code == env.zkp.ZKP_E_ARG


@pytest.mark.parametrize("kind,n,bits,at", [(None, 2047, 64, 0), (None, 2048, 64, 2047), (12, 65, 16, 0), (20, 2048, 64, 2047),
                                            (("glv", 12), 2048, 127, 2047), (("glv", 12), 2048, 200, 0), (12, 65, 254, 64)],
                         ids=["plain8-first", "plain16-last", "expand12-first", "expand20-last", "glv12-one-set-last", "glv12-two-sets-first", "254"])
def test_a_scalar_at_the_bound_is_refused(env, kind, n, bits, at):
    h = handle(env, kind)
    sc = bounded_scalars(77, kind, n, bits)
    good = dev(env, sc)
    bad = list(sc)
    bad[at] = 1 << bits
    code, msg, out, inf = raw_bits_dev(env, h, dev(env, bad), n, bits)
    assert code == env.zkp.ZKP_E_ARG and f"scalar {at} of vector 0" in msg and f"2^{bits}" in msg, msg
    assert np.all(out == SENTINEL) and inf == 0xAB
    # the handle and the workspaces serve the next call
    want = env.zkp.msm_g1_dev(h, good, n)
    got = env.zkp.msm_g1_dev(h, good, n, bits=bits)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    if n <= 65:
        exp, einf = trapdoor_point(env, sc)
        assert got[1] == einf and np.array_equal(got[0], exp)


def test_violation_in_the_last_of_four_ranges(env, monkeypatch):
    monkeypatch.setenv("ZKP_MSM_RANGE_LOG", "10")
    n, bits, at = NPTS, 64, 3 * 1024 + 5
    h = handle(env, 20)
    sc = bounded_scalars(78, 20, n, bits)
    bad = list(sc)
    bad[at] = 1 << bits
    assert env.zkp.selftest_msm_sort_dev(h, [dev(env, sc)], n, bits=bits)["nranges"] == 4
    code, msg, out, inf = raw_bits_dev(env, h, dev(env, bad), n, bits)
    assert code == env.zkp.ZKP_E_ARG and f"scalar {at} of vector 0" in msg, msg
    assert np.all(out == SENTINEL) and inf == 0xAB
    got = env.zkp.msm_g1_dev(h, dev(env, sc), n, bits=bits)
    monkeypatch.delenv("ZKP_MSM_RANGE_LOG")
    want = env.zkp.msm_g1_dev(h, dev(env, sc), n)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])


def test_violation_in_vector_2_of_a_batch(env):
    n, bits, at = 65, 64, 33
    h = handle(env, 12)
    vecs = [bounded_scalars(80 + m, 12, n, bits) for m in range(3)]
    bad = [list(v) for v in vecs]
    bad[2][at] = 1 << bits
    tensors = [dev(env, v) for v in bad]
    ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in tensors])
    xy, inf = np.full((3, 12), SENTINEL, dtype=np.uint64), np.full(3, 0xAB, dtype=np.uint8)
    code = env.zkp.lib().zkp_msm_g1_batch_bits_dev(h._h, ptrs, 3, n, bits, None, xy.ctypes.data_as(C.c_void_p), inf.ctypes.data_as(C.c_void_p))
    msg = env.zkp.lib().zkp_last_error().decode()
    assert code == env.zkp.ZKP_E_ARG and f"scalar {at} of vector 2" in msg and "2^64" in msg, msg
    assert np.all(xy == SENTINEL) and np.all(inf == 0xAB)
    got = env.zkp.msm_g1_batch_dev(h, [dev(env, v) for v in vecs], n, bits=bits)
    for m in range(3):
        exp, einf = trapdoor_point(env, vecs[m])
        assert got[m][1] == einf and np.array_equal(got[m][0], exp), m


def test_host_scalar_violation(env):
    n, bits, at = NPTS, 32, 4000
    h = handle(env, 20)
    sc = bounded_scalars(90, 20, n, bits)
    bad = list(sc)
    bad[at] = 1 << bits
    with pytest.raises(env.zkp.ZkpError, match=f"scalar {at} of vector 0") as ei:
        env.zkp.msm_g1(h, env.orc.fr_from_ints(bad), bits=bits)
    assert ei.value.code == env.zkp.ZKP_E_ARG
    got, want = env.zkp.msm_g1(h, env.orc.fr_from_ints(sc), bits=bits), env.zkp.msm_g1(h, env.orc.fr_from_ints(sc))
    assert got[1] == want[1] and np.array_equal(got[0], want[0])


def test_a_sharded_handle_is_refused():
    """own process: it initialises the library with two slots, as tests/multi_slot_worker.py does"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "msm_bits_sharded_worker.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "OK sharded refusal" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])


# ------------------------------------------------------------------------------------------------------------------ 6. host scalars
@pytest.mark.parametrize("kind", HANDLES, ids=HANDLE_IDS)
def test_host_scalars(env, kind):
    n = NPTS
    h = handle(env, kind)
    for bits in (8, 64, 127, 128):
        sc = env.orc.fr_from_ints(bounded_scalars(40 + bits, kind, n, bits))
        got, want = env.zkp.msm_g1(h, sc, bits=bits), env.zkp.msm_g1(h, sc)
        assert got[1] == want[1] and np.array_equal(got[0], want[0]), (kind, bits)


def test_host_scalars_fed_in_ranges(env):
    """2^19 terms over a 20-bit expansion: where zkp_msm_g1 starts to upload its scalars range by range under the kernels"""
    zkp, torch = env.zkp, env.torch
    n, bits = 1 << 19, 64
    ks = torch.from_numpy(env.orc.rand_fr(0xB175, n).view(np.int64)).cuda()
    pts = torch.zeros(n * 12, dtype=torch.int64, device="cuda")
    zkp.g1_fixed_base_mul_dev(ks, n, pts)
    h = zkp.G1Bases.from_device(pts, n)
    torch.cuda.synchronize()
    h.precompute(20)
    rnd = random.Random(5)
    vals = [rnd.getrandbits(64) for _ in range(n)]
    vals[0] = vals[n - 1] = (1 << 64) - 1
    mont = env.orc.fr_from_ints(vals)
    t = torch.from_numpy(mont.view(np.int64)).cuda()
    g = zkp.selftest_msm_sort_dev(h, [t], n, bits=bits)
    assert g["nslice"] == 4 and g["shared"] == 1
    got, want = zkp.msm_g1(h, mont, bits=bits), zkp.msm_g1(h, mont)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    exp = env.trapdoor.expected_msm(zkp, env.trapdoor.fr_inner_product(t, ks))
    assert got[1] == exp[1] and np.array_equal(got[0], exp[0])


# ------------------------------------------------------------------------------------------------------------------ 7. bit length
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 100003])
def test_fr_bit_length(env, n):
    zkp = env.zkp
    if n == 0:
        assert zkp.fr_bit_length_dev(env.torch.zeros(4, dtype=env.torch.int64, device="cuda"), 0) == 0
        return
    rnd = random.Random(n)
    assert zkp.fr_bit_length_dev(dev(env, [0] * n), n) == 0
    for width in (1, 31, 32, 33, 64, 127, 200, 254):
        base = [rnd.randrange(1 << (width - 1)) for _ in range(n)]
        for at in (0, n - 1):
            v = list(base)
            v[at] = (1 << (width - 1)) + rnd.randrange(1 << (width - 1))
            assert zkp.fr_bit_length_dev(dev(env, v), n) == max(k.bit_length() for k in v) == width, (n, width, at)
    v = [rnd.randrange(1 << 64) for _ in range(n)]
    v[n // 2] = R - 1
    assert zkp.fr_bit_length_dev(dev(env, v), n) == (R - 1).bit_length() == 255


def test_fr_bit_length_of_every_power_of_two(env):
    pw = [1 << k for k in range(255)]
    assert env.zkp.fr_bit_length_dev(dev(env, pw), len(pw)) == 255
    for top in (1, 32, 33, 100, 254):
        assert env.zkp.fr_bit_length_dev(dev(env, pw[:top]), top) == top
    # the bound it reports is one the bounded entry accepts, and one bit less is refused
    h = handle(env, 12)
    t = dev(env, pw[:65])
    bits = env.zkp.fr_bit_length_dev(t, 65)
    assert bits == 65
    want = env.zkp.msm_g1_dev(h, t, 65)
    got = env.zkp.msm_g1_dev(h, t, 65, bits=bits)
    assert got[1] == want[1] and np.array_equal(got[0], want[0])
    with pytest.raises(env.zkp.ZkpError, match="scalar 64 of vector 0"):
        env.zkp.msm_g1_dev(h, t, 65, bits=bits - 1)
