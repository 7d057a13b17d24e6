"""The polynomial layer under the PLONK prover, zkp_kzg_open and Nova's openings (csrc/plonk.hpp), one helper at a time through
zkp_selftest_poly_*_dev: the three-launch scan, fr_scale_pow_kernel, the division by (X - z), fr_poly_eval_kernel, fr_lincomb_kernel and
fr_trim_len_kernel at the sizes where their structure changes -- elements per thread, the 64-lane shuffles and the four wave totals,
256-thread workgroups, more than one total per thread in the middle launch, the power table indexed by the bits of the thread id, two
jobs of unequal length under one grid.  Every expected value is computed here in Python integers mod r from the definition; every
comparison is exact equality of all output words.

Run on an MI355X with `pytest -m gpu tests/test_gpu_poly_primitives.py`."""
import random

import numpy as np
import pytest

import bigmodel as M

pytestmark = pytest.mark.gpu
R = M.R
MONT = M.FR_MONT_R
MONT_INV = pow(MONT, -1, R)
SENTINEL = 0x5E5E5E5E5E5E5E5E  # every word of an output buffer before a call: 4 such words are no canonical residue
FLAGS = [(0, 0), (0, 1), (1, 0), (1, 1)]  # (rev, excl)


@pytest.fixture(scope="module")
def zkp(orc):
    import torch
    assert torch.cuda.is_available()
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


# ---- plain integers <-> memory form --------------------------------------------------------------------------------------------
def pack(vals):
    """python ints -> (n, 4) uint64 Montgomery limbs"""
    if not len(vals):
        return np.zeros((0, 4), dtype=np.uint64)
    return np.frombuffer(b"".join((v * MONT % R).to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def unpack(a):
    raw = np.ascontiguousarray(a, dtype=np.uint64).tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") * MONT_INV % R for i in range(0, len(raw), 32)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).reshape(-1)).cuda()


def sentinel(n):
    """a device buffer of n elements (plus 4 guard elements behind them) filled with SENTINEL words"""
    import torch
    return torch.full((4 * (n + 4),), SENTINEL, dtype=torch.int64, device="cuda")


def read(t, n):
    """-> the first n elements of t; the rest must still be sentinel words (nothing wrote past the end)"""
    a = t.cpu().numpy().view(np.uint64).reshape(-1, 4)
    assert (a[n:] == np.uint64(SENTINEL)).all(), "written past the end of the output"
    return a[:n]


def rand_vals(seed, n, plant=(0, 1, R - 1)):
    """n random field elements with the values of `plant` at spread positions (as many as fit)"""
    rng = random.Random(seed)
    v = [rng.getrandbits(256) % R or 5 for _ in range(n)]
    for k, x in enumerate(plant):
        if k < n:
            v[(n * (2 * k + 1)) // (2 * len(plant) + 1)] = x
    return v


# ---- the definitions -----------------------------------------------------------------------------------------------------------
def scan_def(v, op, rev, excl):
    """forward inclusive op_{j<=i}, exclusive op_{j<i}; suffix inclusive op_{j>=i}, exclusive op_{j>i}"""
    src = v[::-1] if rev else v
    out, acc = [], (0 if op == "add" else 1)
    for x in src:
        nxt = (acc + x) % R if op == "add" else acc * x % R
        out.append(acc if excl else nxt)
        acc = nxt
    return out[::-1] if rev else out


def div_def(c, z):
    """q_j = sum_{i>j} c_i z^(i-j-1), len - 1 outputs (q_{len-2} = c_{len-1}, q_j = c_{j+1} + z q_{j+1})"""
    q = [0] * max(len(c) - 1, 0)
    acc = 0
    for j in range(len(c) - 2, -1, -1):
        acc = (acc * z + c[j + 1]) % R
        q[j] = acc
    return q


def eval_def(c, z):
    acc, pw = 0, 1
    for x in c:
        acc = (acc + x * pw) % R
        pw = pw * z % R
    return acc


def trim_def(v):
    return max((i + 1 for i, x in enumerate(v) if x), default=0)


def scan_inputs(seed, n, op):
    """add: 0, 1 and r - 1 planted.  mul: two inputs -- one with a single zero in the middle (everything behind it in scan order is zero,
    everything before it untouched), one with no zero at all, so that products also cross every workgroup boundary"""
    if op == "add":
        return [rand_vals(seed, n)]
    with_zero = rand_vals(seed, n, plant=(1, R - 1))
    with_zero[n // 2] = 0
    return [with_zero, rand_vals(seed + 1, n, plant=(1, R - 1))]


def run_scan(zkp, op, jobs, chunk):
    """jobs: (d_in, n, rev, excl) -> the outputs"""
    outs = [sentinel(n) for _, n, _, _ in jobs]
    zkp.selftest_poly_scan_dev(op, [(d, o, n, rev, excl) for (d, n, rev, excl), o in zip(jobs, outs)], chunk)
    return [read(o, n) for o, (_, n, _, _) in zip(outs, jobs)]


def scan_sizes(c):
    return sorted({1, 2, 63, 64, 65, 255, 256, 257, 256 * c - 1, 256 * c, 256 * c + 1, 512 * c + 7})


@pytest.mark.parametrize("op", ["add", "mul"])
@pytest.mark.parametrize("chunk", [1, 2, 3, 16])
def test_scan_at_wave_workgroup_and_chunk_edges(zkp, op, chunk):
    """Every n alone under the four rev / excl combinations, then as a two-job batch with a second job of max(1, n // 3) elements and
    other flags, in either order: the shorter job's workgroups run past its end and leave their rows of the scratch unwritten."""
    for n in scan_sizes(chunk):
        m = max(1, n // 3)
        for k, v in enumerate(scan_inputs(1000 * chunk + n, n, op)):
            v2 = scan_inputs(77000 * chunk + n, m, op)[k]
            d_v, d_v2 = dev(pack(v)), dev(pack(v2))
            want = {f: pack(scan_def(v, op, *f)) for f in FLAGS}
            want2 = {f: pack(scan_def(v2, op, *f)) for f in FLAGS}
            if op == "mul" and k == 0 and n > 2:  # the planted zero: zero behind it, the running product before it
                fwd = unpack(want[(0, 0)])
                assert all(fwd[:n // 2]) and not any(fwd[n // 2:])
            for i, f in enumerate(FLAGS):
                got, = run_scan(zkp, op, [(d_v, n, *f)], chunk)
                assert np.array_equal(got, want[f]), (op, chunk, n, k, f)
                f2 = FLAGS[(i + 1) % 4]
                jobs = [(d_v, n, *f), (d_v2, m, *f2)]
                exp = [want[f], want2[f2]]
                if i & 1:  # the shorter job in row 0 of the grid
                    jobs, exp = jobs[::-1], exp[::-1]
                got = run_scan(zkp, op, jobs, chunk)
                assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1]), (op, chunk, n, k, f, f2)


@pytest.mark.parametrize("op", ["add", "mul"])
@pytest.mark.parametrize("chunk,n", [(1, 65537), (2, 2 * 65536 + 1),                                   # per = 2 in scan_mid_kernel
                                     (0, 65536), (0, 65537), (0, 131071), (0, 131072), (0, 131073)])  # the rule, where it changes
def test_scan_with_two_totals_per_thread_and_by_the_production_rule(zkp, op, chunk, n):
    """More than 256 workgroups: a thread of the middle launch takes two totals.  chunk 0: scan_chunk_for and the scratch bound of
    scan_scratch_elems on both sides of 2^16 + 1 (257 workgroups) and of 2^17 (one, then two elements per thread)."""
    v = scan_inputs(31 * n + chunk, n, op)[0]
    d_v = dev(pack(v))
    for f in ((0, 0), (1, 1)):
        got, = run_scan(zkp, op, [(d_v, n, *f)], chunk)
        assert np.array_equal(got, pack(scan_def(v, op, *f))), (op, chunk, n, f)


def test_scan_in_place(zkp):
    """d_out == d_in of the same job is the one overlap the scan allows (the apply launch reads and writes index i in one thread)."""
    n = 777
    for op, f in (("add", (1, 1)), ("mul", (0, 0))):
        w = scan_inputs(6, n, op)[-1]
        d = dev(np.concatenate([pack(w), np.full((4, 4), SENTINEL, dtype=np.uint64)]))
        zkp.selftest_poly_scan_dev(op, [(d, d, n, *f)], 2)
        assert np.array_equal(read(d, n), pack(scan_def(w, op, *f))), (op, f)


# ---- out[i] = in[i] * base^(i + e0) ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("base_kind", ["one", "minus_one", "random"])
@pytest.mark.parametrize("chunk", [1, 2, 3, 8])
def test_scale_pow_power_table_up_to_bit_16(zkp, chunk, base_kind):
    """n = 65536 chunk + 1 is the first size at which a thread id has bit 16 set: the last element's power reads bp[16]."""
    base = {"one": 1, "minus_one": R - 1, "random": rand_vals(900 + chunk, 1, plant=())[0]}[base_kind]
    b = pack([base])[0]
    for n in (1, 255 * chunk, 256 * chunk, 256 * chunk + 1, 65536 * chunk + 1):
        v = rand_vals(4000 * chunk + n, n)
        d_v = dev(pack(v))
        pw = [1] * (n + 1)
        for i in range(1, n + 1):
            pw[i] = pw[i - 1] * base % R
        for e0 in (0, 1):
            out = sentinel(n)
            zkp.selftest_poly_scale_pow_dev(d_v, n, b, e0, out, chunk)
            assert np.array_equal(read(out, n), pack([x * pw[i + e0] % R for i, x in enumerate(v)])), (chunk, base_kind, n, e0)


def test_scale_pow_by_the_production_rule(zkp):
    """chunk 0 at the first length with two elements per thread (2^17) and just below it"""
    base = rand_vals(17, 1, plant=())[0]
    for n in (131071, 131072):
        v = rand_vals(n, n)
        out = sentinel(n)
        zkp.selftest_poly_scale_pow_dev(dev(pack(v)), n, pack([base])[0], 1, out, 0)
        want, pw = [], base
        for x in v:
            want.append(x * pw % R)
            pw = pw * base % R
        assert np.array_equal(read(out, n), pack(want)), n


# ---- (c(X) - c(z)) / (X - z) -----------------------------------------------------------------------------------------------------------
def check_quotient(got, c, z, tag):
    """the direct formula, and q(X) (X - z) + c(z) = c(X) multiplied back"""
    assert np.array_equal(got, pack(div_def(c, z))), tag
    q = unpack(got)
    y = eval_def(c, z)
    back = [(y - z * q[0]) % R] + [(q[j - 1] - z * q[j]) % R for j in range(1, len(q))] + [q[-1]] if q else [y]
    assert back == [x % R for x in c], tag


def run_div(zkp, reqs, chunk):
    """reqs: (d_c, len, z) -> quotients"""
    outs = [sentinel(max(n, 1) - 1) for _, n, _ in reqs]
    zkp.selftest_poly_div_linear_dev([(d, n, pack([z])[0], o) for (d, n, z), o in zip(reqs, outs)], chunk)
    return [read(o, max(n, 1) - 1) for o, (_, n, _) in zip(outs, reqs)]


@pytest.mark.parametrize("chunk", [1, 2, 8])
def test_div_linear_single(zkp, chunk):
    """z = 0 is the copy path; len <= 1 writes nothing (read() checks that the whole buffer still holds the sentinel)."""
    zr = rand_vals(50 + chunk, 1, plant=())[0]
    for n in (1, 2, 3, 64, 65, 257, 256 * chunk + 2, 4096, 4097):
        c = rand_vals(600 * chunk + n, n)
        c[-1] = c[-1] or 9
        d_c = dev(pack(c))
        for z in (0, 1, R - 1, zr):
            got, = run_div(zkp, [(d_c, n, z)], chunk)
            check_quotient(got, c, z, (chunk, n, z))


@pytest.mark.parametrize("chunk", [1, 2, 8])
def test_div_linear_batches_of_unequal_length(zkp, chunk):
    za, zb = rand_vals(70 + chunk, 2, plant=())
    for (na, z0), (nb, z1) in [((4097, za), (65, zb)), ((65, za), (4097, zb)), ((257, 0), (4096, zb)), ((256 * chunk + 2, 1), (3, R - 1)),
                               ((1, za), (64, zb)), ((4096, za), (2, 0)), ((300, 0), (7, 0))]:
        ca, cb = rand_vals(8000 * chunk + na, na), rand_vals(9000 * chunk + nb, nb)
        got = run_div(zkp, [(dev(pack(ca)), na, z0), (dev(pack(cb)), nb, z1)], chunk)
        check_quotient(got[0], ca, z0, (chunk, na, nb, 0))
        check_quotient(got[1], cb, z1, (chunk, na, nb, 1))


# ---- sum c_i z^i ---------------------------------------------------------------------------------------------------------------------------
def test_eval_eight_requests_per_launch(zkp):
    """256 x EVAL_CHUNK = 2048 coefficients make one workgroup: lengths on both sides of one thread, one workgroup and two; the second
    launch has the lengths in reverse order, so every request's first partial sits elsewhere."""
    lens = [0, 1, 8, 9, 2047, 2048, 2049, 4097]
    zr = rand_vals(3, 5, plant=())
    zs = zr[:4] + [0, 1, R - 1] + zr[4:]  # distinct points; 0, 1 and r - 1 on the lengths around one workgroup
    polys = [rand_vals(100 + n, n) for n in lens]
    d = [dev(pack(c)) for c in polys]
    want = [eval_def(c, z) for c, z in zip(polys, zs)]
    assert want[0] == 0 and want[4] == polys[4][0] and want[5] == sum(polys[5]) % R  # len 0, z = 0, z = 1
    order = list(range(8))
    for perm in (order, order[::-1], [7, 0, 6, 1, 5, 2, 4, 3]):
        got = zkp.selftest_poly_eval_dev([(d[i], lens[i], pack([zs[i]])[0]) for i in perm])
        assert np.array_equal(got, pack([want[i] for i in perm])), perm
    # every point on the longest polynomial, one launch
    got = zkp.selftest_poly_eval_dev([(d[7], 4097, pack([z])[0]) for z in zs])
    assert np.array_equal(got, pack([eval_def(polys[7], z) for z in zs]))
    assert zkp.selftest_poly_eval_dev([]).shape == (0, 4)


# ---- sum_k s_k p_k[i] ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_out", [1, 255, 256, 257, 1000])
def test_lincomb_term_ends_around_the_output_length(zkp, n_out):
    def run(terms):
        out = sentinel(n_out)
        zkp.selftest_poly_lincomb_dev([(dev(pack(p)), len(p), pack([s])[0]) for p, s in terms], n_out, out)
        want = [sum(s * p[i] for p, s in terms if i < len(p)) % R for i in range(n_out)]
        assert np.array_equal(read(out, n_out), pack(want)), (n_out, [len(p) for p, _ in terms])

    s = rand_vals(n_out, 12, plant=())
    for ln in (n_out - 1, n_out, n_out + 1, 0):  # one term: below, equal to, above the output length, and empty
        run([(rand_vals(10 * n_out + ln, ln), s[0])])
    run([(rand_vals(n_out, n_out), 0)])      # a zero scalar
    run([(rand_vals(n_out, n_out), R - 1)])
    lens = [n_out, n_out + 5, n_out - 1, 0, n_out // 2, n_out, 64 % (n_out + 1), n_out + 300, 255 % (n_out + 1), n_out, 1, n_out - 1]
    s[5] = 0  # a full-length term with a zero scalar
    s[9] = 1
    run([(rand_vals(20 * n_out + k, ln), s[k]) for k, ln in enumerate(lens)])


# ---- highest non-zero index + 1 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1000])
def test_trim_len_last_nonzero_on_lane_and_workgroup_edges(zkp, n):
    assert zkp.selftest_poly_trim_len_dev(dev(pack([0] * n)), n) == 0
    rng = random.Random(n)
    for last in sorted({p for p in (0, 62, 63, 64, 255, 256, n - 1) if p < n}):
        v = [0] * n
        v[last] = R - 1
        assert zkp.selftest_poly_trim_len_dev(dev(pack(v)), n) == last + 1, (n, last, "alone")
        for i in range(last):  # non-zeros scattered below it
            if rng.random() < 0.3:
                v[i] = rng.getrandbits(200) + 1
        assert trim_def(v) == last + 1
        assert zkp.selftest_poly_trim_len_dev(dev(pack(v)), n) == last + 1, (n, last)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_and_a_valid_call_still_works(zkp):
    import ctypes as C
    n = 300
    v = rand_vals(1, n)
    d, o, o2 = dev(pack(v)), sentinel(n), sentinel(n)
    one = pack([1])[0]
    L = zkp.lib()

    def refused(code, fn, *args):
        with pytest.raises(zkp.ZkpError) as ei:
            fn(*args)
        assert ei.value.code == code, str(ei.value)

    E = zkp.ZKP_E_ARG
    refused(E, zkp.selftest_poly_scan_dev, "add", [(None, o, n, 0, 0)])                                   # null pointers
    refused(E, zkp.selftest_poly_scan_dev, "add", [(d, None, n, 0, 0)])
    refused(E, zkp.selftest_poly_scan_dev, "add", [(d, o, n, 0, 0)], 17)                                   # chunk out of range
    refused(E, zkp.selftest_poly_scan_dev, "add", [])                                                      # no job, three jobs
    refused(E, zkp.selftest_poly_scan_dev, "mul", [(d, o, n, 0, 0), (d, o2, n, 1, 0), (d, sentinel(n), n, 1, 1)])
    refused(E, zkp.selftest_poly_scan_dev, "add", [(d, o, n, 0, 0), (d, o, n, 1, 0)])                      # both jobs into one output
    refused(E, zkp.selftest_poly_scan_dev, "add", [(d, o, n, 0, 0), (o, o2, n, 1, 0)])                     # job 1 reads what job 0 writes
    refused(E, zkp.selftest_poly_scan_dev, "add", [(d[4:], d, n - 1, 0, 0)])                               # shifted overlap
    refused(E, zkp.selftest_poly_scale_pow_dev, None, n, one, 0, o)
    refused(E, zkp.selftest_poly_scale_pow_dev, d, n, one, 0, o, 9)
    refused(E, zkp.selftest_poly_scale_pow_dev, d[4:], n - 1, one, 0, d)
    refused(E, zkp.selftest_poly_div_linear_dev, [(d, n, one, None)])
    refused(E, zkp.selftest_poly_div_linear_dev, [(d, n, one, o)], 9)
    refused(E, zkp.selftest_poly_div_linear_dev, [(d, n, one, o), (d, n, one, o2), (d, n, one, sentinel(n))])
    refused(E, zkp.selftest_poly_div_linear_dev, [(d, n, one, d)])                                         # out aliasing in
    refused(E, zkp.selftest_poly_div_linear_dev, [(d, n, one, o), (o, n, one, o2)])
    refused(E, zkp.selftest_poly_eval_dev, [(d, n, one)] * 9)
    refused(E, zkp.selftest_poly_eval_dev, [(None, n, one)])
    refused(E, zkp.selftest_poly_lincomb_dev, [(d, n, one)] * 13, n, o)
    refused(E, zkp.selftest_poly_lincomb_dev, [(None, n, one)], n, o)
    refused(E, zkp.selftest_poly_lincomb_dev, [(d, n, one)], n, None)
    refused(E, zkp.selftest_poly_lincomb_dev, [(d[4:], n - 1, one)], n - 1, d)
    refused(E, zkp.selftest_poly_trim_len_dev, None, n)
    # a size whose scratch would not fit: refused on the length alone, before any pointer is used
    big = (1 << 22) + 1
    ptr, sz = C.c_void_p(d.data_ptr()), C.c_size_t(big)
    optr, flags, res = C.c_void_p(o.data_ptr()), C.c_uint(0), C.c_size_t(0)
    assert L.zkp_selftest_poly_scan_dev(0, 1, C.byref(ptr), C.byref(optr), C.byref(sz), C.byref(flags), 0, None) == zkp.ZKP_E_SIZE
    assert L.zkp_selftest_poly_scale_pow_dev(ptr, big, one.ctypes.data_as(C.c_void_p), 0, 0, optr, None) == zkp.ZKP_E_SIZE
    assert L.zkp_selftest_poly_div_linear_dev(1, C.byref(ptr), C.byref(sz), one.ctypes.data_as(C.c_void_p), C.byref(optr), 0, None) == zkp.ZKP_E_SIZE
    assert L.zkp_selftest_poly_eval_dev(1, C.byref(ptr), C.byref(sz), one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), None) == zkp.ZKP_E_SIZE
    assert L.zkp_selftest_poly_lincomb_dev(1, C.byref(ptr), C.byref(sz), one.ctypes.data_as(C.c_void_p), 1, optr, None) == zkp.ZKP_E_SIZE
    assert L.zkp_selftest_poly_trim_len_dev(ptr, big, C.byref(res), None) == zkp.ZKP_E_SIZE
    # nothing was written by any of them, and the hooks still work
    assert (o.cpu().numpy().view(np.uint64) == np.uint64(SENTINEL)).all()
    assert np.array_equal(d.cpu().numpy().view(np.uint64).reshape(-1, 4), pack(v))
    got, = run_scan(zkp, "add", [(d, n, 1, 0)], 0)
    assert np.array_equal(got, pack(scan_def(v, "add", 1, 0)))
    z = 12345
    got, = run_div(zkp, [(d, n, z)], 0)
    check_quotient(got, v, z, "after refusals")
    assert np.array_equal(zkp.selftest_poly_eval_dev([(d, n, pack([z])[0])]), pack([eval_def(v, z)]))
    assert zkp.selftest_poly_trim_len_dev(d, n) == trim_def(v)
