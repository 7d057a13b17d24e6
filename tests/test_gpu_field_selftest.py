"""The device field products and G1 adds lane by lane at their contract edges (zkp_selftest_*_dev, csrc/selftest.hip), bit-exact against
the limb model (tests/model/limb_model.py) on the vectors of tests/field_vectors.py.  No tolerances: every output word is compared.

Every vector goes through the model first; the model raises on anything out of contract, so no case is dropped on the way.
Run on an MI355X with `pytest -m gpu tests/test_gpu_field_selftest.py`."""
import random

import numpy as np
import pytest

import bigmodel as M
import field_vectors as V
import limb_model as L

pytestmark = pytest.mark.gpu

P, R = M.P, M.R


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def run_field(zkp, family, op, slots):
    """slots: per case a tuple of up to four operand word lists -> per case the 32 output words"""
    import torch
    n = len(slots)
    words = np.zeros((n, 4, 16), dtype=np.uint32)
    for i, ops in enumerate(slots):
        for j, o in enumerate(ops):
            words[i, j, :len(o)] = o
    d_in = torch.from_numpy(words.view(np.int32).reshape(-1)).cuda()
    d_out = torch.full((n * 32,), -1, dtype=torch.int32, device="cuda")
    zkp.selftest_field_dev(family, op, d_in, n, d_out)
    torch.cuda.synchronize()
    return d_out.cpu().numpy().view(np.uint32).reshape(n, 2, 16).tolist()


def check(got, want, *_widths):
    """got: the two result slots of every case; want: per case (slot 0 words, slot 1 words or None); everything else must be zero"""
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        w0, w1 = w if isinstance(w, tuple) else (w, [])
        assert g[0] == list(w0) + [0] * (16 - len(w0)), (i, "slot 0")
        assert g[1] == list(w1) + [0] * (16 - len(w1)), (i, "slot 1")


# ----------------------------------------------------------------------------------------------------------------- Fq28
@pytest.mark.parametrize("op", ["mul_inline", "mul_chain"])
def test_fq28_product(zkp, op):
    """fq28_mul_inline / fq28_mul_chain: limbs up to 2^30 - 1, value products at and under 2520 p^2, results exactly 0 and exactly p"""
    cases = V.fq28_mul_cases()
    check(run_field(zkp, "fq28", op, cases), [L.fq28_mul(a, b) for a, b in cases], 14)


def fq28_mul_quads():
    c = V.fq28_mul_cases()
    c = c + c[:1] if len(c) % 2 else c
    return [(c[i][0], c[i][1], c[-1 - i][0], c[-1 - i][1]) for i in range(len(c))]


def test_fq28_mul_chain2(zkp):
    """fq28_mul_chain2: two interleaved products per lane"""
    quads = fq28_mul_quads()
    check(run_field(zkp, "fq28", "mul_chain2", quads), [(L.fq28_mul(a, b), L.fq28_mul(cc, d)) for a, b, cc, d in quads], 14, 14)


def test_fq28_mul_chain2_inplace(zkp):
    """fq28_mul_chain2_inplace: the same two products, each written over its first operand (slot 0 = a b, slot 1 = c d)"""
    quads = fq28_mul_quads()
    check(run_field(zkp, "fq28", "mul_chain2_inplace", quads), [(L.fq28_mul(a, b), L.fq28_mul(cc, d)) for a, b, cc, d in quads], 14, 14)


@pytest.mark.parametrize("op", ["sqr", "sqr_chain"])
def test_fq28_square(zkp, op):
    """sqr (a * a) and fq28_sqr_chain (doubled operand): limbs up to 2^30 - 1, values up to sqrt(2520) p"""
    cases = V.fq28_sqr_cases()
    check(run_field(zkp, "fq28", op, [(a,) for a in cases]), [L.fq28_sqr(a) for a in cases], 14)


@pytest.mark.parametrize("op", ["mul2", "mul2_chain"])
def test_fq28_two_product_reduction(zkp, op):
    """fq28_mul2 / fq28_mul2_chain: 18p * 18p + 8p * 2p (xyzz_finish) and a b + c d = 2520 p^2 itself"""
    cases = V.fq28_mul2_cases()
    check(run_field(zkp, "fq28", op, cases), [L.fq28_mul2(*c) for c in cases], 14)


@pytest.mark.parametrize("op", ["sub4", "sub8", "sub16", "sub8w"])
def test_fq28_borrow_free_subtraction(zkp, op):
    """sub4 / sub8 / sub16 / sub8w: subtrahends up to the documented bound and equal to the K p constant limb for limb"""
    cases = V.fq28_sub_cases(op)
    check(run_field(zkp, "fq28", op, cases), [getattr(L, "fq28_" + op)(a, b) for a, b in cases], 14)


def test_fq28_neg4(zkp):
    cases = V.fq28_neg4_cases()
    check(run_field(zkp, "fq28", "neg4", [(a,) for a in cases]), [L.fq28_neg4(a) for a in cases], 14)


def test_fq28_normalise(zkp):
    cases = V.fq28_normalise_cases()
    check(run_field(zkp, "fq28", "normalise", [(a,) for a in cases]), [L.fq28_normalise(a) for a in cases], 14)


def test_fq28_tight_is_zero_mod_p(zkp):
    """exactly 0 and exactly p are the zeros; p and 0 with one bit of one limb flipped are not"""
    cases = V.fq28_is_zero_cases()
    cases += [L.fq28_mul(a, b) for a, b in V.fq28_mul_cases()[::7]]          # and as products leave it: some exactly p, some exactly 0
    want = [[1 if L.fq28_tight_is_zero_mod_p(a) else 0] for a in cases]
    assert sum(w[0] for w in want) >= 4
    check(run_field(zkp, "fq28", "is_zero", [(a,) for a in cases]), want, 1)


def test_fq28_from_sat(zkp):
    cases = V.words_cases(12, 0x5A7, [P - 1, P, 1, (1 << 384) % P])
    check(run_field(zkp, "fq28", "from_sat", [(w,) for w in cases]), [L.fq28_from_sat(w) for w in cases], 14)


# ----------------------------------------------------------------------------------------------------------------- Fr29
def test_fr29_product(zkp):
    """Fr29 operator*: limbs of a up to 2^31 - 1, of b up to 2^29 - 1, value products at and under 70 r^2"""
    cases = V.fr29_mul_cases()
    check(run_field(zkp, "fr29", "mul", cases), [L.fr29_mul(a, b) for a, b in cases], 9)


def test_fr29_mul2(zkp):
    """fr29_mul2 (asm): both products"""
    c = V.fr29_mul_cases()
    quads = [(c[i][0], c[i][1], c[-1 - i][0], c[-1 - i][1]) for i in range(len(c))]
    check(run_field(zkp, "fr29", "mul2", quads), [(L.fr29_mul(a, b), L.fr29_mul(cc, d)) for a, b, cc, d in quads], 9, 9)


def test_fr29_to_canonical(zkp):
    """k r - 1, k r, k r + 1 for k = 0..70, 2^261 - 1, unnormalised limbs up to 2^31, and values where QEST is one short"""
    cases = V.fr29_to_canonical_cases()
    check(run_field(zkp, "fr29", "to_canonical", [(a,) for a in cases]), [L.fr29_to_canonical(a)[0] for a in cases], 8)


def test_fr_memory_form_product(zkp):
    """Fr operator* on memory-form words, canonical operands and any others below 2^256 (result below 4r inside, canonical out)"""
    cases = V.fr_mem_cases()
    want = [L.fr_mul_mem(a, b) for a, b in cases]
    check(run_field(zkp, "fr29", "fr_mul", cases), want, 8)
    check(run_field(zkp, "fr", "mul", cases), want, 8)             # the same operator through the saturated family's entry


@pytest.mark.parametrize("op", ["sub_tight", "sub_wide8"])
def test_fr29_borrow_free_subtraction(zkp, op):
    cases = V.fr29_sub_cases(op)
    check(run_field(zkp, "fr29", op, cases), [getattr(L, "fr29_" + op)(a, b) for a, b in cases], 9)


def test_fr29_normalise(zkp):
    cases = V.fr29_normalise_cases()
    check(run_field(zkp, "fr29", "normalise", [(a,) for a in cases]), [L.fr29_normalise(a) for a in cases], 9)


def test_fr29_pack_tight(zkp):
    cases = V.fr29_pack_cases()
    check(run_field(zkp, "fr29", "pack_tight", [(a,) for a in cases]), [L.fr29_pack_tight(a) for a in cases], 8)


@pytest.mark.parametrize("op", ["from_sat_shl5", "from_sat"])
def test_fr29_from_sat(zkp, op):
    cases = V.words_cases(8, 0x5A8, [R - 1, R, 2 * R - 1])
    check(run_field(zkp, "fr29", op, [(w,) for w in cases]), [getattr(L, "fr29_" + op)(w) for w in cases], 9)


def test_fr29_twiddle_from_mont(zkp):
    cases = V.fr_canonical_words()
    check(run_field(zkp, "fr29", "twiddle", [(w,) for w in cases]), [L.fr29_twiddle_from_mont(w) for w in cases], 9)


# ----------------------------------------------------------------------------------------------------------------- saturated Fq / Fr
@pytest.mark.parametrize("op", ["add", "sub", "neg", "dbl", "mul", "mont_mul"])
@pytest.mark.parametrize("field", ["fq", "fr"])
def test_saturated_field(zkp, field, op):
    """Fp<P> + - neg dbl, the product the kernels call (Fq: the out-of-line body) and the CIOS mont_mul, on canonical operands"""
    cases = V.fp_pairs(field)
    n = L.sat_mod(field)[1]
    check(run_field(zkp, field, op, cases), [L.sat_op(field, op, a, b) for a, b in cases], n)


# ----------------------------------------------------------------------------------------------------------------- Goldilocks
def _gl_words(v):
    return [v & 0xffffffff, v >> 32]


@pytest.mark.parametrize("op", ["add", "sub", "neg", "mul"])
def test_goldilocks(zkp, op):
    pairs = V.gl_pairs(any64=op == "mul")
    check(run_field(zkp, "gl", op, [(_gl_words(a), _gl_words(b)) for a, b in pairs]), [_gl_words(L.gl_op(op, a, b)) for a, b in pairs], 2)


def test_goldilocks_gl_reduce128(zkp):
    """raw (lo, hi) pairs: each of the three conditional corrections taken and not taken in every combination that can occur
    (the lo < c3 wrap included), results exactly 0 and exactly p - 1"""
    pairs = V.gl_reduce_pairs()
    check(run_field(zkp, "gl", "reduce128", [(_gl_words(a), _gl_words(b)) for a, b in pairs]), [_gl_words(L.gl_reduce128(a, b)[0]) for a, b in pairs], 2)


# ----------------------------------------------------------------------------------------------------------------- G1
COORDS = ("x", "y", "zz", "zzz")


def pack_points(pts, stride=None):
    """points (dicts of limb lists; an affine point has x, y only) -> int32 tensor, point-major (stride None) or plane-major"""
    import torch
    n = len(pts)
    w = np.zeros((n, 4, 16), dtype=np.uint32)
    for i, p in enumerate(pts):
        for j, c in enumerate(COORDS):
            if c in p:
                w[i, j, :14] = p[c]
    if stride is not None:      # chunk q (4 words) of point i at uint4 index q * stride + i
        planes = np.zeros((16, stride, 4), dtype=np.uint32)
        planes[:, :n, :] = w.reshape(n, 16, 4).transpose(1, 0, 2)
        w = planes
    return torch.from_numpy(np.ascontiguousarray(w).view(np.int32).reshape(-1)).cuda()


def unpack_points(t, n, stride=None):
    a = t.cpu().numpy().view(np.uint32)
    a = a.reshape(n, 4, 16) if stride is None else a.reshape(16, stride, 4)[:, :n, :].transpose(1, 0, 2).reshape(n, 4, 16)
    assert not a[:, :, 14:].any()
    return [{c: a[i, j, :14].tolist() for j, c in enumerate(COORDS)} for i in range(n)]


def run_g1(zkp, op, a_pts, b_pts, stride=None, in_place=False):
    import torch
    n = len(b_pts) if b_pts is not None else len(a_pts)
    d_a = pack_points(a_pts, stride)
    d_b = pack_points(b_pts if b_pts is not None else a_pts, stride)
    d_out = d_a.clone() if in_place else torch.full_like(d_a, -1)
    d_flag = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    zkp.selftest_g1_dev(op, None if in_place else d_a, d_b, n, stride or n, d_out, d_flag)
    torch.cuda.synchronize()
    return unpack_points(d_out, n, stride), d_flag.cpu().numpy().view(np.uint32).tolist()


def check_points(got, want, kinds):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, kinds[i])
        L.check_stored(g, f"case {i} ({kinds[i]})")          # the next operation on this output is in contract


@pytest.mark.parametrize("op", ["madd", "madd_chain"])
def test_g1_28_madd(zkp, op):
    """g1_28_madd<false/true>: stored X + 13p / Y + 5p, ZZ = 1 and not, q.y canonical and neg4, acc infinite, q == acc, q == -acc, the point
    (0, 2); uniform and mixed waves"""
    cases = V.g1_madd_cases()
    want = [L.g1_28_madd(acc, q) for _, acc, q in cases]
    got, flag = run_g1(zkp, op, [c[1] for c in cases], [c[2] for c in cases])
    check_points(got, want, [c[0] for c in cases])
    assert flag == [1 if L.is_inf(w) else 0 for w in want]


@pytest.mark.parametrize("op", ["mmadd", "mmadd_chain"])
def test_g1_28_mmadd(zkp, op):
    """g1_28_mmadd<false/true> with its return value; false (same x) leaves the accumulator alone"""
    cases = V.g1_mmadd_cases()
    want = [L.g1_28_mmadd(acc, q) for _, acc, q in cases]
    got, flag = run_g1(zkp, op, [c[1] for c in cases], [c[2] for c in cases])
    assert flag == [1 if ok else 0 for ok, _ in want] and 0 in flag and 1 in flag
    check_points(got, [w for _, w in want], [c[0] for c in cases])


def test_g1_28_add(zkp):
    cases = V.g1_add_cases()
    want = [L.g1_28_add(a, b) for _, a, b in cases]
    got, flag = run_g1(zkp, "add", [c[1] for c in cases], [c[2] for c in cases])
    check_points(got, want, [c[0] for c in cases])
    assert flag == [1 if L.is_inf(w) else 0 for w in want]


def test_g1_28_double(zkp):
    cases = V.g1_double_cases()
    got, _ = run_g1(zkp, "double", cases, None)
    check_points(got, [L.g1_28_double(a) for a in cases], ["double"] * len(cases))


def test_g1_28_double_affine(zkp):
    cases = V.g1_double_affine_cases()
    got, _ = run_g1(zkp, "double_affine", cases, None)
    check_points(got, [L.g1_28_double_affine(a) for a in cases], ["double_affine"] * len(cases))


@pytest.mark.parametrize("op", ["add_stream", "add_stream_chain", "add_inplace", "add_inplace_chain", "add_quad", "add_quad_inplace"])
def test_g1_28_add_in_memory(zkp, op):
    """g1_28_add_stream<false/true>, g1_28_add_stream_inplace (and with it g1_28_same_x_stream) and the four-lane g1_28_add_quad on the
    plane-major layout with a stride above the case count: the sums of g1_28_add (the quad form with its own Y3, the difference of two
    reduced products), exceptional quads next to ordinary ones in a wave
    (16 quads) and a wave of exceptional quads only; the in-place forms overwrite their first operand"""
    cases = V.g1_add_cases()
    want = [L.g1_28_add_quad(a, b) if "quad" in op else L.g1_28_add(a, b, stream=True) for _, a, b in cases]
    stride = len(cases) + 37
    got, _ = run_g1(zkp, op, [c[1] for c in cases], [c[2] for c in cases], stride=stride, in_place="inplace" in op)
    check_points(got, want, [c[0] for c in cases])


def test_g1_28_madd_chained_insertions(zkp):
    """The device's own output fed back as the next accumulator, 200 random insertions per lane (multiples of the generator with canonical
    and negated y, so equal and opposite points come up on the way), alternating the plain and the asm-chain form; the model walks the
    same insertions -- proving every intermediate state in contract -- and the limbs are compared at the end and on the way."""
    import torch
    rnd = random.Random(0xC4A1)
    lanes, steps = 64, 200
    model = [L.x28_infinity() for _ in range(lanes)]
    d_acc = pack_points(model)
    d_flag = torch.zeros(lanes, dtype=torch.int32, device="cuda")
    for s in range(steps):
        qs = []
        for lane in range(lanes):
            k = rnd.randrange(1, 24)
            qs.append(L.a28_from_point(V.kG(k) if rnd.random() < 0.97 else V.T3, 0, neg_form=rnd.random() < 0.5))
        zkp.selftest_g1_dev("madd_chain" if s & 1 else "madd", d_acc, pack_points(qs), lanes, lanes, d_acc, d_flag)
        model = [L.g1_28_madd(m, q) for m, q in zip(model, qs)]
        if s % 50 == 49:
            torch.cuda.synchronize()
            check_points(unpack_points(d_acc, lanes), model, [f"lane after {s + 1} insertions"] * lanes)
