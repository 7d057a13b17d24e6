"""Exact limb-level model of the device field and curve primitives (csrc/fq28.hpp, fr29.hpp, g1_28.hpp, ff.hpp).

Every function restates one device primitive on Python integers and returns the limbs the device must produce, bit for bit -- not
merely the same residue.  Every function also CHECKS the operand contract its header states in a comment and raises ContractError when a
vector breaks it: per-column sums of the product scanning below 2^64, the value-product caps (2520 p^2, 70 r^2), no limb of a subtrahend
above the limb of the K p constant it is taken from, no 32-bit wrap in a limb-wise sum.  Running a vector through the model therefore
yields its expected output and proves that it stays in contract at every intermediate step.

The constants are read from the headers (as tests/test_limb_constants.py does, which pins them), not retyped."""
import os
import re

import bigmodel as M

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "zkp-implementation_amd", "csrc")
P, R, GL = M.P, M.R, M.GL
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


class ContractError(AssertionError):
    """An operand outside the documented contract of a primitive."""


def need(cond, msg):
    if not cond:
        raise ContractError(msg)


def header_arrays(path, struct):
    src = open(os.path.join(CSRC, path)).read()
    body = src[src.index("struct " + struct):]
    body = body[:body.index("\n};")]
    out = {}
    for name, vals in re.findall(r"(\w+)\[\d+\]\s*=\s*\{([^}]*)\}", body):
        out[name] = [int(v.strip().rstrip("u"), 16) for v in vals.split(",")]
    for name, val in re.findall(r"uint32_t (\w+) = (0x[0-9a-f]+|\d+)u?;", body):
        out[name] = int(val, 0)
    return out


FQ = header_arrays("fq28.hpp", "Fq28C")
FR = header_arrays("fr29.hpp", "Fr29C")
SAT = {"fq": header_arrays("ff.hpp", "FqParams"), "fr": header_arrays("ff.hpp", "FrParams")}
NL28, NL29 = 14, 9
FQ_ONE, FQ_ZERO = list(FQ["ONE"]), [0] * NL28


def value(l, bits):
    return sum(int(x) << (bits * i) for i, x in enumerate(l))


def slice_limbs(x, bits, n):
    """x in n limbs of `bits` bits, the top limb taking the rest."""
    m = (1 << bits) - 1
    return [(x >> (bits * i)) & m for i in range(n - 1)] + [x >> (bits * (n - 1))]


def words32(x, n):
    return [(x >> (32 * i)) & M32 for i in range(n)]


def v28(l):
    return value(l, 28)


def v29(l):
    return value(l, 29)


# ---------------------------------------------------------------------------------------------------------------------------
# The unsaturated Montgomery product, product scanning (fq28_mul_inline / fq28_mul2 / Fr29 operator* and their asm forms)
# ---------------------------------------------------------------------------------------------------------------------------
def _mont_scan(pairs, bits, n, mod, mod_limbs, inv, what):
    """sum(a b for a, b in pairs) * 2^-(bits n) by the column walk of the device code: one 64-bit accumulator per column.  Returns the result
    limbs and checks that no column sum (limb products + reduction terms + carry) reaches 2^64, and that the walk equals the closed form
    m = -T p^-1 mod 2^(bits n), result = (T + m p) >> (bits n)."""
    mask = (1 << bits) - 1
    width = bits * n
    t = sum(value(a, bits) * value(b, bits) for a, b in pairs)
    m_all = (-t * pow(mod, -1, 1 << width)) % (1 << width)
    closed = (t + m_all * mod) >> width
    # sufficient bound first (the usual case); the exact walk only when it does not settle the question
    quick = sum(n * max(a) * max(b) for a, b in pairs) + n * mask * max(mod_limbs) + (1 << (64 - bits))
    if quick > M64:
        acc, m = 0, []
        for k in range(2 * n - 1):
            lo, hi = max(0, k - n + 1), min(k, n - 1)
            for a, b in pairs:
                acc += sum(a[i] * b[k - i] for i in range(lo, hi + 1))
            acc += sum(m[i] * mod_limbs[k - i] for i in range(lo, min(k - 1, n - 1) + 1)) if k else 0
            if k < n:
                need(acc <= M64, f"{what}: column {k} sum {acc:#x} does not fit 64 bits")
                m.append(((acc & M32) * inv) & mask)
                acc += m[k] * mod_limbs[0]
                need(acc <= M64, f"{what}: column {k} sum {acc:#x} does not fit 64 bits")
                assert acc & mask == 0
            else:
                need(acc <= M64, f"{what}: column {k} sum {acc:#x} does not fit 64 bits")
            acc >>= bits
        assert value(m, bits) == m_all
    need(closed >> (bits * (n - 1)) <= M32, f"{what}: top limb of the result does not fit 32 bits")
    return slice_limbs(closed, bits, n)


def _limbs_below(l, bound, what):
    need(all(0 <= x < bound for x in l), f"{what}: limb {max(l):#x} not below {bound:#x}")


def fq28_mul(a, b, what="fq28_mul"):
    """fq28_mul_inline == fq28_mul_chain (== each half of fq28_mul_chain2): limbs < 2^30, value(a) value(b) <= 2520 p^2; result tight."""
    _limbs_below(a, 1 << 30, what)
    _limbs_below(b, 1 << 30, what)
    need(v28(a) * v28(b) <= 2520 * P * P, f"{what}: value product above 2520 p^2")
    r = _mont_scan([(a, b)], 28, NL28, P, FQ["MOD"], FQ["INV"], what)
    assert v28(r) < 2 * P and all(x < (1 << 28) for x in r)
    return r


def fq28_sqr(a, what="fq28_sqr"):
    """sqr(a) = a * a; fq28_sqr_chain sums the same column values (each off-diagonal product once against 2 a)."""
    return fq28_mul(a, a, what)


def fq28_mul2(a, b, c, d, what="fq28_mul2"):
    """(a b + c d) / 2^392, one reduction: limb(a) limb(b) < 2^58, limb(c) limb(d) < 2^58, a b + c d <= 2520 p^2; result tight."""
    for x in (a, b, c, d):
        _limbs_below(x, 1 << 32, what)
    need(max(a) * max(b) < (1 << 58) and max(c) * max(d) < (1 << 58), f"{what}: a limb product reaches 2^58")
    need(v28(a) * v28(b) + v28(c) * v28(d) <= 2520 * P * P, f"{what}: value above 2520 p^2")
    r = _mont_scan([(a, b), (c, d)], 28, NL28, P, FQ["MOD"], FQ["INV"], what)
    assert v28(r) < 2 * P and all(x < (1 << 28) for x in r)
    return r


def _normalise(a, bits, what):
    mask, c, r = (1 << bits) - 1, 0, []
    for x in a[:-1]:
        t = x + c
        need(t <= M32, f"{what}: limb + carry wraps 32 bits")
        r.append(t & mask)
        c = t >> bits
    need(a[-1] + c <= M32, f"{what}: top limb + carry wraps 32 bits")
    return r + [a[-1] + c]


def fq28_normalise(a):
    return _normalise(a, 28, "fq28 normalise")


def _add(a, b, what):
    r = [x + y for x, y in zip(a, b)]
    need(max(r) <= M32, f"{what}: a limb sum wraps 32 bits")
    return r


def fq28_add(a, b):
    return _add(a, b, "fq28 add")


def _sub_k(a, b, table, what):
    """a + (K p) - b limb by limb: no limb of b above the limb of K p, no sum above 32 bits."""
    for i, (x, k) in enumerate(zip(b, table)):
        need(x <= k, f"{what}: limb {i} of the subtrahend ({x:#x}) above the constant's ({k:#x})")
    r = [x + (k - y) for x, y, k in zip(a, b, table)]
    need(max(r) <= M32, f"{what}: a limb wraps 32 bits")
    return r


def fq28_sub4(a, b):
    return _sub_k(a, b, FQ["KP4_29"], "sub4")


def fq28_sub8(a, b):
    return _sub_k(a, b, FQ["KP8_29"], "sub8")


def fq28_sub16(a, b):
    return _sub_k(a, b, FQ["KP16_29"], "sub16")


def fq28_sub8w(a, b):
    return _sub_k(a, b, FQ["KP8_30"], "sub8w")


def fq28_neg4(a):
    return _sub_k(FQ_ZERO, a, FQ["KP4_29"], "neg4")


def is_tight28(a):
    return all(x < (1 << 28) for x in a[:13]) and v28(a) < 2 * P


def fq28_tight_is_zero_mod_p(a):
    need(is_tight28(a), "tight_is_zero_mod_p: operand not tight")
    z = all(x == 0 for x in a) or list(a) == FQ["MOD"]
    assert z == (v28(a) % P == 0)     # for a tight value the two limb patterns are the only multiples of p
    return z


def fq28_from_sat(w12):
    """12 x 32-bit words -> 14 x 28-bit limbs: a re-slicing of any 384-bit integer (the callers pass canonical values)."""
    _limbs_below(w12, 1 << 32, "fq28_from_sat")
    return slice_limbs(value(w12, 32), 28, NL28)


# ---------------------------------------------------------------------------------------------------------------------------
# Fr29
# ---------------------------------------------------------------------------------------------------------------------------
def fr29_mul(a, b, weak=False, what="fr29_mul"):
    """Fr29 operator* == each half of fr29_mul2: limbs of a < 2^31, of b < 2^29, value(a) value(b) <= 70 r^2; result tight.
    weak: the memory-form product with non-canonical operands -- the value cap is exceeded on purpose, the result stays below 4r."""
    _limbs_below(a, 1 << 31, what)
    _limbs_below(b, 1 << 29, what)
    if not weak:
        need(v29(a) * v29(b) <= 70 * R * R, f"{what}: value product above 70 r^2")
    r = _mont_scan([(a, b)], 29, NL29, R, FR["MOD"], (1 << 29) - 1, what)
    need(v29(r) < (4 if weak else 2) * R, f"{what}: result not below {'4' if weak else '2'} r")
    assert all(x < (1 << 29) for x in r[:8])
    return r


def fr29_add(a, b):
    return _add(a, b, "fr29 add")


def fr29_sub_tight(a, b):
    return _sub_k(a, b, FR["KP4"], "sub_tight")


def fr29_sub_wide8(a, b):
    return _sub_k(a, b, FR["KP8"], "sub_wide8")


def fr29_normalise(a):
    return _normalise(a, 29, "fr29 normalise")


def fr29_from_sat(w8):
    _limbs_below(w8, 1 << 32, "fr29_from_sat")
    return slice_limbs(value(w8, 32), 29, NL29)


def fr29_from_sat_shl5(w8):
    _limbs_below(w8, 1 << 32, "fr29_from_sat_shl5")
    return slice_limbs(value(w8, 32) << 5, 29, NL29)


def fr29_to_canonical(x):
    """Any limbs with value < 2^261 -> (the 8 words of the canonical residue, whether the QEST quotient was one short)."""
    n = fr29_normalise(x)
    v = v29(n)
    need(v < (1 << 261), "fr29_to_canonical: value not below 2^261")
    q = ((n[8] >> 17) * FR["QEST"]) >> 16
    y = v - q * R
    assert 0 <= y < 2 * R, "QEST overshoots or leaves 2r or more"   # a property of the constant, pinned by test_limb_constants
    short = y >= R
    assert q + (1 if short else 0) == v // R
    return words32(y - R if short else y, 8), short


def fr_mul_mem(a8, b8):
    """Fr operator* on memory-form words (any two integers below 2^256): canonical a b 2^-256 mod r."""
    out, _ = fr29_to_canonical(fr29_mul(fr29_from_sat_shl5(a8), fr29_from_sat(b8), weak=True, what="Fr operator*"))
    assert value(out, 32) == value(a8, 32) * value(b8, 32) * pow(1 << 256, -1, R) % R
    return out


def fr29_pack_tight(c):
    _limbs_below(c, 1 << 29, "fr29_pack_tight")
    need(v29(c) < (1 << 256), "fr29_pack_tight: value not below 2^256")
    return words32(v29(c), 8)


def fr29_twiddle_from_mont(w8):
    need(value(w8, 32) < R, "fr29_twiddle_from_mont: operand not canonical")
    return fr29_from_sat(words32(value(w8, 32) * 32 % R, 8))


# ---------------------------------------------------------------------------------------------------------------------------
# Saturated Fp<P> (canonical in, canonical out) and Goldilocks
# ---------------------------------------------------------------------------------------------------------------------------
def sat_mod(field):
    return {"fq": (P, 12), "fr": (R, 8)}[field]


def sat_op(field, op, a, b=None):
    mod, n = sat_mod(field)
    x, y = value(a, 32), value(b, 32) if b is not None else 0
    need(x < mod and y < mod, f"{field} {op}: operand not canonical")
    if op == "add":
        r = (x + y) % mod
    elif op == "sub":
        r = (x - y) % mod
    elif op == "neg":
        r = (-x) % mod
    elif op == "dbl":
        r = 2 * x % mod
    elif op in ("mul", "mont_mul"):
        r = x * y * pow(1 << (32 * n), -1, mod) % mod
    else:
        raise KeyError(op)
    return words32(r, n)


def gl_op(op, a, b=0):
    if op == "mul":   # any 64-bit operands
        need(0 <= a <= M64 and 0 <= b <= M64, "gl mul: operand not a 64-bit word")
        t = a * b
        return gl_reduce128(t & M64, t >> 64)[0]
    need(a < GL and b < GL, f"gl {op}: operand not canonical")
    return {"add": (a + b) % GL, "sub": (a - b) % GL, "neg": (-a) % GL}[op]


def gl_reduce128(lo, hi):
    """The steps of ff.hpp's gl_reduce128 with explicit 64-bit wraps -> (result, (wrapped at lo - c3, wrapped at + c2 EPS, subtracted p))."""
    need(0 <= lo <= M64 and 0 <= hi <= M64, "gl_reduce128: operand not a 64-bit word")
    eps = (1 << 32) - 1
    c2, c3 = hi & M32, hi >> 32
    y = (lo - c3) & M64
    b1 = lo < c3
    if b1:
        assert y >= eps                      # "cannot wrap again"
        y -= eps
    z = y + c2 * eps
    b2 = z > M64
    if b2:
        z &= M64
        assert z <= (1 << 64) - (1 << 33)    # "no second wrap"
        z += eps
    b3 = z >= GL
    res = z - GL if b3 else z
    assert res == (lo + (hi << 64)) % GL
    return res, (b1, b2, b3)


# ---------------------------------------------------------------------------------------------------------------------------
# G1 in XYZZ on Fq28 (g1_28.hpp), line for line.  A point is a dict x, y, zz, zzz of limb lists; an affine point x, y.
# ---------------------------------------------------------------------------------------------------------------------------
def x28(x, y, zz, zzz):
    return {"x": list(x), "y": list(y), "zz": list(zz), "zzz": list(zzz)}


def x28_infinity():
    return x28(FQ_ZERO, FQ_ZERO, FQ_ZERO, FQ_ZERO)


def is_inf(p):
    return all(v == 0 for v in p["zz"])


def check_stored(p, what="stored point"):
    """The stored-point invariants at the head of g1_28.hpp."""
    need(all(v < (1 << 28) for v in p["x"][:13]) and v28(p["x"]) < 14 * P, f"{what}: X outside limbs < 2^28, value < 14p")
    need(all(v < (1 << 28) for v in p["y"][:13]) and v28(p["y"]) < 6 * P, f"{what}: Y outside limbs < 2^28, value < 6p")
    need(is_tight28(p["zz"]) and is_tight28(p["zzz"]), f"{what}: ZZ / ZZZ not tight")
    need(all(v <= M32 for k in ("x", "y", "zz", "zzz") for v in p[k]), f"{what}: a limb above 32 bits")


def xyzz_finish(r, pp, ppp, u1, s1):
    q = fq28_mul(u1, pp, "finish Q")
    rn = fq28_normalise(r)
    rr = fq28_sqr(rn, "finish RR")
    x3 = fq28_normalise(fq28_sub8w(fq28_sub4(rr, ppp), fq28_add(q, q)))
    t = fq28_sub16(q, x3)
    y3 = fq28_mul2(rn, t, fq28_sub8(FQ_ZERO, s1), ppp, "finish Y3")
    return x3, y3


def g1_28_double_affine(p):
    u = fq28_normalise(fq28_add(p["y"], p["y"]))
    v = fq28_sqr(u)
    w = fq28_mul(u, v)
    s = fq28_mul(p["x"], v)
    xx = fq28_sqr(p["x"])
    m = fq28_add(fq28_add(xx, xx), xx)
    ox = fq28_normalise(fq28_sub8w(fq28_sqr(m), fq28_add(s, s)))
    t = fq28_sub16(s, ox)
    oy = fq28_normalise(fq28_sub4(fq28_mul(m, t), fq28_mul(w, p["y"])))
    return x28(ox, oy, v, w)


def g1_28_double(p):
    u = fq28_add(p["y"], p["y"])
    v = fq28_sqr(u)
    w = fq28_mul(u, v)
    s = fq28_mul(p["x"], v)
    xx = fq28_sqr(p["x"])
    m = fq28_add(fq28_add(xx, xx), xx)
    ox = fq28_normalise(fq28_sub8w(fq28_sqr(m), fq28_add(s, s)))
    t = fq28_sub16(s, ox)
    oy = fq28_normalise(fq28_sub4(fq28_mul(m, t), fq28_mul(w, p["y"])))
    return x28(ox, oy, fq28_mul(v, p["zz"]), fq28_mul(w, p["zzz"]))


def g1_28_madd(acc, q):
    """-> the new accumulator (CHAIN or not: the same limbs)."""
    if is_inf(acc):
        return x28(q["x"], fq28_normalise(q["y"]), FQ_ONE, FQ_ONE)
    u2 = fq28_mul(q["x"], acc["zz"], "madd U2")
    s2 = fq28_mul(q["y"], acc["zzz"], "madd S2")
    p = fq28_sub16(u2, acc["x"])
    r = fq28_sub8(s2, acc["y"])
    pp = fq28_sqr(p, "madd PP")
    if fq28_tight_is_zero_mod_p(pp):
        if fq28_tight_is_zero_mod_p(fq28_sqr(r, "madd RR")):
            return g1_28_double_affine(q)
        return x28_infinity()
    ppp = fq28_mul(p, pp, "madd PPP")
    x3, y3 = xyzz_finish(r, pp, ppp, acc["x"], acc["y"])
    return x28(x3, y3, fq28_mul(acc["zz"], pp), fq28_mul(acc["zzz"], ppp))


def g1_28_mmadd(acc, q):
    """-> (return value, accumulator afterwards); ZZ / ZZZ of acc are not read (implied 1)."""
    p = fq28_sub16(q["x"], acc["x"])
    pp = fq28_sqr(p, "mmadd PP")
    if fq28_tight_is_zero_mod_p(pp):
        return False, x28(acc["x"], acc["y"], acc["zz"], acc["zzz"])
    r = fq28_sub8(q["y"], acc["y"])
    ppp = fq28_mul(p, pp, "mmadd PPP")
    x3, y3 = xyzz_finish(r, pp, ppp, acc["x"], acc["y"])
    return True, x28(x3, y3, pp, ppp)


def g1_28_add(a, b, stream=False):
    """g1_28_add, and with stream=True g1_28_add_stream(_inplace): the same products in another order (g1_28_add_quad: below).  The one
    difference in limbs: of two infinite operands g1_28_add keeps a, the streaming form copies b (both have ZZ = 0)."""
    if is_inf(a) and stream:
        return x28(b["x"], b["y"], b["zz"], b["zzz"])
    if is_inf(b):
        return x28(a["x"], a["y"], a["zz"], a["zzz"])
    if is_inf(a):
        return x28(b["x"], b["y"], b["zz"], b["zzz"])
    u1 = fq28_mul(a["x"], b["zz"], "add U1")
    u2 = fq28_mul(b["x"], a["zz"], "add U2")
    s1 = fq28_mul(a["y"], b["zzz"], "add S1")
    s2 = fq28_mul(b["y"], a["zzz"], "add S2")
    p = fq28_sub4(u2, u1)
    r = fq28_sub4(s2, s1)
    pp = fq28_sqr(p, "add PP")
    if fq28_tight_is_zero_mod_p(pp):
        if fq28_tight_is_zero_mod_p(fq28_sqr(r, "add RR")):
            return g1_28_double(a)
        return x28_infinity()
    ppp = fq28_mul(p, pp, "add PPP")
    x3, y3 = xyzz_finish(r, pp, ppp, u1, s1)
    return x28(x3, y3, fq28_mul(fq28_mul(a["zz"], b["zz"]), pp), fq28_mul(fq28_mul(a["zzz"], b["zzz"]), ppp))


def g1_28_add_quad(a, b):
    """g1_28_add_quad, the four lanes of a quad written out.  Its ordinary path is NOT xyzz_finish: R is squared and multiplied without
    being normalised (the same products), and Y3 = normalise(sub4(R (Q - X3), S1 PPP)) is the difference of two reduced products instead
    of one two-product reduction -- the same residue below 6p in other limbs.  Infinite operands and P = 0 go to lane 0's g1_28_add."""
    m1 = [fq28_mul(a["x"], b["zz"], "quad U1"), fq28_mul(b["x"], a["zz"], "quad U2"),
          fq28_mul(a["y"], b["zzz"], "quad S1"), fq28_mul(b["y"], a["zzz"], "quad S2")]
    p, r = fq28_sub4(m1[1], m1[0]), fq28_sub4(m1[3], m1[2])      # the odd lanes hold -P, -R the same way (unused)
    fq28_sub4(m1[0], m1[1]), fq28_sub4(m1[2], m1[3])
    pp, zz12 = fq28_sqr(p, "quad PP"), fq28_mul(a["zz"], b["zz"], "quad ZZ1 ZZ2")
    rr, zzz12 = fq28_sqr(r, "quad RR"), fq28_mul(a["zzz"], b["zzz"], "quad ZZZ1 ZZZ2")
    if is_inf(a) or is_inf(b) or fq28_tight_is_zero_mod_p(pp):
        return g1_28_add(a, b)
    ppp, zz3, q = fq28_mul(p, pp, "quad PPP"), fq28_mul(zz12, pp, "quad ZZ3"), fq28_mul(m1[0], pp, "quad Q")
    x3 = fq28_normalise(fq28_sub8w(fq28_sub4(rr, ppp), fq28_add(q, q)))
    t = fq28_sub16(q, x3)
    v, tt, zzz3 = fq28_mul(m1[2], ppp, "quad V"), fq28_mul(r, t, "quad T"), fq28_mul(zzz12, ppp, "quad ZZZ3")
    return x28(x3, fq28_normalise(fq28_sub4(tt, v)), zz3, zzz3)


# ---- ground truth side: limbs <-> the curve point they stand for ----------------------------------------------------------
R392 = (1 << 392) % P


def fq28_mont(x, k=0):
    """canonical limbs of the Montgomery form of x, raised by k p in the top limb (limbs 0..12 stay below 2^28)."""
    return slice_limbs(x * R392 % P + k * P, 28, NL28)


def affine_of(p):
    """the curve point (plain integers) an X28 stands for, None at infinity"""
    if is_inf(p):
        return None
    zz, zzz = v28(p["zz"]) % P, v28(p["zzz"]) % P
    assert zz and zzz and pow(zz, 3, P) == zzz * zzz * R392 % P   # zz^3 = zzz^2 for the values the Montgomery forms stand for
    return (v28(p["x"]) * pow(zz, -1, P) % P, v28(p["y"]) * pow(zzz, -1, P) % P)


def a28_from_point(pt, kx=0, neg_form=False):
    """affine base point in the internal form; neg_form: y as neg4 of the canonical form of -y (the same point, y in (3p, 4p])"""
    x, y = pt
    return {"x": fq28_mont(x, kx), "y": fq28_neg4(fq28_mont((-y) % P)) if neg_form else fq28_mont(y)}


def x28_from_point(pt, z=1, kx=0, ky=0):
    """the point with ZZ = z^2, ZZZ = z^3 and X, Y raised by kx p / ky p (the worst representatives the invariant admits: kx <= 13, ky <= 5)"""
    x, y = pt
    zz, zzz = z * z % P, z * z * z % P
    return x28(fq28_mont(x * zz % P, kx), fq28_mont(y * zzz % P, ky), fq28_mont(zz), fq28_mont(zzz))
