"""Big-int model of the FAST pairing algorithms of csrc/pairing_tower.hpp and csrc/pairing.hpp (TEST INFRASTRUCTURE ONLY): prepared G2
lines, the sparse line product, Frobenius maps, Granger-Scott cyclotomic squaring, the Fq12 inverse through the norms, and the
x-chain final exponentiation E(f) = f^(3 (p^12 - 1) / r).  tests/test_pairing_fast_model_cpu.py pins every piece to the plain model
(pairing_model.py); the C++ tower over HFq and the device kernels are then compared with THIS model word for word.

Same tower and coefficient order as pairing_model.py: Fq2 = Fq[u]/(u^2+1), Fq6 = Fq2[v]/(v^3-(1+u)), Fq12 = Fq6[w]/(w^2-v).
"""
import bigmodel as M
import pairing_model as PM

P, R = M.P, M.R
X_ABS = PM.X_ABS
X = -X_ABS

# the hard part as a polynomial in p: lambda_0 + lambda_1 p + lambda_2 p^2 + lambda_3 p^3 = 3 (p^4 - p^2 + 1) / r
LAMBDA3 = (X - 1) ** 2
LAMBDA2 = X * LAMBDA3
LAMBDA1 = X * LAMBDA2 - LAMBDA3
LAMBDA0 = X * LAMBDA1 + 3

# the Miller loop as a list of steps, most significant bit of |x| (below the leading one) first: True = doubling, False = addition
STEPS = []
for _bit in bin(X_ABS)[3:]:
    STEPS.append(True)
    if _bit == "1":
        STEPS.append(False)
N_STEPS = len(STEPS)  # 63 doublings + 5 additions = 68
DBL_MASK = sum(1 << i for i, d in enumerate(STEPS) if d)  # bit i set: step i squares f first


# ---- Fq2 / Fq6 helpers the plain model does not have
def f2_sqr(a): return PM.f2_mul(a, a)
def f2_conj(a): return (a[0], (-a[1]) % P)
def f2_dbl(a): return PM.f2_add(a, a)


def f2_pow(a, e):
    r = PM.F2_ONE
    for bit in bin(e)[2:]:
        r = PM.f2_mul(r, r)
        if bit == "1":
            r = PM.f2_mul(r, a)
    return r


def f6_neg(a): return tuple(PM.f2_neg(x) for x in a)
def f6_scale2(a, k): return tuple(PM.f2_mul(x, k) for x in a)


def f6_inv(a):
    c0, c1, c2 = a
    xi = PM.f2_mul_xi
    t0 = PM.f2_sub(f2_sqr(c0), xi(PM.f2_mul(c1, c2)))
    t1 = PM.f2_sub(xi(f2_sqr(c2)), PM.f2_mul(c0, c1))
    t2 = PM.f2_sub(f2_sqr(c1), PM.f2_mul(c0, c2))
    n = PM.f2_add(PM.f2_mul(c0, t0), xi(PM.f2_add(PM.f2_mul(c2, t1), PM.f2_mul(c1, t2))))
    ni = PM.f2_inv(n)
    return (PM.f2_mul(t0, ni), PM.f2_mul(t1, ni), PM.f2_mul(t2, ni))


def f12_inv(a):
    """(c0 - c1 w) / (c0^2 - v c1^2): one Fq6 inverse, which is one Fq2 inverse, which is one Fq inversion.  0 -> 0."""
    if a == (PM.F6_ZERO, PM.F6_ZERO):
        return a
    c0, c1 = a
    n = PM.f6_sub(PM.f6_mul(c0, c0), PM.f6_mul_v(PM.f6_mul(c1, c1)))
    ni = f6_inv(n)
    return (PM.f6_mul(c0, ni), f6_neg(PM.f6_mul(c1, ni)))


def f12_sqr(a): return PM.f12_mul(a, a)


# ---- the sparse product: f * ((A, B, 0), (0, C, 0)), C in Fq
def line_as_f12(a, b, c):
    return ((a, b, PM.F2_ZERO), (PM.F2_ZERO, (c % P, 0), PM.F2_ZERO))


def f12_mul_line(f, a, b, c):
    f0, f1 = f
    xi = PM.f2_mul_xi

    def mul_ab(g):      # (g0, g1, g2) * (A, B, 0)
        return (PM.f2_add(PM.f2_mul(g[0], a), xi(PM.f2_mul(g[2], b))), PM.f2_add(PM.f2_mul(g[0], b), PM.f2_mul(g[1], a)),
                PM.f2_add(PM.f2_mul(g[1], b), PM.f2_mul(g[2], a)))

    def mul_c(g):       # (g0, g1, g2) * (0, C, 0)
        return (xi(PM.f2_scale(g[2], c)), PM.f2_scale(g[0], c), PM.f2_scale(g[1], c))
    return (PM.f6_add(mul_ab(f0), PM.f6_mul_v(mul_c(f1))), PM.f6_add(mul_c(f0), mul_ab(f1)))


# ---- Frobenius: a_(j,i) v^i w^j = a_(j,i) w^(2i+j)  ->  conj^k(a_(j,i)) * GAMMA[k][2i+j] * w^(2i+j),  GAMMA[k][m] = xi^(m (p^k-1)/6)
XI = (1, 1)
GAMMA = {k: [f2_pow(XI, m * (P ** k - 1) // 6) for m in range(6)] for k in (1, 2, 3)}


def f12_frobenius(a, k):
    out = []
    for j in (0, 1):
        half = []
        for i in range(3):
            c = a[j][i]
            if k & 1:
                c = f2_conj(c)
            half.append(PM.f2_mul(c, GAMMA[k][2 * i + j]))
        out.append(tuple(half))
    return tuple(out)


# ---- Granger-Scott squaring in the cyclotomic subgroup (valid after the easy part of the final exponentiation)
def f12_cyclotomic_sqr(a):
    xi = PM.f2_mul_xi
    r0, r4, r3 = a[0]
    r2, r1, r5 = a[1]

    def sq2(x, y):  # (x + y s)^2 with s^2 = xi: (x^2 + xi y^2, 2 x y)
        t = PM.f2_mul(x, y)
        return (PM.f2_sub(PM.f2_sub(PM.f2_mul(PM.f2_add(x, y), PM.f2_add(xi(y), x)), t), xi(t)), f2_dbl(t))
    t0, t1 = sq2(r0, r1)
    t2, t3 = sq2(r2, r3)
    t4, t5 = sq2(r4, r5)

    def three_minus_two(t, z): return PM.f2_add(f2_dbl(PM.f2_sub(t, z)), t)   # 3 t - 2 z
    def three_plus_two(t, z): return PM.f2_add(f2_dbl(PM.f2_add(t, z)), t)    # 3 t + 2 z
    z0 = three_minus_two(t0, r0)
    z1 = three_plus_two(t1, r1)
    z2 = three_plus_two(xi(t5), r2)
    z3 = three_minus_two(t4, r3)
    z4 = three_minus_two(t2, r4)
    z5 = three_plus_two(t3, r5)
    return ((z0, z4, z3), (z2, z1, z5))


def cyclotomic_exp_x_abs(a):
    """a^|x| by cyclotomic squarings, most significant bit first"""
    r = a
    for bit in bin(X_ABS)[3:]:
        r = f12_cyclotomic_sqr(r)
        if bit == "1":
            r = PM.f12_mul(r, a)
    return r


def exp_x(a):
    """a^x for a in the cyclotomic subgroup (x < 0: the inverse there is the conjugate)"""
    return PM.f12_conj(cyclotomic_exp_x_abs(a))


def easy_part(f):
    """f^((p^6 - 1)(p^2 + 1))"""
    t = PM.f12_mul(PM.f12_conj(f), f12_inv(f))
    return PM.f12_mul(f12_frobenius(t, 2), t)


def final_exp(f):
    """E(f) = f^(3 (p^12 - 1) / r): the CUBE of pairing_model's final exponentiation.  gcd(3, r) = 1, so E(f) = 1 iff that is 1."""
    m = easy_part(f)
    b = m
    for _ in range(2):                                   # m^((x-1)^2) = m^lambda_3
        b = PM.f12_mul(exp_x(b), PM.f12_conj(b))
    c = exp_x(b)                                         # m^lambda_2
    d = PM.f12_mul(exp_x(c), PM.f12_conj(b))             # m^lambda_1
    e = PM.f12_mul(exp_x(d), PM.f12_mul(f12_cyclotomic_sqr(m), m))  # m^lambda_0
    return PM.f12_mul(PM.f12_mul(e, f12_frobenius(d, 1)), PM.f12_mul(f12_frobenius(c, 2), f12_frobenius(b, 3)))


# ---- prepared G2: the walk done once, per step the pair (lambda, lambda x_T - y_T)
def prepare_g2(q):
    """q: G2 affine or None -> list of N_STEPS (lambda, lambda x_T - y_T), or None for the identity"""
    if q is None:
        return None
    t, out = q, []
    for dbl in STEPS:
        if dbl:
            lam = PM.f2_mul(PM.f2_scale(PM.f2_mul(t[0], t[0]), 3), PM.f2_inv(PM.f2_scale(t[1], 2)))
            out.append((lam, PM.f2_sub(PM.f2_mul(lam, t[0]), t[1])))
            t = PM.g2_double(t)
        else:
            lam = PM.f2_mul(PM.f2_sub(q[1], t[1]), PM.f2_inv(PM.f2_sub(q[0], t[0])))
            out.append((lam, PM.f2_sub(PM.f2_mul(lam, t[0]), t[1])))
            t = PM.g2_add(t, q)
    return out


def miller_product(ps, prepared):
    """prod_j miller_loop(P_j, Q_j) with the squarings shared; ps[j]: G1 affine or None, prepared[j]: prepare_g2(Q_j)"""
    f = PM.F12_ONE
    for s, dbl in enumerate(STEPS):
        if dbl:
            f = f12_sqr(f)
        for p, lines in zip(ps, prepared):
            if p is None or lines is None:
                continue
            lam, a = lines[s]
            f = f12_mul_line(f, a, PM.f2_scale(lam, (-p[0]) % P), p[1])
    return PM.f12_conj(f)


# ---- memory form: 12 Fq Montgomery residues (radix 2^384) as 72 little-endian u64 words, arkworks coefficient order
def f12_to_words(a):
    out = []
    for c in PM.f12_flat(a):
        out += M.to_limbs(M.fq_to_mont(c), 6)
    return out


def f12_from_words(w):
    c = [M.fq_from_mont(M.from_limbs(w[6 * i:6 * i + 6])) for i in range(12)]
    return (((c[0], c[1]), (c[2], c[3]), (c[4], c[5])), ((c[6], c[7]), (c[8], c[9]), (c[10], c[11])))


def frobenius_table_words():
    """The 15 constants of csrc/pairing_tower.hpp in its order (k = 1, 2, 3; m = 1 .. 5), each an Fq2 as 12 Montgomery u64 words"""
    out = []
    for k in (1, 2, 3):
        for m in range(1, 6):
            g = GAMMA[k][m]
            out.append(M.to_limbs(M.fq_to_mont(g[0]), 6) + M.to_limbs(M.fq_to_mont(g[1]), 6))
    return out
