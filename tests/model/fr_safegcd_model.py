"""Big-int / fixed-width model of zkp-implementation_amd/csrc/fr_inv.hpp (Bernstein-Yang division steps for the scalar field, nine
signed 30-bit limbs, 25 rounds of 30 steps): the same arithmetic with Python integers, every 32- and 64-bit quantity range-checked,
so that the CPU tests can run the algorithm on edge cases and on inputs chosen to need many steps, and the GPU test has the words the
device must return.  The 30 steps on the low words are safegcd_model.divsteps_30, as the device code calls divsteps_30 of
fq28_inv.hpp.  Test infrastructure, not product code."""
from safegcd_model import _check64, _s32, divsteps_30

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
M30 = (1 << 30) - 1
NL = 9
ROUNDS = 25
MOD = [(R >> (30 * i)) & M30 for i in range(NL)]
MOD_INV30 = pow(R, -1, 1 << 30)
R3 = pow(2, 3 * 256, R)  # the correction of fr_inverse_gcd: (a R)^-1 R^3 R^-1 = a^-1 R, Montgomery radix 2^256


def to_limbs(x):
    """non-negative x < 2^270 -> 9 limbs of 30 bits"""
    return [(x >> (30 * i)) & M30 for i in range(NL)]


def value(l):
    return sum(v << (30 * i) for i, v in enumerate(l))


def update_fg(f, g, u, v, q, r):
    cf = _check64(u * f[0] + v * g[0])
    cg = _check64(q * f[0] + r * g[0])
    assert cf & M30 == 0 and cg & M30 == 0
    cf >>= 30
    cg >>= 30
    for i in range(1, NL):
        cf = _check64(cf + u * f[i] + v * g[i])
        cg = _check64(cg + q * f[i] + r * g[i])
        f[i - 1], g[i - 1] = cf & M30, cg & M30
        cf >>= 30
        cg >>= 30
    f[NL - 1], g[NL - 1] = _s32(cf), _s32(cg)
    assert f[NL - 1] == cf and g[NL - 1] == cg, "top limb does not fit 32 bits"


def update_de(d, e, u, v, q, r):
    sd, se = (-1 if d[NL - 1] < 0 else 0), (-1 if e[NL - 1] < 0 else 0)
    md, me = (u & sd) + (v & se), (q & sd) + (r & se)
    cd = _check64(u * d[0] + v * e[0])
    ce = _check64(q * d[0] + r * e[0])
    md -= (MOD_INV30 * (cd & 0xffffffff) + md) & M30
    me -= (MOD_INV30 * (ce & 0xffffffff) + me) & M30
    assert -(1 << 31) <= md < (1 << 31) and -(1 << 31) <= me < (1 << 31)
    cd = _check64(cd + MOD[0] * md)
    ce = _check64(ce + MOD[0] * me)
    assert cd & M30 == 0 and ce & M30 == 0
    cd >>= 30
    ce >>= 30
    for i in range(1, NL):
        cd = _check64(cd + u * d[i] + v * e[i] + MOD[i] * md)
        ce = _check64(ce + q * d[i] + r * e[i] + MOD[i] * me)
        d[i - 1], e[i - 1] = cd & M30, ce & M30
        cd >>= 30
        ce >>= 30
    d[NL - 1], e[NL - 1] = _s32(cd), _s32(ce)
    assert d[NL - 1] == cd and e[NL - 1] == ce
    assert -2 * R < value(d) < R and -2 * R < value(e) < R, "d, e leave (-2r, r)"


def normalize(x, negate):
    v = value(x)
    if v < 0:
        v += R
    if negate:
        v = -v
    if v < 0:
        v += R
    assert 0 <= v < R
    return v


def modinv(x, early_exit=True):
    """-> (x^-1 mod r, rounds used); x < 2r (0 and r -> 0).  With early_exit the loop stops like a wave whose lanes have all reached
    g = 0."""
    assert 0 <= x < 2 * R
    gl = to_limbs(x)                      # fr_s30_reduce_once: limb-wise g - r with borrows, kept when non-negative
    t, c = [0] * NL, 0
    for i in range(NL):
        t[i] = gl[i] - MOD[i] + c
        if i < NL - 1:
            c = t[i] >> 30
            t[i] &= M30
    assert -(1 << 31) <= t[NL - 1] < (1 << 31)
    if t[NL - 1] >= 0:
        gl = t
    assert value(gl) == x % R
    f, g = list(MOD), gl
    d, e = [0] * NL, [1] + [0] * (NL - 1)
    eta, used = -1, ROUNDS
    for it in range(ROUNDS):
        eta, u, v, q, r = divsteps_30(eta, f[0], g[0])
        assert abs(u) + abs(v) <= 1 << 30 and abs(q) + abs(r) <= 1 << 30
        update_de(d, e, u, v, q, r)
        update_fg(f, g, u, v, q, r)
        if value(g) == 0 and used == ROUNDS:
            used = it + 1
            if early_exit:
                break
    assert value(g) == 0, "g != 0 after the fixed number of rounds"
    fv = value(f)
    assert abs(fv) in (1, R), "f must end at +-gcd"
    return normalize(d, fv < 0), used


def inverse_words(x):
    """What fr_inverse_gcd returns for the memory-form value x < 2r (a Montgomery residue a R): the canonical a^-1 R as an integer"""
    return modinv(x)[0] * R3 * pow(2, -256, R) % R


def edge_inputs():
    """The inputs both tests walk: 0, 1, r - 1, the non-canonical r, r + 5, 2r - 1, 2^k +- 1, r >> k, and inputs chosen to need many
    rounds (Fibonacci-like ratios, values near r / golden ratio)"""
    xs = [0, 1, 2, 3, R - 1, R - 2, (R + 1) // 2, (R - 1) // 2, 1 << 254, (1 << 255) - 1, R, R + 1, R + 5, 2 * R - 1, 2 * R - 2]
    a, b = 1, 1
    while b < R:
        a, b = b, a + b
        xs.append(b % R)
    for k in range(1, 255, 5):
        xs += [(1 << k) - 1, (1 << k) + 1, R >> k, (R >> k) | 1, R - (1 << k)]
    phi = (R * 0x9E3779B97F4A7C15) >> 64  # r / golden ratio
    xs += [phi, phi + 1, R - phi]
    return xs
