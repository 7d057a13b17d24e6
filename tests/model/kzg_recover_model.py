"""Big-integer mirror of the cell recovery (csrc/kzg_recover_plan.hpp, kzg_recover.hpp, kzg_recover_host.inc): the product tree of the
vanishing polynomial with its padding, leaves and levels as the plan states them, and the pipeline around it.  Written
independently of the header; tests/test_kzg_recover_model_cpu.py checks it against Lagrange interpolation, and
tests/host/kzg_recover_plan.cpp runs the header's own step list over a small field."""
from g1_ntt_model import R, root

G = 7  # the coset shift: g^n != 1 for every n <= 2^32
PAD = None  # the padding root 0, a factor Y


def inv(a):
    return pow(a, R - 2, R)


def ntt(vec, inverse=False, shift=None):
    """the transform of zkp_ntt_fr: forward, vec are coefficients and the result their values at shift w^i; inverse undoes it"""
    n = len(vec)
    log_n = n.bit_length() - 1
    assert 1 << log_n == n
    w = root(log_n)
    if inverse:
        w = inv(w)
    v = [x % R for x in vec]
    if shift is not None and not inverse:
        v = [x * pow(shift, i, R) % R for i, x in enumerate(v)]
    # recursive radix 2, decimation in time
    def rec(a, wn):
        if len(a) == 1:
            return a
        e, o = rec(a[0::2], wn * wn % R), rec(a[1::2], wn * wn % R)
        out, t = [0] * len(a), 1
        for k in range(len(a) // 2):
            x = t * o[k] % R
            out[k], out[k + len(a) // 2] = (e[k] + x) % R, (e[k] - x) % R
            t = t * wn % R
        return out
    v = rec(v, w)
    if inverse:
        ninv = inv(n)
        v = [x * ninv % R for x in v]
        if shift is not None:
            si = inv(shift)
            v = [x * pow(si, i, R) % R for i, x in enumerate(v)]
    return v


def plan(log_n, log_l, leaf_log, m):
    """(padded root count, pad, factors per leaf, leaves, [d of every level])"""
    if m == 0:
        return 0, 0, 0, 0, []
    roots = 1
    while roots < m:
        roots *= 2
    per = min(1 << leaf_log, roots)
    levels, d = [], per
    while d < roots:
        levels.append(d)
        d *= 2
    return roots, roots - m, per, roots // per, levels


def leaf(rootvals):
    """the low coefficients of the monic product of (Y - a), a factor at a time as the workgroup does it; None is the root 0"""
    c = []
    for s, a in enumerate(rootvals):
        a = 0 if a is PAD else a
        c = [((c[t - 1] if t else 0) - a * (1 if t == s else c[t])) % R for t in range(s + 1)]
    return c


def join(a, b):
    """the d low coefficients of two monic nodes -> the 2d low coefficients of their product, through transforms of 2d and
    out_k = a_k b_k + (-1)^k (a_k + b_k)"""
    d = len(a)
    fa, fb = ntt(a + [0] * d), ntt(b + [0] * d)
    out = [(x * y + (-1 if k & 1 else 1) * (x + y)) % R for k, (x, y) in enumerate(zip(fa, fb))]
    return ntt(out, inverse=True)


def vanishing(log_n, log_l, leaf_log, missing):
    """the coefficients of Zs(Y) = prod_{k in missing} (Y - rho^k), lowest first, m + 1 of them, through the plan's tree"""
    m = len(missing)
    if m == 0:
        return [1]
    rho = root(log_n - log_l)
    roots, pad, per, leaves, levels = plan(log_n, log_l, leaf_log, m)
    entries = [pow(rho, k, R) for k in missing] + [PAD] * pad
    nodes = [leaf(entries[q * per:(q + 1) * per]) for q in range(leaves)]
    for d in levels:
        assert all(len(x) == d for x in nodes)
        nodes = [join(nodes[2 * p], nodes[2 * p + 1]) for p in range(len(nodes) // 2)]
    assert len(nodes) == 1 and len(nodes[0]) == roots and not any(nodes[0][:pad])
    return nodes[0][pad:] + [1]


def recover(evals, present, length, log_n, log_l, leaf_log=5):
    """-> (the `length` low coefficients, consistent), from the values of the present cosets alone"""
    n, r = 1 << log_n, 1 << (log_n - log_l)
    l = n // r
    missing = [k for k in range(r) if not present[k]]
    m = len(missing)
    assert length >= 1 and (r - m) * l >= length
    if m == 0:
        c = ntt(evals, inverse=True)
        return c[:length], not any(c[length:])
    zs = vanishing(log_n, log_l, leaf_log, missing)
    zs = zs + [0] * (r - len(zs))
    z_dom = ntt(zs)
    z_shift = ntt(zs, shift=pow(G, l, R))
    ez = [evals[i] * z_dom[i % r] % R if present[i % r] else 0 for i in range(n)]
    p = ntt(ez, inverse=True)
    q = ntt(p, shift=G)
    q = [x * inv(z_shift[i % r]) % R for i, x in enumerate(q)]
    c = ntt(q, inverse=True, shift=G)
    return c[:length], not any(c[length:])


def poly_mul_linear(c, a):
    """c(Y) (Y - a)"""
    out = [0] * (len(c) + 1)
    for i, x in enumerate(c):
        out[i + 1] = (out[i + 1] + x) % R
        out[i] = (out[i] - a * x) % R
    return out


def lagrange(points, values):
    """coefficients of the interpolant through (points[i], values[i]), O(k^2)"""
    k = len(points)
    full = [1]
    for x in points:
        full = poly_mul_linear(full, x)
    out = [0] * k
    for x, y in zip(points, values):
        # full / (Y - x) by synthetic division
        q, carry = [0] * k, 0
        for i in range(k, 0, -1):
            carry = (full[i] + carry * x) % R
            q[i - 1] = carry
        denom = 0
        for cq in reversed(q):
            denom = (denom * x + cq) % R
        s = y * inv(denom) % R
        for i in range(k):
            out[i] = (out[i] + s * q[i]) % R
    return out


def workspace_bytes(log_n, log_l):
    """(device bytes, pinned bytes) of a recoverer: n + 5 r field elements, the root list of r words and the mask of r bytes"""
    n, r = 1 << log_n, 1 << (log_n - log_l)
    return (32 * (n + 5 * r) + 5 * r + 31) // 32 * 32, 5 * r
