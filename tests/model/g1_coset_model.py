"""Model of the coset openings (csrc/g1_ntt_plan.hpp from g1_coset_srs_map on, g1_ntt.hpp, g1_ntt_host.inc), with integers mod r
standing in for points as in g1_ntt_model.py: the n / l multi-point proofs of a polynomial, one per coset {w^(k + j r) : j < l} of the
domain, r = n / l.  The index arithmetic is the plan header's, written independently; tests/host/g1_coset_plan.cpp prints the
header's tables and tests/test_g1_coset_model_cpu.py compares them with these.  Two closed forms the GPU tests lean on are here too."""
from g1_ntt_model import R, bitrev, root, transform  # noqa: F401


def srs_slot_source(n, l, b, j):
    """the SRS index in slot j of slice b (a vector of 2r points), None for the identity"""
    r = n // l
    return (r - 2 - j) * l + b if j < r - 1 else None


def coeff_slot_source(n, l, length, b, t):
    """the coefficient index in slot t of row b of g (2r scalars), None for zero"""
    r = n // l
    src = (t + 1) * l + b
    return src if t < r - 1 and src < length else None


def slice_source(n, l, i):
    """the index of u that becomes h_i, None for the identity"""
    r = n // l
    return r - 2 + i if i < r - 1 else None


LAUNCH = 1 << 18


def mac(n, l, group_log):
    """(terms per lane, groups per output, lanes, lanes per launch) of the multiply-accumulate pass"""
    terms = min(l, 1 << group_log)
    groups = l // terms
    return terms, groups, groups * 2 * (n // l), LAUNCH // terms


def mac_element(n, l, group_log, lane, j):
    """term j of a lane: the element b * 2r + k of the transformed slices and rows"""
    m = 2 * (n // l)
    terms = mac(n, l, group_log)[0]
    q, k = divmod(lane, m)
    return (q * terms + j) * m + k


def fold_steps(n, l, group_log):
    """[(half, lanes, last)]: partial q += partial q + half for q < half, until one is left"""
    groups = mac(n, l, group_log)[1]
    out = []
    while groups > 1:
        groups //= 2
        out.append((groups, groups * 2 * (n // l), groups == 1))
    return out


def sizes(n, l, group_log):
    """bytes: (srs_hat, partial, work, slice, scalars, table, total)"""
    r = n // l
    _, groups, lanes, _ = mac(n, l, group_log)
    s = [512 * n, 256 * lanes if groups > 1 else 0, 512 * r, 256 * r, 64 * n, 256 * min(2 * n, LAUNCH)]
    return tuple(s + [sum(s)])


def open_cosets(srs, f, n, l, group_log=0):
    """-> (the r proofs, the n evaluations) of f (len(f) <= n coefficients), through the l slices in vectors of 2r"""
    r = n // l
    assert r >= 2 and 1 <= len(f) <= n and len(srs) >= n - l
    m = 2 * r
    s_hat, g_hat = [], []
    ninv = pow(m, R - 2, R)  # folded into the scalars
    for b in range(l):
        s_hat += transform([srs[k] if (k := srs_slot_source(n, l, b, j)) is not None else 0 for j in range(m)])
        g = transform([f[k] if (k := coeff_slot_source(n, l, len(f), b, t)) is not None else 0 for t in range(m)])
        g_hat += [x * ninv % R for x in g]
    terms, groups, lanes, _ = mac(n, l, group_log)
    partial = [sum(g_hat[e] * s_hat[e] for e in (mac_element(n, l, group_log, lane, j) for j in range(terms))) % R for lane in range(lanes)]
    for half, cnt, _ in fold_steps(n, l, group_log):
        for q in range(cnt):
            partial[q] = (partial[q] + partial[q + cnt]) % R
    u = transform(partial[:m], inverse=True, scale=False)
    h = [u[k] if (k := slice_source(n, l, i)) is not None else 0 for i in range(r)]
    return transform(h), transform(list(f) + [0] * (n - len(f)))


def quotient(f, n, l, k):
    """the coefficients of the quotient of f by X^l - x_k^l, by the division recurrence q_t = f_{t+l} + x_k^l q_{t+l}"""
    c = pow(root(n.bit_length() - 1), k * l, R)
    q = [0] * n
    for t in range(n - l - 1, -1, -1):
        q[t] = ((f[t + l] if t + l < len(f) else 0) + c * (q[t + l] if t + l < n else 0)) % R
    return q[:max(n - l, 1)]


def evaluate(f, x):
    acc = 0
    for c in reversed(f):
        acc = (acc * x + c) % R
    return acc


def interpolant(evals_of_coset, n, l, k):
    """the coefficients of the polynomial of degree < l with the values y_j at w^(k + j r): coefficient i is x_k^-i times coefficient
    i of the inverse transform of size l of y"""
    x_inv = pow(root(n.bit_length() - 1), -k, R)
    c = transform(list(evals_of_coset), inverse=True)
    return [c[i] * pow(x_inv, i, R) % R for i in range(l)]


def batch_inverse(xs):
    """1 / x for every x (none zero): one modular inversion and 3 multiplications each"""
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % R
    inv, out = pow(acc, R - 2, R), [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * xs[i] % R
    return out


def proofs_closed_form(f, evals, s, n, l):
    """q_k(s) for every coset from f(s) and the n evaluations, O(n):
    q_k(s) = f(s) / (s^l - c) - sum_{j<l} y_j a_j / (l c (s - a_j)),  a_j = w^(k + j r), c = x_k^l"""
    r = n // l
    w = root(n.bit_length() - 1)
    a = [1] * n
    for m in range(1, n):
        a[m] = a[m - 1] * w % R
    term = [y * x % R * d % R for y, x, d in zip(evals, a, batch_inverse([(s - x) % R for x in a]))]
    fs, sl, l_inv = evaluate(f, s), pow(s, l, R), pow(l, R - 2, R)
    c = [a[k * l] for k in range(r)]  # x_k^l
    den, c_inv = batch_inverse([(sl - x) % R for x in c]), batch_inverse(c)
    return [(fs * den[k] - sum(term[k::r]) % R * l_inv % R * c_inv[k]) % R for k in range(r)]
