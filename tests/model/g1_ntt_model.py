"""Model of the transform over G1 points and of the all-openings construction on top of it (csrc/g1_ntt_plan.hpp, g1_ntt.hpp,
g1_ntt_host.inc), with integers mod r standing in for points: the point [a]G is the integer a, [k]P is k * a, the SRS point S_k is
s^k.  The index arithmetic below is the same as the plan header's, written independently; tests/host/g1_ntt_plan.cpp prints the
header's tables and tests/test_g1_ntt_cpu.py compares them with these."""

R = 0x73eda753299d7d483339d80809a1d80553bda402fffe5bfeffffffff00000001
ROOT_2_32 = pow(7, (R - 1) >> 32, R)


def root(log_n):
    """the 2^log_n-th root of unity of zkp_ntt_fr (csrc/host_ff.hpp: fr_root_of_unity)"""
    return pow(ROOT_2_32, 1 << (32 - log_n), R)


def bitrev(i, log_n):
    return int(format(i, "0%db" % log_n)[::-1], 2) if log_n else 0


def butterfly(log_n, stage, i):
    """(lo, hi, exp) of lane i of a stage: twiddle-major numbering where a block is shorter than a wave, else block-major"""
    half, groups = 1 << stage, 1 << (log_n - 1 - stage)
    if half < 64 and groups >= 64:
        j, blk = divmod(i, groups)
    else:
        blk, j = divmod(i, half)
    lo = blk * 2 * half + j
    return lo, lo + half, j * groups


def transform(vec, inverse=False, scale=True):
    """the staged transform as the kernels run it: bit-reversed load, log_n stages in place, n^-1 folded into the last stage"""
    n = len(vec)
    log_n = n.bit_length() - 1
    assert 1 << log_n == n
    w = root(log_n)
    if inverse:
        w = pow(w, R - 2, R)
    v = [0] * n
    for i, x in enumerate(vec):
        v[bitrev(i, log_n)] = x % R
    ninv = pow(n, R - 2, R) if inverse and scale else 1
    for stage in range(log_n):
        c = ninv if stage == log_n - 1 else 1
        if c != 1:
            for i in range(n // 2):  # the left operands of the last stage are the first half
                v[i] = v[i] * c % R
        for i in range(n // 2):
            lo, hi, e = butterfly(log_n, stage, i)
            t = v[hi] * (c * pow(w, e, R) % R) % R
            v[lo], v[hi] = (v[lo] + t) % R, (v[lo] - t) % R
    return v


def transform_by_definition(vec, inverse=False):
    n = len(vec)
    log_n = n.bit_length() - 1
    w = root(log_n)
    if inverse:
        w = pow(w, R - 2, R)
    out = [sum(pow(w, i * j, R) * x for j, x in enumerate(vec)) % R for i in range(n)]
    if inverse:
        ninv = pow(n, R - 2, R)
        out = [x * ninv % R for x in out]
    return out


def lagrange(srs, n):
    """L_i(s) G for srs = [s^k]: the inverse transform of the first n points"""
    return transform(srs[:n], inverse=True)


def srs_slot_source(n, j):
    """the SRS index in slot j of the vector s of 2n points, None for the identity"""
    d = n - 1
    return d - 1 - j if j < d else None


def coeff_slot_source(n, length, t):
    """the coefficient index in slot t of the scalar vector g of 2n, None for zero"""
    return t + 1 if t + 1 < length and t + 1 < n else None


def slice_source(n, i):
    """the index of u that becomes h_i, None for the identity"""
    return n - 2 + i if i < n - 1 else None


def open_all(srs, f, n):
    """-> (proofs, evaluations) of f (len(f) <= n coefficients) at the n roots of unity, through the embedding in vectors of 2n"""
    assert 1 <= len(f) <= n and len(srs) >= n - 1
    s = [srs[k] if (k := srs_slot_source(n, j)) is not None else 0 for j in range(2 * n)]
    g = [f[k] if (k := coeff_slot_source(n, len(f), t)) is not None else 0 for t in range(2 * n)]
    s_hat, g_hat = transform(s), transform(g)
    ninv = pow(2 * n, R - 2, R)  # folded into the pointwise scalars
    u = transform([a * (b * ninv % R) % R for a, b in zip(s_hat, g_hat)], inverse=True, scale=False)
    h = [u[k] if (k := slice_source(n, i)) is not None else 0 for i in range(n)]
    return transform(h), transform(list(f) + [0] * (n - len(f)))
