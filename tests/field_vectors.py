"""Edge vectors for the limb-level tests of the device primitives (tests/test_limb_model_cpu.py, tests/test_gpu_field_selftest.py).

Deterministic and seeded.  Every generator builds operands AT the documented contract edges on purpose (values k p +- 1, products at the
2520 p^2 / 70 r^2 caps, limbs raised to just below the allowed bound, subtrahends equal to the K p constant) and asserts a minimum count
and the presence of the special outcomes it is there for; nothing is filtered away for being out of contract -- the model
(tests/model/limb_model.py) raises on such a vector."""
import math
import random

import bigmodel as M
import limb_model as L

P, R, GL = L.P, L.R, L.GL
CAP_Q, CAP_R = 2520 * P * P, 70 * R * R


# ---- limb shapes ---------------------------------------------------------------------------------------------------------
def canon(v, bits=28, n=14):
    return L.slice_limbs(v, bits, n)


def loose(v, bound, bits=28, n=14):
    """the same value with the lower limbs raised to just below `bound` by borrowing from the limb above, wherever that limb can lend"""
    l = L.slice_limbs(v, bits, n)
    for i in range(n - 2, -1, -1):
        t = min(l[i + 1], (bound - 1 - l[i]) >> bits)
        l[i] += t << bits
        l[i + 1] -= t
    assert L.value(l, bits) == v and max(l[:-1]) < bound
    return l


def single(i, x, n=14):
    l = [0] * n
    l[i] = x
    return l


def fq_values(rnd, nrand=12):
    v = [0, 1, P - 1, P, P + 1, 2 * P - 1, L.v28(L.FQ["ONE"])]
    for k in (2, 4, 6, 8, 14, 16, 18, 50):
        v += [k * P - 1, k * P, k * P + 1]
    for k in range(28, 392, 28):
        v += [(1 << k) - 1, (1 << k) + 1]
    return v + [rnd.randrange(P) for _ in range(nrand)]


def fr_values(rnd, nrand=12):
    v = [0, 1, R - 1, R, R + 1, 2 * R - 1, L.v29(L.FR["ONE"])]
    for k in (2, 4, 8, 12, 34, 35, 70):
        v += [k * R - 1, k * R, k * R + 1]
    for k in range(29, 261, 29):
        v += [(1 << k) - 1, (1 << k) + 1]
    return v + [rnd.randrange(R) for _ in range(nrand)]


def _partners(rnd, va, cap, vmax):
    top = min(cap // va, vmax) if va else vmax
    return [top, max(top - 1, 0), rnd.randrange(top + 1), 0]


# ---- Fq28 ----------------------------------------------------------------------------------------------------------------
def fq28_mul_cases(seed=0xF928):
    """(a, b): limbs below 2^30, value products at and just under 2520 p^2"""
    rnd = random.Random(seed)
    B, vmax = 1 << 30, 2520 * P
    shaped = []
    for va in fq_values(rnd):
        shaped += [canon(va), loose(va, B), loose(va, 1 << 29)]
    shaped += [single(i, B - 1) for i in range(14)] + [[B - 1] * 14, [B - 1] * 13 + [0], [(1 << 28) - 1] * 14]
    cases = []
    for a in shaped:
        for vb in _partners(rnd, L.v28(a), CAP_Q, vmax):
            for b in (canon(vb), loose(vb, B)):
                cases.append((a, b) if rnd.random() < 0.5 else (b, a))
    for ka, kb in ((1, 2520), (14, 180), (18, 140), (50, 50)):
        for da, db in ((0, 0), (-1, 0), (0, -1), (-1, -1)):
            cases += [(canon(ka * P + da), loose(kb * P + db, B)), (loose(ka * P + da, B), loose(kb * P + db, B))]
    # operands that are multiples of p and not zero: the exact result is p; with a zero operand it is 0
    for k in (1, 2, 14, 50):
        cases += [(loose(k * P, B), canon(0)), (canon(k * P), loose(P, B)), (canon(k * P), canon(3))]
    res = [L.v28(L.fq28_mul(a, b)) for a, b in cases]
    assert len(cases) >= 1000 and res.count(0) >= 4 and res.count(P) >= 12
    assert sum(1 for a, b in cases if L.v28(a) * L.v28(b) == CAP_Q) >= 8
    return cases


def fq28_sqr_cases(seed=0x5928):
    rnd = random.Random(seed)
    B = 1 << 30
    vals = [v for v in fq_values(rnd, 40) if v * v <= CAP_Q]
    root = math.isqrt(CAP_Q)
    vals += [root, root - 1, 50 * P, 50 * P + 1]
    cases = []
    for v in vals:
        cases += [canon(v), loose(v, B), loose(v, 1 << 29)]
    cases += [single(i, B - 1) for i in range(13)] + [single(13, root >> 364)]
    low = [B - 1] * 13
    cases += [low + [0], low + [(root - L.v28(low + [0])) >> 364]]      # every lower limb at the bound, the top limb filling up to the cap
    assert len(cases) >= 250 and all(L.v28(a) ** 2 <= CAP_Q for a in cases)
    return cases


def fq28_mul2_cases(seed=0x2928):
    """(a, b, c, d): limb(a) limb(b) < 2^58 and limb(c) limb(d) < 2^58, a b + c d at and under 2520 p^2"""
    rnd = random.Random(seed)
    B28, B29, B30 = 1 << 28, 1 << 29, 1 << 30
    cases = []
    # the worst case of xyzz_finish: R t + (8p - S1) PPP with R, t < 18p and 8p, 2p; and the cap itself, 50 * 50 + 20 * 1
    for d in (0, 1):
        cases.append((canon(18 * P - d), loose(18 * P - 1, B30), loose(8 * P - d, B30), canon(2 * P - 1)))
        cases.append((canon(50 * P - d), loose(50 * P, B30), loose(20 * P, B30), canon(P)))
        cases.append((loose(50 * P, B30), canon(50 * P - d), canon(P), loose(20 * P, B30)))
        cases.append((loose(50 * P, B29), loose(50 * P - d, B29), loose(2 * P, B29), loose(10 * P, B29)))
    cases.append((canon(0), loose(P, B30), loose(3 * P, B30), canon(0)))            # exactly 0
    cases.append(([B28 - 1] * 14, [B30 - 1] * 13 + [0], [B30 - 1] * 13 + [0], [B28 - 1] * 13 + [0]))
    vals = fq_values(rnd)
    for va in vals:
        for a in (canon(va), loose(va, B28)) if va >> 364 < B28 else ():
            vb = _partners(rnd, va, CAP_Q, 2520 * P)[rnd.randrange(3)]
            b = loose(vb, B30) if rnd.random() < 0.7 else canon(vb)
            rem = CAP_Q - va * vb
            vd = rnd.choice([2 * P - 1, P, rnd.randrange(2 * P), 1])
            vc = min(rem // vd, 2520 * P) - rnd.choice([0, 0, 1, rnd.randrange(1 << 64)])
            vc = max(vc, 0)
            c, dd = loose(vc, B30), canon(vd)
            cases.append((a, b, c, dd) if rnd.random() < 0.5 else (c, dd, b, a))
    res = [L.v28(L.fq28_mul2(*c)) for c in cases]
    assert len(cases) >= 100 and 0 in res and res.count(P) >= 2
    assert sum(1 for a, b, c, d in cases if L.v28(a) * L.v28(b) + L.v28(c) * L.v28(d) == CAP_Q) >= 3
    return cases


def fq28_normalise_cases(seed=0x0928):
    rnd = random.Random(seed)
    hi = 0xfffffff0            # a limb + the carry of the limb below (at most 15) stays inside 32 bits
    cases = [[hi] * 14, [0] * 14, [(1 << 28) - 1] * 14, [(1 << 28)] * 14, [hi] * 13 + [0], single(0, hi), single(12, hi), single(13, hi)]
    for v in fq_values(rnd):
        cases += [canon(v), loose(v, 1 << 30), loose(v, 1 << 31)]
    cases += [[rnd.randrange(hi + 1) for _ in range(14)] for _ in range(60)]
    assert len(cases) >= 200
    return cases


FQ_SUBS = {  # name: (table, documented subtrahend: value bound in p, limb bound of limbs 0..12)
    "sub4": ("KP4_29", 2, 1 << 28), "sub8": ("KP8_29", 6, 1 << 28), "sub16": ("KP16_29", 14, 1 << 28), "sub8w": ("KP8_30", 4, 1 << 29)}


def fq28_sub_cases(name, seed=0x5B28):
    """(a, b) for sub4 / sub8 / sub16 / sub8w: subtrahends up to the documented bound and up to the K p constant itself, limb for limb"""
    rnd = random.Random(seed + len(name) + int(name[3:].rstrip("w")))
    table, kmax, lb = FQ_SUBS[name]
    K = L.FQ[table]
    bs = [list(K), [0] * 14, canon(kmax * P - 1), canon(kmax * P - 2), [lb - 1] * 13 + [(kmax * P - 1) >> 364], [lb - 1] * 13 + [0]]
    bs += [[K[i] if j == i else 0 for j in range(14)] for i in range(14)]
    for v in fq_values(rnd):
        if v < kmax * P:
            bs += [canon(v), loose(v, lb)]
    as_ = [[0] * 14, [(1 << 30) - 1] * 14, [0xb0000000 - 1] * 14]
    cases = []
    for b in bs:
        for a in as_ + [loose(rnd.randrange(18 * P), 1 << 30), canon(rnd.randrange(2 * P))]:
            cases.append((a, b))
    assert len(cases) >= 300
    return cases


def fq28_neg4_cases(seed=0x4E28):
    rnd = random.Random(seed)
    cases = [list(L.FQ["KP4_29"]), canon(0), canon(1), canon(P - 1), canon(P), canon(2 * P - 1), [(1 << 28) - 1] * 13 + [0]]
    cases += [canon(rnd.randrange(P)) for _ in range(120)]
    return cases


def fq28_is_zero_cases(seed=0x1528):
    rnd = random.Random(seed)
    mod = L.FQ["MOD"]
    cases = [canon(v) for v in (0, 1, P - 1, P, P + 1, 2 * P - 1, 1 << 364, 1 << 380)]
    for i in range(14):   # p and 0 with one limb off by one bit: neither is a multiple of p
        for bit in (0, 13, 27 if i < 13 else 16):
            if (mod[i] ^ (1 << bit)) < (1 << 28):
                m = list(mod)
                m[i] ^= 1 << bit
                if L.v28(m) < 2 * P:
                    cases.append(m)
            cases.append(single(i, 1 << bit))
    cases += [canon(rnd.randrange(2 * P)) for _ in range(100)]
    res = [L.fq28_tight_is_zero_mod_p(c) for c in cases]
    assert res.count(True) == 2 and len(cases) >= 150
    return cases


def words_cases(nwords, seed, specials):
    rnd = random.Random(seed)
    full = (1 << (32 * nwords)) - 1
    vals = list(specials) + [0, 1, full, full - 1, 0x5555555555555555555555555555555555555555555555555555555555555555 & full,
                             0xaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaaa & full]
    vals += [1 << k for k in range(0, 32 * nwords, 7)] + [(1 << k) - 1 for k in range(1, 32 * nwords, 11)]
    vals += [rnd.randrange(full + 1) for _ in range(60)]
    return [L.words32(v, nwords) for v in vals]


# ---- Fr29 ----------------------------------------------------------------------------------------------------------------
def c29(v):
    return canon(v, 29, 9)


def l29(v, bound):
    return loose(v, bound, 29, 9)


def fr29_mul_cases(seed=0xF929):
    """(a, b): limbs of a below 2^31, of b below 2^29, value products at and under 70 r^2"""
    rnd = random.Random(seed)
    BA, BB = 1 << 31, 1 << 29
    bmax, amax = (1 << 261) - 1, 70 * R
    cases = []
    for va in fr_values(rnd):
        for a in (c29(va), l29(va, BA), l29(va, 1 << 30)):
            for vb in _partners(rnd, va, CAP_R, bmax):
                cases.append((a, c29(vb)))
    for vb in fr_values(rnd):
        if vb <= bmax:
            for va in _partners(rnd, vb, CAP_R, amax):
                cases += [(c29(va), c29(vb)), (l29(va, BA), c29(vb))]
    for ka, kb in ((1, 70), (2, 35), (7, 10), (8, 8), (34, 2), (70, 1)):
        for da, db in ((0, 0), (-1, 0), (0, -1)):
            cases += [(l29(ka * R + da, BA), c29(kb * R + db)), (c29(ka * R + da), c29(kb * R + db))]
    cases += [(single(i, BA - 1, 9), c29(_partners(rnd, (BA - 1) << (29 * i), CAP_R, bmax)[0])) for i in range(9)]
    cases += [([BA - 1] * 9, c29(_partners(rnd, L.v29([BA - 1] * 9), CAP_R, bmax)[0])), ([BA - 1] * 8 + [0], [BB - 1] * 8 + [0]),
              (l29(R, BA), c29(0)), (c29(0), [BB - 1] * 9)]
    res = [L.v29(L.fr29_mul(a, b)) for a, b in cases]
    assert len(cases) >= 600 and res.count(0) >= 2 and res.count(R) >= 8
    assert sum(1 for a, b in cases if L.v29(a) * L.v29(b) == CAP_R) >= 6
    return cases


def fr29_to_canonical_cases(seed=0xCA29):
    rnd = random.Random(seed)
    vals = [(1 << 261) - 1, (1 << 261) - 2, 1 << 260, (1 << 249) - 1, 1 << 249]
    for k in range(71):
        vals += [k * R - 1, k * R, k * R + 1] if k else [0, 1]
    # values at which the quotient estimate is one short: right above a multiple of r that the truncated top bits cannot tell from below
    vals += [k * R + rnd.randrange(1 << 245) for k in range(1, 71) for _ in range(2)]
    vals += [rnd.randrange(1 << 261) for _ in range(100)]
    cases = []
    for v in vals:
        cases += [c29(v), l29(v, 1 << 31)]
    info = [L.fr29_to_canonical(c) for c in cases]
    short = [s for _, s in info]
    outs = [L.value(w, 32) for w, _ in info]
    assert len(cases) >= 700 and short.count(True) >= 60 and short.count(False) >= 60
    assert any(s and o == 0 for o, s in zip(outs, short))          # k r itself, met with the estimate k - 1
    assert 0 in outs and R - 1 in outs
    return cases


def fr_mem_cases(seed=0x3E29):
    """pairs of 8-word operands of the memory-form product, canonical and not (anything below 2^256)"""
    rnd = random.Random(seed)
    sp = [0, 1, 2, R - 1, R, R + 1, 2 * R - 1, 2 * R, 1 << 255, (1 << 256) - 1, (1 << 256) - 2, (1 << 256) % R, rnd.randrange(R), rnd.randrange(1 << 256)]
    pairs = [(a, b) for a in sp for b in sp]
    pairs += [(rnd.randrange(R), rnd.randrange(R)) for _ in range(100)] + [(rnd.randrange(1 << 256), rnd.randrange(1 << 256)) for _ in range(100)]
    assert len(pairs) >= 350
    return [(L.words32(a, 8), L.words32(b, 8)) for a, b in pairs]


def fr29_sub_cases(name, seed=0x5B29):
    rnd = random.Random(seed + len(name))
    K, kmax = (L.FR["KP4"], 2) if name == "sub_tight" else (L.FR["KP8"], 4)
    bs = [list(K), [0] * 9, c29(kmax * R - 1), [(1 << 29) - 1] * 8 + [(kmax * R - 1) >> 232], [(1 << 29) - 1] * 8 + [0]]
    bs += [[K[i] if j == i else 0 for j in range(9)] for i in range(9)]
    bs += [c29(v) for v in fr_values(rnd) if v < kmax * R]
    as_ = [[0] * 9, [(1 << 31) - 1] * 9, [0xc0000000 - 1] * 9]
    cases = [(a, b) for b in bs for a in as_ + [l29(rnd.randrange(34 * R), 1 << 31), c29(rnd.randrange(2 * R))]]
    assert len(cases) >= 150
    return cases


def fr29_normalise_cases(seed=0x0929):
    rnd = random.Random(seed)
    hi = 0xfffffff0
    cases = [[hi] * 9, [0] * 9, [(1 << 29) - 1] * 9, [1 << 29] * 9, single(0, hi, 9), single(8, hi, 9)]
    for v in fr_values(rnd):
        cases += [c29(v), l29(v, 1 << 31), l29(v, 1 << 32)]
    cases += [[rnd.randrange(hi + 1) for _ in range(9)] for _ in range(60)]
    return cases


def fr29_pack_cases(seed=0x9A29):
    rnd = random.Random(seed)
    vals = [0, 1, R - 1, R, 2 * R - 1, (1 << 256) - 1, 1 << 255, (1 << 232) - 1, 1 << 232] + [(1 << k) + 1 for k in range(29, 256, 29)]
    vals += [rnd.randrange(2 * R) for _ in range(100)]
    return [c29(v) for v in vals]


def fr_canonical_words(seed=0x7129):
    rnd = random.Random(seed)
    vals = [0, 1, R - 1, R - 2, (R + 1) // 2, (R - 1) // 2, (1 << 256) % R] + [(R >> k) + d for k in range(1, 7) for d in (0, 1)]
    vals += [(k * R) // 32 + d for k in range(1, 32) for d in (0, 1)]      # where one of the five doublings crosses r
    vals += [rnd.randrange(R) for _ in range(100)]
    return [L.words32(v % R, 8) for v in vals]


# ---- saturated Fp and Goldilocks -----------------------------------------------------------------------------------------
def fp_pairs(field, seed=0x5A70):
    mod, n = L.sat_mod(field)
    rnd = random.Random(seed + n)
    sp = [0, 1, 2, mod - 1, mod - 2, (mod + 1) // 2, (mod - 1) // 2, (1 << (32 * n)) % mod, (1 << (32 * n - 32)) - 1, 1 << (32 * (n - 1)),
          (1 << 32) - 1, 1 << 32]
    sp = [v % mod for v in sp]
    pairs = [(a, b) for a in sp for b in sp] + [(rnd.randrange(mod), rnd.randrange(mod)) for _ in range(150)]
    assert len(pairs) >= 290
    return [(L.words32(a, n), L.words32(b, n)) for a, b in pairs]


GL_SPECIALS = [0, 1, 2, (1 << 32) - 1, 1 << 32, (1 << 32) + 1, 1 << 63, GL - 2, GL - 1]


def gl_pairs(seed=0x6011, any64=False):
    rnd = random.Random(seed)
    sp = list(GL_SPECIALS) + ([GL, GL + 1, (1 << 64) - 1] if any64 else [])
    pairs = [(a, b) for a in sp for b in sp]
    top = (1 << 64) if any64 else GL
    pairs += [(rnd.randrange(top), rnd.randrange(top)) for _ in range(200)]
    pairs += [(rnd.randrange(GL), GL - 1 - rnd.randrange(1 << 20)) for _ in range(40)]
    return pairs


def gl_reduce_pairs(seed=0x6012):
    """(lo, hi) such that every reachable combination of the three conditional corrections of gl_reduce128 occurs"""
    rnd = random.Random(seed)
    e = (1 << 32) - 1
    los = [0, 1, e - 1, e, e + 1, 1 << 63, GL - 1, GL, GL + 1, (1 << 64) - 1, (1 << 64) - (1 << 32), (1 << 64) - (1 << 33), (1 << 64) - (1 << 33) + 2]
    cs = [0, 1, 2, e - 1, e, 1 << 31]
    pairs = [(lo, (c3 << 32) | c2) for lo in los for c3 in cs for c2 in cs]
    for _ in range(150):
        k = rnd.randrange(1 << 64)
        for x in (k * GL, k * GL - 1 if k else 0, k * GL + 1):
            pairs.append((x & L.M64, x >> 64))
    pairs += [(rnd.randrange(1 << 64), rnd.randrange(1 << 64)) for _ in range(200)]
    pairs += [(rnd.randrange(1 << 32), rnd.randrange(1 << 64)) for _ in range(100)]       # lo below c3: the first wrap
    info = [L.gl_reduce128(lo, hi) for lo, hi in pairs]
    combos = {b for _, b in info}
    reachable = {(False, False, False), (False, False, True), (False, True, False), (True, False, False), (True, False, True), (True, True, False)}
    assert combos == reachable, sorted(reachable - combos)      # a wrap at + c2 EPS leaves a value below p: (x, True, True) cannot occur
    res = [r for r, _ in info]
    assert res.count(0) >= 50 and res.count(GL - 1) >= 50 and len(pairs) >= 1000
    return pairs


# ---- G1 ------------------------------------------------------------------------------------------------------------------
T3 = (0, 2)      # a curve point with x = 0 (order 3): its X is the all-zero limb vector and must not read as infinity
_MULT = {}


def kG(k):
    if k not in _MULT:
        _MULT[k] = M.g1_mul(M.G1, k)
    return _MULT[k]


def stored_reps(rnd, pt, n):
    """n representations of one point as a stored XYZZ point, the worst the invariant admits first"""
    reps = [L.x28_from_point(pt, 1, 0, 0), L.x28_from_point(pt, rnd.randrange(2, P), 13, 5), L.x28_from_point(pt, 1, 13, 5),
            L.x28_from_point(pt, rnd.randrange(2, P), 0, 0)]
    while len(reps) < n:
        reps.append(L.x28_from_point(pt, rnd.randrange(2, P), rnd.randrange(14), rnd.randrange(6)))
    return reps[:n]


def arrange(ordinary, exceptional, wave=64):
    """uniform waves of ordinary cases, waves that mix both kinds, and a closing wave of exceptional cases only"""
    assert len(ordinary) >= 2 * wave and exceptional
    out = list(ordinary[:wave])
    rest = list(ordinary[wave:])
    step = max(1, len(rest) // len(exceptional))
    for i, e in enumerate(exceptional):
        out += rest[i * step:(i + 1) * step] + [e]
    out += rest[len(exceptional) * step:]
    out += [ordinary[0]] * (-len(out) % wave)
    out += [exceptional[i % len(exceptional)] for i in range(wave)]
    return out


def g1_madd_cases(seed=0x61AD):
    """(kind, acc as X28, q as A28)"""
    rnd = random.Random(seed)
    ordinary, exc = [], []
    pts = [kG(k) for k in range(1, 9)] + [T3]
    for i, a in enumerate(pts):
        for j, q in enumerate(pts):
            if a[0] == q[0]:
                continue
            for rep in stored_reps(rnd, a, 3):
                ordinary.append(("sum", rep, L.a28_from_point(q, 0, neg_form=rnd.random() < 0.5)))
    for a in pts:
        for neg in (False, True):
            q = L.a28_from_point(a, 0, neg)
            exc.append(("acc infinite", L.x28_infinity(), q))
            exc.append(("acc infinite", L.x28(L.FQ_ONE, canon(5 * P + 1), L.FQ_ZERO, L.FQ_ONE), q))     # ZZ = 0 decides, whatever X, Y hold
            for rep in stored_reps(rnd, a, 3):
                exc.append(("double", rep, q))
                exc.append(("cancel", rep, L.a28_from_point(M.g1_neg(a), 0, neg)))
    cases = arrange(ordinary, exc)
    assert len(ordinary) >= 200 and len(exc) >= 100
    return cases


def g1_mmadd_cases(seed=0x33AD):
    """(kind, acc: the affine point a first insertion left, as X28 with ZZ = ZZZ = 1, q as A28)"""
    rnd = random.Random(seed)
    ordinary, exc = [], []
    pts = [kG(k) for k in range(1, 11)] + [T3]

    def first(pt, neg):    # what g1_28_madd leaves in an empty bucket
        a = L.a28_from_point(pt, 0, neg)
        return L.x28(a["x"], L.fq28_normalise(a["y"]), L.FQ_ONE, L.FQ_ONE)
    for a in pts:
        for q in pts:
            for na in (False, True):
                for nq in (False, True):
                    if a[0] != q[0]:
                        ordinary.append(("sum", first(a, na), L.a28_from_point(q, 0, nq)))
                    else:
                        exc.append(("same x", first(a, na), L.a28_from_point(q, 0, nq)))
                        exc.append(("same x", first(a, na), L.a28_from_point(M.g1_neg(q), 0, nq)))
    cases = arrange(ordinary, exc)
    assert len(ordinary) >= 200 and len(exc) >= 40
    return cases


def g1_add_cases(seed=0xADD0):
    """(kind, a, b), both X28"""
    rnd = random.Random(seed)
    ordinary, exc = [], []
    pts = [kG(k) for k in range(1, 8)] + [T3]
    inf = L.x28_infinity()
    for a in pts:
        for b in pts:
            if a[0] != b[0]:
                for ra, rb in zip(stored_reps(rnd, a, 3), stored_reps(rnd, b, 3)[::-1]):
                    ordinary.append(("sum", ra, rb))
        ra = stored_reps(rnd, a, 4)
        rb = stored_reps(rnd, a, 4)[::-1]
        rn = stored_reps(rnd, M.g1_neg(a), 4)
        for i in range(4):
            exc += [("a infinite", inf, ra[i]), ("b infinite", ra[i], inf), ("double", ra[i], rb[i]), ("cancel", ra[i], rn[i])]
    exc += [("both infinite", inf, inf), ("both infinite", L.x28(L.FQ_ONE, L.FQ_ONE, L.FQ_ZERO, L.FQ_ONE), inf)]
    cases = arrange(ordinary, exc)
    assert len(ordinary) >= 150 and len(exc) >= 100
    return cases


def g1_double_cases(seed=0xD0B1):
    rnd = random.Random(seed)
    return [rep for k in list(range(1, 12)) + [None] for rep in stored_reps(rnd, kG(k) if k else T3, 6)]


def g1_double_affine_cases():
    return [L.a28_from_point(kG(k) if k else T3, 0, neg) for k in list(range(1, 40)) + [None] for neg in (False, True)]
