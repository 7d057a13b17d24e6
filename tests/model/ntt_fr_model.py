"""Limb-level model of the Fr transform passes (csrc/ntt.hpp: ntt_pass_strided<Fr>, ntt_pass_last<Fr>, ntt_tile / ntt_round with K = 2) on the
primitives of limb_model.py, the same walk on BOUNDS instead of data, and the builder of the adversarial vectors that drive the lazy
reduction to its ceiling.

Three things live here:

  Transform   one transform as the driver runs it (csrc/ntt_host.inc: run_ntt): radices and table shapes from tests/golden/ntt_plans.txt,
              the tables the driver builds, and the pass kernels for one tile column at a time.  Every limb_model primitive checks its
              own contract, so a vector that runs through raises ContractError at the first operand outside a documented bound, and
              the words it returns are the words the device must store.
  walk        the tile on ceilings: a value ceiling and nine limb ceilings per row, for the two classes of tile input (canonical
              words below r; tight products below 2r), and check_consumers for what reads the grown values afterwards.
  adversarial_column
              inputs for one tile column whose row R - 2 comes within 2r of the walk's ceiling, searched on vtile, the tile on
              values alone.

A tile column is a list of 2^log_r limb lists in TILE ROW ORDER: row e holds input bitrev(e) (the kernels load the rows bit-reversed).
Values are the integers the words have in memory (the arkworks residue a 2^256 mod r), as in fr29.hpp.

ntt_round's item loop is restated stage by stage: the items of a round touch disjoint rows, a stage pairs row `low` with row
low | 2^s, and O::fix runs on every row once the round's K stages are done.  That is the same arithmetic on the same operands."""
import os
import random
import re

import bigmodel as M
import limb_model as L

R = M.R
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
K = 2             # NttOps<Fr>::K
UNIT_Q_MAX = 1    # NttOps<Fr>::UNIT_Q_MAX
MONT256 = (1 << 256) % R
MASK29 = (1 << 29) - 1
# a product of two table entries (powtab_get: lo * hi, both canonical): below lo hi / 2^261 + r = 1.0142 r.  The bound of every factor
# that is not canonical: the inter-pass twiddle off the two-level table and the coset power.
FACTOR_CANONICAL = R - 1
FACTOR_PRODUCT = ((R - 1) * (R - 1) >> 261) + R


def bitrev(x, bits):
    return int(format(x, "0%db" % bits)[::-1], 2) if bits else 0


# ---------------------------------------------------------------------------------------------------------------------------
# Plans: read, not derived
# ---------------------------------------------------------------------------------------------------------------------------
_plans = None


def plans():
    """(log_n, wide, inverse, matrix allowed) -> dict(passes, r, h, matrix, strided [(log_outer, inner, log_t, direct_len)], last)"""
    global _plans
    if _plans is None:
        _plans = {}
        pat = re.compile(r"ntt f=fr log_n=(\d+) wide=(\d) inv=(\d) nowide=0 mmax=(\d+) -> passes=(\d) r=([\d,]+) h=(\d+) .*?"
                         r"((?:p\d=[\d,]+ )*)matrix=(\d) last=([\d,]+)")
        for line in open(os.path.join(ROOT, "tests", "golden", "ntt_plans.txt")):
            m = pat.match(line)
            if not m or m.group(4) not in ("0", "24"):
                continue
            passes = int(m.group(5))
            strided = [tuple(int(v) for v in p.split("=")[1].split(",")) for p in m.group(8).split()]
            last = [int(v) for v in m.group(10).split(",")]
            _plans[(int(m.group(1)), int(m.group(2)), int(m.group(3)), m.group(4) == "24")] = {
                "passes": passes, "r": [int(v) for v in m.group(6).split(",")][:passes], "h": int(m.group(7)),
                "matrix": m.group(9) == "1", "strided": [(s[0], s[1], s[2], s[5]) for s in strided],
                "last": dict(zip(("log_r", "log_r0", "log_m", "log_r1", "t_log"), last))}
    return _plans


def fr_radices():
    """every radix a recorded Fr plan contains"""
    return sorted({r for p in plans().values() for r in p["r"]})


# ---------------------------------------------------------------------------------------------------------------------------
# Tables, as ntt_host.inc builds them (pow_table_kernel: canonical twiddle form w 2^261 mod r)
# ---------------------------------------------------------------------------------------------------------------------------
_tw_cache = {}


def tw_of(x):
    """the stored twiddle of the field element x (NttOps<Fr>::to_tw of its Montgomery form)"""
    t = _tw_cache.get(x)
    if t is None:
        t = _tw_cache[x] = L.fr29_twiddle_from_mont(L.words32(x * MONT256 % R, 8))
    return t


def root(log_n, inverse):
    w = M.root_of_unity(log_n)
    return pow(w, -1, R) if inverse else w


_radix_cache = {}


def radix_table(log_r, inverse):
    key = (log_r, bool(inverse))
    if key not in _radix_cache:
        w, t, out = root(log_r, inverse), 1, []
        for _ in range((1 << log_r) >> 1):
            out.append(tw_of(t))
            t = t * w % R
        _radix_cache[key] = out
    return _radix_cache[key]


class PowTab:
    """value(e) = lo[e & (2^h - 1)] * hi[e >> h], lo[e] = c base^e, hi[j] = base^(j 2^h); entries made on demand"""

    def __init__(self, base, c, h):
        self.base, self.c, self.h = base, c, h

    def get(self, e):
        a = tw_of(self.c * pow(self.base, e & ((1 << self.h) - 1), R) % R)
        hi = e >> self.h
        if hi:   # a tight product, not canonical
            a = L.fr29_mul(a, tw_of(pow(self.base, hi << self.h, R)), what="powtab_get")
        return a


def load(word):
    return L.fr29_from_sat(L.words32(word, 8))


def store(x):
    """NttOps<Fr>::store.  fr29_to_canonical takes the quotient estimate from the top limb: below 2^29 is what QEST's range covers."""
    n = L.fr29_normalise(x)
    L.need(n[8] < (1 << 29), "store: top limb not below 2^29")
    return L.value(L.fr29_to_canonical(x)[0], 32)


def store_tight(x):
    return L.value(L.fr29_pack_tight(x), 32)


# ---------------------------------------------------------------------------------------------------------------------------
# The tile
# ---------------------------------------------------------------------------------------------------------------------------
def rounds_of(log_r):
    """(first stage, stages, FIRST) of the ntt_round calls of ntt_tile"""
    out, s = [], 0
    if K <= log_r:
        out.append((0, K, True))
        s = K
    while s + K <= log_r:
        out.append((s, K, False))
        s += K
    if log_r - s == 1:
        out.append((s, 1, False))
    return out


class Trace:
    """What the tiles of a run went through: the largest value after each stage"""

    def __init__(self):
        self.max_value, self.stage_max = 0, {}

    def stage(self, s, x, lo, hi):
        m = max(L.v29(x[row]) for row in range(lo, hi))
        self.stage_max[s] = max(self.stage_max.get(s, 0), m)
        self.max_value = max(self.max_value, m)


def tile(x, log_r, tw, trace=None, variant=""):
    """ntt_tile on one column, in place.
    variant: the mutants the tests try: "no_fix" (no normalise at the end of a round), "unit_sub_tight" (the unit butterfly
    subtracts from 4r)."""
    lo, hi = 0, 1 << log_r
    for s_lo, k, first in rounds_of(log_r):
        for q in range(k):
            s = s_lo + q
            bit = 1 << s
            for low in range(lo, hi):
                if low & bit:
                    continue
                high = low | bit
                u, v = x[low], x[high]
                if first and 1 <= q <= UNIT_Q_MAX and (low & ((1 << q) - 1)) == 0:   # O::unit_butterfly: twiddle 1 for every lane
                    t = L.fr29_normalise(v)
                    x[high] = L.fr29_sub_tight(u, t) if variant == "unit_sub_tight" else L.fr29_sub_wide8(u, t)
                    x[low] = L.fr29_add(u, t)
                    continue
                if s == 0:
                    t = v
                else:
                    t = L.fr29_mul(v, tw[(low & (bit - 1)) << (log_r - 1 - s)], what="stage %d row %d" % (s, high))
                x[low] = L.fr29_add(u, t)
                x[high] = L.fr29_sub_tight(u, t)
            if trace is not None:
                trace.stage(s, x, lo, hi)
        if variant != "no_fix":
            for row in range(lo, hi):
                x[row] = L.fr29_normalise(x[row])


# ---------------------------------------------------------------------------------------------------------------------------
# One transform
# ---------------------------------------------------------------------------------------------------------------------------
class Transform:
    """run_ntt<Fr> for one (log_n, direction, coset, allow_wide, matrix knob).  coset: the memory word of g (Montgomery form), or None."""

    def __init__(self, log_n, inverse=False, coset=None, wide=False, matrix=True, variant=""):
        self.log_n, self.inverse, self.variant = log_n, bool(inverse), variant
        self.plan = pl = plans()[(log_n, int(wide), int(self.inverse), bool(matrix))]
        self.P, self.r = pl["passes"], pl["r"]
        n_inv = pow(1 << log_n, -1, R)
        self.w = root(log_n, self.inverse)
        self.pre = self.post = self.post_const = None
        ninv_in_pass0 = False
        if coset is not None:
            g = coset * pow(MONT256, -1, R) % R
            tab = PowTab(pow(g, -1, R) if self.inverse else g, n_inv if self.inverse else 1, (log_n + 1) // 2)
            if self.inverse:
                self.post = tab
            else:
                self.pre = tab
        elif self.inverse and self.P == 1:
            self.post_const = tw_of(n_inv)
        else:
            ninv_in_pass0 = self.inverse
        self.inter0 = PowTab(self.w, n_inv if ninv_in_pass0 else 1, pl["h"])   # pass 0: inter_lo_ninv on an inverse
        self.inter = PowTab(self.w, 1, pl["h"])
        self.tw = [radix_table(r, self.inverse) for r in self.r]

    # -- a strided pass (p < P - 1): view [outer][R][inner], one column (o, i)
    def column_indices(self, p, o, i):
        """the element index of input j = 0 .. R - 1 of column (o, i); output k lands where input k was"""
        _, inner, _, _ = self.plan["strided"][p]
        return [((o << self.r[p]) + j) * inner + i for j in range(1 << self.r[p])]

    def factor(self, p, k, i):
        """the inter-pass twiddle of output k of a column with inner index i"""
        log_outer, _, _, direct_len = self.plan["strided"][p]
        if p == 0 and self.plan["matrix"]:   # twiddle_matrix_kernel: tw_pack on the way in, tw_unpack on the way out
            return L.fr29_from_sat(L.fr29_to_canonical(self.inter0.get(k * i))[0])
        if p > 0 and direct_len:
            return tw_of(pow(self.w, (k * i) << log_outer, R))
        return (self.inter0 if p == 0 else self.inter).get((k * i) << log_outer)

    def column_load(self, p, o, i, words):
        """words: the R memory words of the column, input order -> the tile column"""
        log_r = self.r[p]
        idx = self.column_indices(p, o, i)
        x = []
        for e in range(1 << log_r):
            j = bitrev(e, log_r)
            v = load(words[j])
            if p == 0 and self.pre is not None:
                v = L.fr29_mul(v, self.pre.get(idx[j]), what="pre-scale")
            x.append(v)
        return x

    def column_store(self, p, i, x):
        """the inter-pass product and store_tight -> R memory words, output order"""
        return [store_tight(L.fr29_mul(x[k], self.factor(p, k, i), what="inter-pass product")) for k in range(len(x))]

    def column(self, p, o, i, words, trace=None):
        x = self.column_load(p, o, i, words)
        tile(x, self.r[p], self.tw[p], trace=trace, variant=self.variant)
        return self.column_store(p, i, x)

    # -- the last pass: view [R0][M][R], one tile column (k0, m)
    def last_indices(self, k0, m):
        """(input index of j, output index of k) for j, k = 0 .. R - 1"""
        l = self.plan["last"]
        log_r2 = l["log_m"] - l["log_r1"]
        mrev = (m >> log_r2) | ((m & ((1 << log_r2) - 1)) << l["log_r1"])
        rr = 1 << l["log_r"]
        return ([(((k0 << l["log_m"]) + m) << l["log_r"]) + j for j in range(rr)],
                [k0 + ((mrev + (k << l["log_m"])) << l["log_r0"]) for k in range(rr)])

    def last_load(self, k0, m, words):
        log_r = self.plan["last"]["log_r"]
        idx = self.last_indices(k0, m)[0]
        x = []
        for e in range(1 << log_r):
            j = bitrev(e, log_r)
            v = load(words[j])
            if self.P == 1 and self.pre is not None:
                v = L.fr29_mul(v, self.pre.get(idx[j]), what="pre-scale")
            x.append(v)
        return x

    def last_store(self, k0, m, x):
        out = self.last_indices(k0, m)[1]
        res = []
        for k, v in enumerate(x):
            if self.post_const is not None:
                v = L.fr29_mul(v, self.post_const, what="post-scale (1/n)")
            elif self.post is not None:
                v = L.fr29_mul(v, self.post.get(out[k]), what="post-scale (coset)")
            res.append(store(v))
        return res

    def last(self, k0, m, words, trace=None):
        x = self.last_load(k0, m, words)
        tile(x, self.plan["last"]["log_r"], self.tw[-1], trace=trace, variant=self.variant)
        return self.last_store(k0, m, x)

    def pass_strided(self, p, data, trace=None):
        log_outer, inner, _, _ = self.plan["strided"][p]
        out = list(data)
        for o in range(1 << log_outer):
            for i in range(inner):
                idx = self.column_indices(p, o, i)
                for at, v in zip(idx, self.column(p, o, i, [data[j] for j in idx], trace)):
                    out[at] = v
        return out

    def pass_last(self, data, trace=None):
        l = self.plan["last"]
        out = [0] * len(data)
        for k0 in range(1 << l["log_r0"]):
            for m in range(1 << l["log_m"]):
                src, dst = self.last_indices(k0, m)
                for at, v in zip(dst, self.last(k0, m, [data[j] for j in src], trace)):
                    out[at] = v
        return out

    def run(self, words, trace=None):
        """memory words in natural order -> memory words in natural order"""
        assert len(words) == 1 << self.log_n
        data = list(words)
        for p in range(self.P - 1):
            data = self.pass_strided(p, data, trace)
        return self.pass_last(data, trace)


def ntt_fr(words, inverse=False, coset=None, wide=False, matrix=True, trace=None, variant=""):
    return Transform(len(words).bit_length() - 1, inverse, coset, wide, matrix, variant).run(words, trace)


# ---------------------------------------------------------------------------------------------------------------------------
# The same tile on ceilings
# ---------------------------------------------------------------------------------------------------------------------------
class Bound:
    """inclusive ceilings: of the value, and of each of the nine limbs"""
    __slots__ = ("v", "l")

    def __init__(self, v, l):
        self.v, self.l = v, l


def b_input(cls):
    """canonical: a word below r through fr29_from_sat.  tight: a product, or a word below 2r through fr29_from_sat."""
    v = {"canonical": R - 1, "tight": 2 * R - 1}[cls]
    return Bound(v, [MASK29] * 8 + [v >> 232])


def b_add(a, b):
    l = [x + y for x, y in zip(a.l, b.l)]
    L.need(max(l) <= L.M32, "add: a limb sum can wrap 32 bits")
    return Bound(a.v + b.v, l)


def b_sub(u, t, table, k, what):
    for i in range(9):
        L.need(t.l[i] <= table[i], "%s: limb %d of the subtrahend can reach %#x, above the constant's %#x" % (what, i, t.l[i], table[i]))
    l = [x + c for x, c in zip(u.l, table)]
    L.need(max(l) <= L.M32, what + ": a limb can wrap 32 bits")
    return Bound(u.v + k * R, l)


def b_normalise(a):
    c, l = 0, []
    for i in range(8):
        t = a.l[i] + c
        L.need(t <= L.M32, "normalise: limb + carry can wrap 32 bits")
        l.append(min(t, MASK29))
        c = t >> 29
    L.need(a.l[8] + c <= L.M32, "normalise: top limb + carry can wrap 32 bits")
    return Bound(a.v, l + [min(a.l[8] + c, a.v >> 232)])


def b_mul(a, factor, what):
    """a * w for any w <= factor with limbs below 2^29: the contract of fr29.hpp's product; the result is tight"""
    L.need(max(a.l) < (1 << 31), "%s: a limb of the multiplier can reach %#x, not below 2^31" % (what, max(a.l)))
    L.need(a.v * factor <= 70 * R * R, "%s: value product can reach %.2f r^2, above 70 r^2" % (what, a.v * factor / (R * R)))
    return b_input("tight")


def walk(log_r, cls, variant=""):
    """-> (the largest value ceiling after each stage, the Bound of every row at the end).  Raises ContractError where a ceiling
    leaves a contract inside the tile."""
    x = [b_input(cls) for _ in range(1 << log_r)]
    stages = []
    for s_lo, k, first in rounds_of(log_r):
        for q in range(k):
            s = s_lo + q
            bit = 1 << s
            for low in range(1 << log_r):
                if low & bit:
                    continue
                high = low | bit
                u, v = x[low], x[high]
                if first and 1 <= q <= UNIT_Q_MAX and (low & ((1 << q) - 1)) == 0:
                    t = b_normalise(v)
                    x[high] = b_sub(u, t, L.FR["KP4"], 4, "unit butterfly") if variant == "unit_sub_tight" else \
                        b_sub(u, t, L.FR["KP8"], 8, "unit butterfly")
                    x[low] = b_add(u, t)
                    continue
                t = v if s == 0 else b_mul(v, FACTOR_CANONICAL, "stage %d" % s)
                x[low] = b_add(u, t)
                x[high] = b_sub(u, t, L.FR["KP4"], 4, "stage %d" % s)
            stages.append(max(b.v for b in x))
        if variant != "no_fix":
            x = [b_normalise(b) for b in x]
    return stages, x


def check_consumers(rows):
    """What reads a finished tile: the inter-pass product (matrix / direct entry: canonical; two-level table: a product of two
    entries) before store_tight, the post-scale product (1/n: canonical; coset power: a product) before store, and store alone."""
    tight = b_input("tight")
    L.need(tight.v < (1 << 256) and max(tight.l[:8]) < (1 << 29), "a tight product does not fit fr29_pack_tight")
    for b in rows:
        b_mul(b, FACTOR_CANONICAL, "inter-pass / post-scale product, canonical factor")
        b_mul(b, FACTOR_PRODUCT, "inter-pass / post-scale product, factor from two table entries")
        n = b_normalise(b)
        L.need(n.l[8] < (1 << 29), "store: the top limb can reach %#x, not below 2^29" % n.l[8])
        L.need(b.v < (1 << 261), "store: the value can reach 2^261")


def ceiling(log_r, cls):
    return walk(log_r, cls)[0][-1]


# ---------------------------------------------------------------------------------------------------------------------------
# The tile on values.  The integer a Montgomery product returns depends on the integers of its operands alone, (a w + m r) / 2^261 with
# m = -a w / r mod 2^261, and neither the limb-wise sums nor normalise change a value: so the values of a tile can be followed without
# its limbs, some thirty times faster.  The builder below searches with this twin; the tests run what it finds through the limb
# model, which has to report the same largest value.
# ---------------------------------------------------------------------------------------------------------------------------
M261 = (1 << 261) - 1
RINV261 = pow(R, -1, 1 << 261)


def vmul(a, w):
    t = a * w
    return (t + ((-t * RINV261) & M261) * R) >> 261


_radix_values = {}


def radix_values(log_r, inverse):
    key = (log_r, bool(inverse))
    if key not in _radix_values:
        _radix_values[key] = [L.v29(w) for w in radix_table(log_r, inverse)]
    return _radix_values[key]


def vtile(x, log_r, twv, lo=0, hi=None, stop=None):
    """tile() on integers, in place -> the largest value after any stage.  lo, hi, stop: rows [lo, hi) only (an aligned block) and
    stages below `stop` only: what a product of stage `stop` in that block reads."""
    hi = (1 << log_r) if hi is None else hi
    stop = log_r if stop is None else stop
    top = 0
    for s_lo, k, first in rounds_of(log_r):
        for q in range(k):
            s = s_lo + q
            if s >= stop:
                return top
            bit = 1 << s
            for low in range(lo, hi):
                if low & bit:
                    continue
                high = low | bit
                u, v = x[low], x[high]
                if first and 1 <= q <= UNIT_Q_MAX and (low & ((1 << q) - 1)) == 0:
                    x[low], x[high] = u + v, u - v + 8 * R
                    continue
                t = v if s == 0 else vmul(v, twv[(low & (bit - 1)) << (log_r - 1 - s)])
                x[low], x[high] = u + t, u - t + 4 * R
            top = max(top, max(x[lo:hi]))
    return top


# ---------------------------------------------------------------------------------------------------------------------------
# Adversarial inputs for one tile column
# ---------------------------------------------------------------------------------------------------------------------------
class DirectLoader:
    """the user's word sits in the tile as it is (pass 0 or a single pass, no coset)"""

    def value(self, row, word):
        return word

    def operands(self, row, word):
        return None


class PreScaleLoader:
    """a single pass behind the coset pre-scale: the tile gets word * g^index, a tight product"""

    def __init__(self, tr):
        assert tr.P == 1 and tr.pre is not None
        log_r = tr.r[0]
        self.w = [L.v29(tr.pre.get(bitrev(row, log_r))) for row in range(1 << log_r)]

    def operands(self, row, word):
        return word, self.w[row]

    def value(self, row, word):
        return vmul(word, self.w[row])


class Pass0Loader:
    """the last-pass tile (k0, 0) of a two-pass transform: row e is output k0 of the pass-0 column bitrev(e), steered through input
    j0 of that column (the rest of the column stays as `data` has it)"""

    def __init__(self, tr, data, k0, j0=0):
        assert tr.P == 2 and tr.pre is None
        self.tr, self.data, self.k0, self.j0, self.log_r = tr, data, k0, j0, tr.plan["last"]["log_r"]
        self.twv = radix_values(tr.r[0], tr.inverse)
        self.w = {}

    def user_index(self, row):
        return self.tr.column_indices(0, 0, bitrev(row, self.log_r))[self.j0]

    def operands(self, row, word):
        i = bitrev(row, self.log_r)
        idx = self.tr.column_indices(0, 0, i)
        x = [word if j == self.j0 else self.data[idx[j]] for j in (bitrev(e, self.tr.r[0]) for e in range(len(idx)))]
        vtile(x, self.tr.r[0], self.twv)
        if row not in self.w:
            self.w[row] = L.v29(self.tr.factor(0, self.k0, i))
        return x[self.k0], self.w[row]

    def value(self, row, word):
        return vmul(*self.operands(row, word))


def steer(operands, rng, want, probes=4, steps=8):
    """A word x for which the Montgomery product a(x) * w comes out as small ("min") or as large ("max") an integer as it can.
    The residue of a is affine in x, and the product lies in [a w / 2^261, a w / 2^261 + r): a residue rho at or above
    floor(a w / 2^261) comes out as rho itself, one below it as rho + r.  Which representative of a arrives, and with it the floor,
    depends on x again: a few random words show the range of the floor, then the aim moves through that range (upwards from its low
    end for "min", downwards from its high end for "max") until the product comes out on the wanted side."""
    a0, a1 = operands(0)[0] % R, operands(1)[0] % R
    alpha_inv = pow((a1 - a0) % R, -1, R)   # (not invertible: the product does not depend on the freed input)
    best, floors = None, []

    def probe(x):
        nonlocal best
        a, w = operands(x)
        t = vmul(a, w)
        if best is None or (t < best[0] if want == "min" else t > best[0]):
            best = (t, x)
        floors.append(a * w >> 261)
        return t, w

    for _ in range(probes):
        _, w = probe(rng.randrange(R))
    lo, hi = min(floors), max(floors)
    step = max((hi - lo) // steps, 1)
    unit = (1 << 261) * pow(w, -1, R) % R
    for j in range(2 * steps + 1):
        rho = lo + 1 + j * step if want == "min" else max(hi - 1 - j * step, 0)
        t, _ = probe((rho * unit - a0) * alpha_inv % R)
        if t == (rho if want == "min" else rho + R):
            break
    return best[1]


def adversarial_column(log_r, inverse, loader, seed, words=None):
    """-> (the words of a tile column, TILE ROW ORDER, that send row R - 2 to the top of its range; the largest value the column
    then holds).  Row R - 2 ends as x0 - x2 + 8r + sum over s >= 2 of (4r - t_s), t_s the product formed from row 2^(s+1) - 2 at stage s:
    rows 0, 1 large, rows 2, 3 small, and in every block [2^s, 2^(s+1)) the input of row 2^s chosen so that t_s comes out small.  The
    blocks are disjoint.  words: what the rows hold to begin with (default: random words below r)."""
    rng = random.Random(seed)
    rr, twv = 1 << log_r, radix_values(log_r, inverse)
    words = [rng.randrange(R) for _ in range(rr)] if words is None else list(words)
    for row in range(min(4, rr)):
        want = "max" if row < 2 else "min"
        if loader.operands(row, 0) is None:
            words[row] = R - 1 if want == "max" else 0
        else:
            words[row] = steer(lambda x, row=row: loader.operands(row, x), rng, want)
    values = [loader.value(row, words[row]) for row in range(rr)]
    for s in range(2, log_r):
        lo, hi = 1 << s, 2 << s

        def operands(x, lo=lo, hi=hi, s=s):
            col = list(values)
            col[lo] = loader.value(lo, x)
            vtile(col, log_r, twv, lo=lo, hi=hi, stop=s)
            return col[hi - 2], twv[(lo - 2) << (log_r - 1 - s)]

        words[lo] = steer(operands, rng, "min")
        values[lo] = loader.value(lo, words[lo])
    return words, vtile(values, log_r, twv)


def random_reach(log_r, inverse, cls, seed, tiles=64):
    """the largest value over `tiles` random tile columns of an input class: canonical words, or tight products of a random word and a
    random canonical factor, as they arrive behind a pre-scale"""
    rng = random.Random(seed)
    twv, best = radix_values(log_r, inverse), 0
    for _ in range(tiles):
        x = [rng.randrange(R) for _ in range(1 << log_r)]
        if cls == "tight":
            x = [vmul(v, rng.randrange(R)) for v in x]
        best = max(best, vtile(x, log_r, twv))
    return best
