"""Ground truth for the MSM's bucket reduction (csrc/msm.hpp: msm_combine, msm_fold_parts*, msm_pyramid*, msm_collect; the hook
zkp_selftest_msm_reduce_dev of include/zkp_hip.h).  The truth is the group, not limbs: every bucket is a pool entry k G with a known
discrete log k, so what a bucket set must reduce to follows from the index map alone,

    result 0      S   = sum_i k[map[i]]                          (the sum of the set's buckets)
    result 1 + j  U_j = sum over i with bit j of i set           (i: the 0-based bucket index; the odd half of pyramid level j)

both mod r, and the expected points are ONE fixed-base multiplication over all of them.  The checker decodes every device point
(limb_model.affine_of), compares it with the expected point and holds it to the stored-point invariant (limb_model.check_stored): the next
add reads it.  Limbs of the outputs are not compared -- the three add forms are pinned limb by limb in tests/test_gpu_field_selftest.py,
and which form runs where is the plan's choice.

Layouts (a point is 64 words: X, Y, ZZ, ZZZ of 14 limbs + 2 zero words each):
  entry-major   (n, 64)
  plane-major   (16, cap, 4): chunk q (4 words) of entry e at uint4 index q cap + e
  a bucket set  nb = 2^(c-1) buckets, bucket b = i + 1 at entry w nb + pyr_pos(i, nb) -- even indices first, odd indices behind them."""
import random

import numpy as np

import limb_model as L

P, R = L.P, L.R
COORDS = ("x", "y", "zz", "zzz")
ONE, Z, WORST, NEG, Z2 = range(5)   # the variants of a pool point
NVAR = 5


def pyr_pos(i, n):
    """physical position of logical entry i of an n-entry pyramid level (msm_plan.hpp); works on numpy arrays"""
    return (i >> 1) + (i & 1) * (n >> 1)


def words_of(p):
    w = np.zeros(64, dtype=np.uint32)
    for j, c in enumerate(COORDS):
        w[16 * j:16 * j + 14] = p[c]
    return w


def point_of(w):
    """64 words -> the limb dict of limb_model; the two spare words of every coordinate must be zero, as every producer leaves them"""
    L.need(not any(int(w[16 * j + 14]) | int(w[16 * j + 15]) for j in range(4)), "a spare word of a coordinate is not zero")
    return {c: [int(v) for v in w[16 * j:16 * j + 14]] for j, c in enumerate(COORDS)}


def points_of_logs(orc, logs):
    """k G for every k of a flat list, as affine integer pairs; None (infinity) exactly where k = 0 mod r"""
    logs = [k % R for k in logs]
    if not logs:
        return []
    xy, inf = orc.g1_fixed_base_mul(orc.fr_from_ints(logs))
    pts = orc.points_to_ints(xy, inf)
    assert all((p is None) == (k == 0) for p, k in zip(pts, logs))
    return pts


class Pool:
    """nbase points k_j G, each in five forms, and infinity as the last entry.  k[e]: the discrete log of entry e; words[e]: its 64 words.
      ONE    ZZ = ZZZ = 1                               Z, Z2  the same point under two random z
      WORST  X raised by 13 p, Y by 5 p (random z): the worst representative the stored-point invariant admits
      NEG    the negation (log r - k_j) under a random z
    idx(j, variant) names an entry; INF is infinity, all-zero as every producer writes it, with log 0."""

    def __init__(self, orc, seed=0x9001, nbase=64):
        rnd = random.Random(seed)
        self.nbase = nbase
        self.base_k = [rnd.randrange(1, R) for _ in range(nbase)]
        self.base_pt = points_of_logs(orc, self.base_k)
        self.k, self.pt, words = [], [], []
        for kj, (x, y) in zip(self.base_k, self.base_pt):
            zs = [rnd.randrange(2, P) for _ in range(4)]
            forms = [(kj, (x, y), dict(z=1)), (kj, (x, y), dict(z=zs[0])), (kj, (x, y), dict(z=zs[1], kx=13, ky=5)),
                     (R - kj, (x, P - y), dict(z=zs[2])), (kj, (x, y), dict(z=zs[3]))]
            for k, pt, kw in forms:
                self.k.append(k)
                self.pt.append(pt)
                words.append(words_of(L.x28_from_point(pt, **kw)))
        self.INF = len(self.k)
        self.k.append(0)
        self.pt.append(None)
        words.append(np.zeros(64, dtype=np.uint32))
        self.words = np.stack(words)
        self.k_obj = np.array(self.k, dtype=object)

    def idx(self, j, variant=ONE):
        return (j % self.nbase) * NVAR + variant

    def __len__(self):
        return len(self.k)

    def gather(self, maps):
        """index maps of any shape -> the limb array, shape + (64,)"""
        return self.words[np.asarray(maps)]

    def logs(self, maps):
        """index maps of any shape -> object array of discrete logs"""
        return self.k_obj[np.asarray(maps)]


# ---- expected values, from the maps alone -----------------------------------------------------------------------------------
def result_logs(bucket_logs):
    """(W, nb) discrete logs of the buckets in logical order -> W rows [S, U_0, .., U_{c-2}] mod r"""
    bucket_logs = np.asarray(bucket_logs, dtype=object)
    nb = bucket_logs.shape[1]
    c = nb.bit_length()
    assert nb == 1 << (c - 1)
    i = np.arange(nb)
    sel = [np.ones(nb, dtype=bool)] + [((i >> j) & 1) == 1 for j in range(c - 1)]
    return [[int(sum(row[s].tolist())) % R for s in sel] for row in bucket_logs]


def fold_logs(part_logs):
    """(parts, ...) logs -> the folded buckets: the sum over the parts"""
    a = np.asarray(part_logs, dtype=object)
    out = a[0]
    for x in a[1:]:
        out = out + x
    return out % R


def combine_log(piece_logs, carry_log=0):
    """a combined bucket: the sum of its pieces, plus the carry under resume"""
    return (sum(int(k) for k in piece_logs) + int(carry_log)) % R


def result_name(e):
    return "sum" if e == 0 else f"U_{e - 1}: odd half of level {e - 1}"


# ---- the checker ---------------------------------------------------------------------------------------------------------------
def _fmt(pt):
    return "infinity" if pt is None else f"({pt[0] % (1 << 64):#x}.., {pt[1] % (1 << 64):#x}..)"


def check_point(w, want, what):
    """one device point (64 words) against the affine point it must stand for"""
    try:
        p = point_of(w)
        L.check_stored(p, what)
        got = L.affine_of(p)
    except AssertionError as e:
        raise AssertionError(f"{what}: not a stored point: {e or 'ZZ^3 != ZZZ^2'}") from None
    if got != want:
        raise AssertionError(f"{what}: is {_fmt(got)}, expected {_fmt(want)}")


def check_results(words, want):
    """words: (W, c, 64) as the hook returns them; want: W rows of c affine points (points_of_logs over result_logs)"""
    words = np.asarray(words)
    assert words.shape[:2] == (len(want), len(want[0])), (words.shape, len(want), len(want[0]))
    for w, row in enumerate(want):
        for e, pt in enumerate(row):
            check_point(words[w, e], pt, f"window {w}, result {e} ({result_name(e)})")


def check_buckets(words, want, kind="bucket", only=None):
    """words: (W, nb, 64) in logical order (unpack_planes / unpack_entries); want: W rows of nb affine points.  only: iterable of
    (w, i) to look at; a failure names the bucket id i + 1"""
    words = np.asarray(words)
    where = only if only is not None else ((w, i) for w in range(len(want)) for i in range(len(want[w])))
    for w, i in where:
        check_point(words[w, i], want[w][i], f"window {w}, {kind} {i + 1}")


# ---- layouts ------------------------------------------------------------------------------------------------------------------
def to_physical(sets):
    """(W, nb, 64) logical -> (W nb, 64) entry-major at the buckets' positions"""
    sets = np.asarray(sets)
    W, nb, _ = sets.shape
    phys = np.empty_like(sets)
    phys[:, pyr_pos(np.arange(nb), nb)] = sets
    return phys.reshape(W * nb, 64)


def from_physical(entries, W, nb):
    entries = np.asarray(entries).reshape(W, nb, 64)
    return entries[:, pyr_pos(np.arange(nb), nb)]


def planes_of_entries(entries):
    """(n, 64) entry-major -> (16, n, 4) plane-major"""
    n = entries.shape[0]
    return np.ascontiguousarray(entries.reshape(n, 16, 4).transpose(1, 0, 2))


def entries_of_planes(planes):
    n = planes.shape[1]
    return np.ascontiguousarray(planes.transpose(1, 0, 2)).reshape(n, 64)


def pack_planes(sets):
    """(W, nb, 64) logical -> the bucket array as the kernels read it, (16, W nb, 4)"""
    return planes_of_entries(to_physical(sets))


def unpack_planes(planes, W, nb):
    return from_physical(entries_of_planes(np.asarray(planes).reshape(16, W * nb, 4)), W, nb)


# ---- the reduction in plain Python (limb_model adds): what the CPU test holds the checker against -----------------------------
def add_all(points, quad=False):
    """left-to-right sum of limb dicts with limb_model's general add (quad: the four-lane form)"""
    acc = L.x28_infinity()
    for p in points:
        acc = L.g1_28_add_quad(acc, p) if quad else L.g1_28_add(acc, p)
    return acc


def reduce_by_adds(bucket_words):
    """(nb, 64) words in logical order -> (c, 64): S and every U_j by direct summation in logical order"""
    pts = [point_of(w) for w in bucket_words]
    nb = len(pts)
    c = nb.bit_length()
    out = [add_all(pts)]
    for j in range(c - 1):
        out.append(add_all([p for i, p in enumerate(pts) if (i >> j) & 1], quad=bool(j & 1)))
    return np.stack([words_of(p) for p in out])
