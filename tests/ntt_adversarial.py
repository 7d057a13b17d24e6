"""The Fr vectors that drive the transform's lazy reduction to its ceiling (tests/model/ntt_fr_model.py builds them), shared by
tests/test_ntt_fr_model_cpu.py (through the limb model: in contract, equal to the oracle, reach) and
tests/test_gpu_ntt_lazy_bounds.py (through the kernels, every word against the oracle).  Seeds are fixed; everything is built on
first use and kept for the process.  Words are memory words (Montgomery form), as numpy (n, 4) uint64 arrays or as integers."""
import functools
import random

import numpy as np

import ntt_fr_model as N

R = N.R
COSET = random.Random(0xC05E7).randrange(2, R)   # the memory word of the coset generator


def to_array(words):
    return np.array([[(w >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)] for w in words], dtype=np.uint64).reshape(-1, 4)


def to_ints(a):
    return [sum(int(x) << (64 * k) for k, x in enumerate(row)) for row in np.asarray(a, dtype=np.uint64).reshape(-1, 4)]


COSET_ARRAY = to_array([COSET])[0]


def random_array(seed, n):
    """n words below r (the top 64-bit word below r's)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 1 << 64, size=(n, 4), dtype=np.uint64)
    a[:, 3] = rng.integers(0, R >> 192, size=n, dtype=np.uint64)
    return a


def natural(column, log_r):
    """tile row order -> input order"""
    return [column[N.bitrev(j, log_r)] for j in range(1 << log_r)]


@functools.lru_cache(None)
def single(log_r, inverse):
    """canonical words straight into a radix-2^log_r tile (a single pass, or a column of pass 0), input order -> (words, reach)"""
    column, reach = N.adversarial_column(log_r, inverse, N.DirectLoader(), 0xAD00 + 2 * log_r + int(inverse))
    return natural(column, log_r), reach


@functools.lru_cache(None)
def single_coset(log_n):
    """a forward single pass behind the coset pre-scale: the tile's inputs are tight products -> (words, reach)"""
    tr = N.Transform(log_n, coset=COSET)
    column, reach = N.adversarial_column(log_n, False, N.PreScaleLoader(tr), 0xC000 + log_n)
    return natural(column, log_n), reach


# (log_n, allow_wide, batch, knob) -> the multi-pass classes and the inner indices of the planted pass-0 columns: 0, 1, T - 1, the
# last one and some in between (T = columns per tile: 4 up to radix 2^8, 2 for 2^9, 1 for 2^10)
PLANTED = {
    "2^12": dict(log_n=12, wide=False, batch=1, matrix=True, columns=[0, 1, 3, 17, 40, 63]),
    "2^12 two-level table": dict(log_n=12, wide=False, batch=1, matrix=False, columns=[0, 1, 3, 17, 40, 63]),
    "2^16": dict(log_n=16, wide=False, batch=1, matrix=True, columns=[0, 1, 3, 100, 129, 255]),
    "2^17 three passes": dict(log_n=17, wide=False, batch=1, matrix=True, columns=[0, 1, 3, 777, 1024, 2047]),
    "4 x 2^17 wide": dict(log_n=17, wide=True, batch=4, matrix=True, columns=[0, 1, 130, 255]),
    "2^19": dict(log_n=19, wide=True, batch=1, matrix=True, columns=[0, 1, 200, 511]),
    "2^20": dict(log_n=20, wide=True, batch=1, matrix=True, columns=[0, 1, 513, 1023]),
}


def planted(name, inverse):
    """-> (batch * n words as an array: random, with the adversarial column of pass 0's radix planted at the listed inner indices of the
    first and the last transform of the batch; [(transform, inner index)])"""
    c = PLANTED[name]
    tr = N.Transform(c["log_n"], inverse, wide=c["wide"], matrix=c["matrix"])
    n = 1 << c["log_n"]
    a = random_array(0x9F0000 + 2 * c["log_n"] + int(inverse), c["batch"] * n)
    col = to_array(single(tr.r[0], inverse)[0])
    where = [(b, i) for b in sorted({0, c["batch"] - 1}) for i in c["columns"]]
    for b, i in where:
        a[np.array(tr.column_indices(0, 0, i)) + b * n] = col
    return a, where


def last_tile_arrivals(tr, data, k0s):
    """the values the last-pass tiles (k0, 0), k0 in k0s, of a two-pass transform find in memory, tile row order"""
    log_r0, log_r = tr.r[0], tr.plan["last"]["log_r"]
    twv = N.radix_values(log_r0, tr.inverse)
    out = {k0: [0] * (1 << log_r) for k0 in k0s}
    for row in range(1 << log_r):
        i = N.bitrev(row, log_r)
        idx = tr.column_indices(0, 0, i)
        x = [data[idx[N.bitrev(e, log_r0)]] for e in range(1 << log_r0)]
        N.vtile(x, log_r0, twv)
        for k0 in k0s:
            out[k0][row] = N.vmul(x[k0], N.L.v29(tr.factor(0, k0, i)))
    return out


@functools.lru_cache(None)
def last_pass(log_n):
    """A forward two-pass transform with a pre-image aimed at one last-pass tile: the tile of k0 = R0 - 2, the output row of pass 0
    that grows most, so that what arrives is as large as a tight value gets.  Row e of that tile is steered through input 0 of the pass-0
    column bitrev(e).  -> (words as an array, k0, reach, the largest value over the last-pass tiles k0 < 64 of the same random words
    before anything was planted)"""
    tr = N.Transform(log_n)
    log_r = tr.plan["last"]["log_r"]
    k0 = (1 << tr.r[0]) - 2
    a = random_array(0x1A5700 + log_n, 1 << log_n)
    data = to_ints(a)
    twv = N.radix_values(log_r, False)
    baseline = max(N.vtile(list(x), log_r, twv) for x in last_tile_arrivals(tr, data, range(64)).values())
    loader = N.Pass0Loader(tr, data, k0)
    users = [loader.user_index(row) for row in range(1 << log_r)]
    column, reach = N.adversarial_column(log_r, False, loader, 0x1A00 + log_n, words=[data[u] for u in users])
    a[np.array(users)] = to_array(column)
    return a, k0, reach, baseline
