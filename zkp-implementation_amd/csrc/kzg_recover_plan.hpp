// kzg_recover_plan.hpp -- everything zkp_kzg_recover_cosets* (kzg_recover_host.inc, kernels in kzg_recover.hpp) launches, as a list
// of steps: the padded root count, the leaf launch, every tree level (transform size, batch count, offsets in the workspace), the
// transforms of size r and n, and the bytes of a handle.  Plain C++17 without HIP, so that tests/host/kzg_recover_plan.cpp walks the
// same list with g++ alone over F_65537; under hipcc (ff.hpp included first) the kernels call the same index functions.
//
// n = 2^log_n points, cosets of l = 2^log_l, r = n / l of them; w the root of the transforms of n, rho = w^l.  Coset k < r sits at the
// indices k + j r of a natural-order evaluation vector and is the root set of X^l - rho^k.  M: the m missing cosets.
//   Z(X) = prod_{k in M} (X^l - rho^k) = Zs(X^l),  Zs(Y) = prod_{k in M} (Y - rho^k):  Z(w^i) = Zs(rho^(i mod r)),
//   Z(g w^i) = Zs(g^l rho^(i mod r)) -- r values each, one transform of r (the second with the coset shift g^l).
//   E Z on the domain (0 on missing cosets) -> iNTT_n = the coefficients of f Z (len + m l <= n) -> coset NTT_n with g ->
//   times Z(g w^i)^-1 -> coset iNTT_n = the coefficients of f; a non-zero one at an index >= len: the input was inconsistent.
//
// Zs is built as a product tree.  The m roots are padded to R = 2^root_log with the root 0 (a factor Y), so that every node is monic of
// a power-of-two degree d and is held as its d low coefficients (the leading 1 is implicit); the `pad` = R - m lowest coefficients
// of the final product are zero and are dropped.  A leaf multiplies 2^leaf_log factors in LDS (schoolbook); level j joins pairs of
// degree d = 2^j:  (Y^d + A)(Y^d + B) = Y^2d + (A + B) Y^d + A B, the low 2d coefficients being the cyclic product of size 2d of A and
// B (degree <= 2d - 2: nothing wraps) plus (A + B) Y^d; and Y^d at the k-th root of order 2d is (-1)^k, so in the transformed
// domain  out_k = a_k b_k + (-1)^k (a_k + b_k).  O(R log^2 R) products in all.
//
// A batch (kzg_recover_plan_batch): `polys` rows that miss the same cosets.  Everything up to the inverses of Zs(g^l rho^k) depends on
// M alone and is the single plan's; the n-sized steps take `polys` contiguous rows of vec, and the caller's evaluations may be in
// cell layout (coset k at k l + j), transposed through tiles on the way in (inside the masked multiply) and out (the last step).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkp {

#ifdef ZKP_HD
#define ZKP_RECOVER_FN ZKP_HD
#else
#define ZKP_RECOVER_FN inline
#endif

constexpr unsigned KZG_RECOVER_MAX_LOG = 23;       // the opener's range: log_l < log_n <= 23
constexpr unsigned KZG_RECOVER_MAX_LEAF_LOG = 8;   // a leaf is one workgroup of at most 256 lanes, one per coefficient
constexpr unsigned KZG_RECOVER_LEAF_LOG = 5;       // the default, ZKP_KZG_RECOVER_LEAF_LOG otherwise: profiles/kzg_recover.md
constexpr unsigned KZG_RECOVER_THREADS = 256;      // workgroup of the pointwise kernels
constexpr unsigned KZG_RECOVER_INV_CHUNK = 4;      // values one lane of the inversion pass inverts with one field inversion
constexpr uint32_t KZG_RECOVER_PAD_ROOT = 0xffffffffu;  // entry of the root list that stands for the root 0
constexpr uint64_t KZG_RECOVER_NTT_BATCH = 32768;  // a batched transform takes at most 65535 rows: the tree levels go in pieces of this
constexpr uint64_t KZG_RECOVER_MAX_POLYS = 4096;   // polynomials of one batch call (the batched opener's range)
#ifndef ZKP_KZG_RECOVER_ROWS
#define ZKP_KZG_RECOVER_ROWS 4  // (a variant build may state another: build.py -DZKP_KZG_RECOVER_ROWS=...)
#endif
constexpr unsigned KZG_RECOVER_ROWS = ZKP_KZG_RECOVER_ROWS;  // rows of a batch one lane of a pointwise pass takes: profiles/kzg_recover_batch.md
constexpr unsigned KZG_RECOVER_TILE_LOG = 8;       // a tile of the cell-layout transposition: KZG_RECOVER_THREADS elements
constexpr int KZG_RECOVER_NATURAL = 0, KZG_RECOVER_CELLS = 1;  // ZKP_KZG_LAYOUT_*

inline bool kzg_recover_shape_ok(unsigned log_n, unsigned log_l) { return log_l < log_n && log_n <= KZG_RECOVER_MAX_LOG; }
inline bool kzg_recoverable(unsigned log_n, unsigned log_l, uint64_t m, uint64_t len) {
    const uint64_t r = (uint64_t)1 << (log_n - log_l);
    return m <= r && ((r - m) << log_l) >= len;
}

// Byte offsets of the pieces of a handle's device workspace, sized for the worst case m = r - 1 (R = r), and its pinned staging buffer
struct KzgRecoverSizes {
    size_t vec;      // n elements: E Z, then everything up to the coefficients of f
    size_t zs0;      // r: the coefficients of Zs, then Zs(rho^i)
    size_t zs1;      // r: the same, then Zs(g^l rho^i), then the inverses
    size_t x;        // R <= r: the nodes of a tree level, d low coefficients each
    size_t w;        // 2R: the same padded to 2d each, transformed
    size_t roots;    // R words: the missing indices, KZG_RECOVER_PAD_ROOT behind them
    size_t mask;     // r bytes: present
    size_t total;    // of the device workspace
    size_t stage_roots, stage_mask, stage_total;  // the pinned staging buffer: the root list and the mask as they are copied
};
inline KzgRecoverSizes kzg_recover_sizes(unsigned log_n, unsigned log_l) {
    const size_t n = (size_t)1 << log_n, r = n >> log_l;
    KzgRecoverSizes s;
    s.vec = 0;
    s.zs0 = s.vec + 32 * n;
    s.zs1 = s.zs0 + 32 * r;
    s.x = s.zs1 + 32 * r;
    s.w = s.x + 32 * r;
    s.roots = s.w + 64 * r;
    s.mask = s.roots + 4 * r;
    s.total = (s.mask + r + 31) & ~(size_t)31;
    s.stage_roots = 0;
    s.stage_mask = 4 * r;
    s.stage_total = 5 * r;
    return s;
}

// The same for a handle of up to max_polys polynomials per call: only vec grows, everything behind it depends on `present` alone
// and stays single.  (The cell-layout output is transformed in vec itself, in place behind the tail: no second vector.)
inline KzgRecoverSizes kzg_recover_sizes_batch(unsigned log_n, unsigned log_l, uint64_t max_polys) {
    KzgRecoverSizes s = kzg_recover_sizes(log_n, log_l);
    const size_t grow = 32 * ((size_t)1 << log_n) * (size_t)(max_polys - 1);
    s.zs0 += grow;
    s.zs1 += grow;
    s.x += grow;
    s.w += grow;
    s.roots += grow;
    s.mask += grow;
    s.total += grow;
    return s;
}

enum KzgRecoverStepKind {
    KZG_RECOVER_LEAF,      // roots -> x: `batch` workgroups of `lanes` lanes, 2^log factors each
    KZG_RECOVER_PAD,       // x -> w: `batch` nodes of d = 2^log low coefficients, zero-padded to 2d
    KZG_RECOVER_TREE_FWD,  // w: `batch` transforms of 2^log
    KZG_RECOVER_PAIR,      // w -> x: `batch` products of 2^log values, out_k = a_k b_k + (-1)^k (a_k + b_k)
    KZG_RECOVER_TREE_INV,  // x: `batch` inverse transforms of 2^log
    KZG_RECOVER_ZS,        // x -> zs0, zs1: coefficient k of Zs is x[pad + k] below m, 1 at m, 0 behind
    KZG_RECOVER_ZS_FWD,    // zs0: the transform of r
    KZG_RECOVER_ZS_SHIFT,  // zs1: the transform of r with the coset shift g^l
    KZG_RECOVER_MUL,       // evaluations, mask, zs0 -> vec (n lanes)
    KZG_RECOVER_COPY,      // m = 0: evaluations -> vec through the inverse transform of n
    KZG_RECOVER_N_INV,     // vec: the inverse transform of n
    KZG_RECOVER_N_SHIFT,   // vec: the transform of n with the coset shift g
    KZG_RECOVER_INV,       // zs1: r inversions, `lanes` lanes of KZG_RECOVER_INV_CHUNK -- one chain of ~380 dependent products per lane,
                           // 0.4 ms whatever r: it is stated right behind ZS_SHIFT and launched on the handle's side stream, beside
                           // the steps up to DIV, which nothing of it touches (they use zs0 and vec)
    KZG_RECOVER_DIV,       // vec times zs1[i mod r] (n lanes), once the inversions are done
    KZG_RECOVER_N_UNSHIFT, // vec: the inverse transform of n with the coset shift g
    KZG_RECOVER_TAIL,      // vec -> the caller's coefficients (and zero-padded evaluations), the inconsistency word (n lanes)
    KZG_RECOVER_EVALS      // the caller's evaluations, where asked for: the transform of n of the zero-padded coefficients
};
// A batch plan in cell layout only, its last step: vec (where TAIL and EVALS then work) -> the caller's evaluations, transposed.  It
// stands beside the enumeration (whose range holds it), not in it: a walk of the single plan never meets it and need not name it.
constexpr KzgRecoverStepKind KZG_RECOVER_CELLS_OUT = static_cast<KzgRecoverStepKind>(KZG_RECOVER_EVALS + 1);
struct KzgRecoverStep {
    KzgRecoverStepKind kind;
    unsigned log;     // of a transform's size, of a leaf's factors or of a node's d
    uint64_t batch;   // transforms, workgroups or nodes
    uint64_t lanes;   // of a kernel (per workgroup for the leaves)
    size_t in, out;   // byte offsets in the workspace (the caller's buffers: 0)
    size_t in_bytes, out_bytes;
};

struct KzgRecoverPlan {
    unsigned log_n, log_l, log_r, leaf_log;
    uint64_t m;
    unsigned root_log;   // R = 2^root_log >= m padded roots (m = 0: no tree)
    uint64_t roots, pad; // R, R - m
    unsigned leaf_roots_log;  // min(leaf_log, root_log): factors of a leaf
    uint64_t leaves;
    unsigned levels;     // root_log - leaf_roots_log
    unsigned steps;
    KzgRecoverSizes sz;
    uint64_t polys;      // rows of the call (the single entries: 1)
    int layout;          // of the caller's evaluations, in and out: KZG_RECOVER_NATURAL or KZG_RECOVER_CELLS
};
inline KzgRecoverPlan kzg_recover_plan(unsigned log_n, unsigned log_l, unsigned leaf_log, uint64_t m) {
    KzgRecoverPlan p;
    p.log_n = log_n;
    p.log_l = log_l;
    p.log_r = log_n - log_l;
    p.leaf_log = leaf_log;
    p.m = m;
    p.root_log = 0;
    while (((uint64_t)1 << p.root_log) < m) p.root_log++;
    p.roots = m ? (uint64_t)1 << p.root_log : 0;
    p.pad = p.roots - m;
    p.leaf_roots_log = leaf_log < p.root_log ? leaf_log : p.root_log;
    p.leaves = m ? p.roots >> p.leaf_roots_log : 0;
    p.levels = m ? p.root_log - p.leaf_roots_log : 0;
    p.steps = m ? 1 + 4 * p.levels + 11 : 3;
    p.sz = kzg_recover_sizes(log_n, log_l);
    p.polys = 1;
    p.layout = KZG_RECOVER_NATURAL;
    return p;
}
// A call of `polys` <= max_polys rows in `layout` on a handle made for max_polys: the steps up to the values of Zs are the single
// plan's; the n-sized steps take `polys` rows, and the cell layout adds KZG_RECOVER_CELLS_OUT
inline KzgRecoverPlan kzg_recover_plan_batch(unsigned log_n, unsigned log_l, unsigned leaf_log, uint64_t m, uint64_t polys, int layout,
                                             uint64_t max_polys) {
    KzgRecoverPlan p = kzg_recover_plan(log_n, log_l, leaf_log, m);
    p.sz = kzg_recover_sizes_batch(log_n, log_l, max_polys);
    p.polys = polys;
    p.layout = layout;
    if (layout == KZG_RECOVER_CELLS) p.steps++;
    return p;
}
// lanes of a pointwise pass over `polys` rows of n: a lane takes one index of up to KZG_RECOVER_ROWS rows
inline uint64_t kzg_recover_row_groups(uint64_t polys) { return (polys + KZG_RECOVER_ROWS - 1) / KZG_RECOVER_ROWS; }

// Step i < p.steps, in the order the driver launches them
inline KzgRecoverStep kzg_recover_step(const KzgRecoverPlan& p, unsigned i) {
    const uint64_t n = (uint64_t)1 << p.log_n, r = (uint64_t)1 << p.log_r, R = p.roots;
    const KzgRecoverSizes& z = p.sz;
    KzgRecoverStep s = {KZG_RECOVER_TAIL, 0, 1, 0, 0, 0, 0, 0};
    auto set = [&](KzgRecoverStepKind kind, unsigned log, uint64_t batch, uint64_t lanes, size_t in, size_t in_bytes, size_t out, size_t out_bytes) {
        s = KzgRecoverStep{kind, log, batch, lanes, in, out, in_bytes, out_bytes};
    };
    // the n-sized steps: B rows, N bytes of vec, L lanes of a pointwise pass; in cell layout the tail pads in place and the
    // evaluations are transformed in vec
    const uint64_t B = p.polys, L = n * kzg_recover_row_groups(B);
    const size_t N = 32 * n * (size_t)B;
    const bool cells = p.layout == KZG_RECOVER_CELLS;
    if (!p.m) {
        if (i == 0) set(KZG_RECOVER_COPY, p.log_n, B, cells ? L : 0, 0, 0, z.vec, N);
        else if (i == 1) set(KZG_RECOVER_TAIL, 0, B, L, z.vec, N, cells ? z.vec : 0, cells ? N : 0);
        else if (i == 2) set(KZG_RECOVER_EVALS, p.log_n, B, 0, cells ? z.vec : 0, cells ? N : 0, cells ? z.vec : 0, cells ? N : 0);
        else set(KZG_RECOVER_CELLS_OUT, 0, B, L, z.vec, N, 0, 0);
        return s;
    }
    if (i == 0) {
        const uint64_t per = (uint64_t)1 << p.leaf_roots_log;
        set(KZG_RECOVER_LEAF, p.leaf_roots_log, p.leaves, per < 64 ? 64 : per, z.roots, 4 * R, z.x, 32 * R);
        return s;
    }
    i -= 1;
    if (i < 4 * p.levels) {
        const unsigned log_d = p.leaf_roots_log + i / 4;
        const uint64_t nodes = R >> log_d;
        switch (i % 4) {
        case 0: set(KZG_RECOVER_PAD, log_d, nodes, 2 * R, z.x, 32 * R, z.w, 64 * R); break;
        case 1: set(KZG_RECOVER_TREE_FWD, log_d + 1, nodes, 0, z.w, 64 * R, z.w, 64 * R); break;
        case 2: set(KZG_RECOVER_PAIR, log_d + 1, nodes / 2, R, z.w, 64 * R, z.x, 32 * R); break;
        default: set(KZG_RECOVER_TREE_INV, log_d + 1, nodes / 2, 0, z.x, 32 * R, z.x, 32 * R); break;
        }
        return s;
    }
    i -= 4 * p.levels;
    switch (i) {
    case 0: set(KZG_RECOVER_ZS, 0, 1, r, z.x, 32 * R, z.zs0, 64 * r); break;  // (zs1 follows zs0)
    case 1: set(KZG_RECOVER_ZS_FWD, p.log_r, 1, 0, z.zs0, 32 * r, z.zs0, 32 * r); break;
    case 2: set(KZG_RECOVER_ZS_SHIFT, p.log_r, 1, 0, z.zs1, 32 * r, z.zs1, 32 * r); break;
    case 3: set(KZG_RECOVER_INV, 0, 1, (r + KZG_RECOVER_INV_CHUNK - 1) / KZG_RECOVER_INV_CHUNK, z.zs1, 32 * r, z.zs1, 32 * r); break;
    case 4: set(KZG_RECOVER_MUL, 0, B, L, z.zs0, 32 * r, z.vec, N); break;
    case 5: set(KZG_RECOVER_N_INV, p.log_n, B, 0, z.vec, N, z.vec, N); break;
    case 6: set(KZG_RECOVER_N_SHIFT, p.log_n, B, 0, z.vec, N, z.vec, N); break;
    case 7: set(KZG_RECOVER_DIV, 0, B, L, z.zs1, 32 * r, z.vec, N); break;
    case 8: set(KZG_RECOVER_N_UNSHIFT, p.log_n, B, 0, z.vec, N, z.vec, N); break;
    case 9: set(KZG_RECOVER_TAIL, 0, B, L, z.vec, N, cells ? z.vec : 0, cells ? N : 0); break;
    case 10: set(KZG_RECOVER_EVALS, p.log_n, B, 0, cells ? z.vec : 0, cells ? N : 0, cells ? z.vec : 0, cells ? N : 0); break;
    default: set(KZG_RECOVER_CELLS_OUT, 0, B, L, z.vec, N, 0, 0); break;
    }
    return s;
}

// ---- the index arithmetic of the kernels ----
// entry j < R of the root list: missing index j below m, the pad root behind
// leaf q takes the entries [q 2^leaf_roots_log, (q + 1) 2^leaf_roots_log) and writes as many coefficients at the same indices of x

// KZG_RECOVER_PAD, lane i < 2R: w[i] = x[kzg_recover_pad_source(log_d, i)], zero where that is negative
ZKP_RECOVER_FN int64_t kzg_recover_pad_source(unsigned log_d, uint64_t i) {
    const uint64_t d = (uint64_t)1 << log_d, k = i & (2 * d - 1);
    return k < d ? (int64_t)(((i >> (log_d + 1)) << log_d) + k) : -1;
}
// KZG_RECOVER_PAIR, lane i < R of a level whose transforms have 2^log_2d values: x[i] = w[a] w[b] + (-1)^i (w[a] + w[b])
struct KzgRecoverPair {
    uint64_t a, b;
    bool minus;
};
ZKP_RECOVER_FN KzgRecoverPair kzg_recover_pair(unsigned log_2d, uint64_t i) {
    const uint64_t k = i & (((uint64_t)1 << log_2d) - 1);
    KzgRecoverPair p;
    p.a = 2 * (i - k) + k;
    p.b = p.a + ((uint64_t)1 << log_2d);
    p.minus = (k & 1) != 0;
    return p;
}
// KZG_RECOVER_INV: lane t < lanes inverts the values t + c lanes, c < KZG_RECOVER_INV_CHUNK, that are below r
ZKP_RECOVER_FN uint64_t kzg_recover_inv_index(uint64_t lanes, uint64_t t, unsigned c) { return t + (uint64_t)c * lanes; }


// ---- a batch: rows and the two layouts of the caller's evaluations ----
// Natural index i < n of row p  <->  offset (in elements) in a buffer of rows of n.  Natural: value j of coset k at k + j r; cells:
// at k l + j, a row being r cells of l contiguous values (what zkp_kzg_verify_cells takes).
ZKP_RECOVER_FN uint64_t kzg_recover_offset(int layout, unsigned log_n, unsigned log_l, uint64_t p, uint64_t i) {
    const unsigned log_r = log_n - log_l;
    const uint64_t k = i & (((uint64_t)1 << log_r) - 1), j = i >> log_r;
    return (p << log_n) + (layout == KZG_RECOVER_CELLS ? (k << log_l) + j : i);
}
struct KzgRecoverRowIndex {
    uint64_t p, i;
};
ZKP_RECOVER_FN KzgRecoverRowIndex kzg_recover_index(int layout, unsigned log_n, unsigned log_l, uint64_t off) {
    const unsigned log_r = log_n - log_l;
    const uint64_t e = off & (((uint64_t)1 << log_n) - 1);
    KzgRecoverRowIndex x;
    x.p = off >> log_n;
    x.i = layout == KZG_RECOVER_CELLS ? (e >> log_l) + ((e & (((uint64_t)1 << log_l) - 1)) << log_r) : e;
    return x;
}
// The transposition between the layouts goes through tiles of 2^tk_log cosets by 2^tj_log values, at most KZG_RECOVER_THREADS
// elements, one per lane: on the cell side a lane's t counts j first (runs of 2^tj_log contiguous elements), on the natural side k
// first (runs of 2^tk_log), so that both the global read and the global write of a workgroup are contiguous runs -- 512 bytes each
// where l and r are at least 16.  A tile sits in LDS limb-major, element (kk, jj) at slot kk (2^tj_log + 1) + jj of each limb plane:
// the odd row length spreads the k-first reads over the banks.
struct KzgRecoverTile {
    unsigned tk_log, tj_log;
};
ZKP_RECOVER_FN KzgRecoverTile kzg_recover_tile(unsigned log_n, unsigned log_l) {
    const unsigned log_r = log_n - log_l, half = KZG_RECOVER_TILE_LOG / 2;
    KzgRecoverTile t;
    t.tk_log = log_r < half ? log_r : half;
    t.tj_log = log_l < KZG_RECOVER_TILE_LOG - t.tk_log ? log_l : KZG_RECOVER_TILE_LOG - t.tk_log;
    t.tk_log = log_r < KZG_RECOVER_TILE_LOG - t.tj_log ? log_r : KZG_RECOVER_TILE_LOG - t.tj_log;
    return t;
}
ZKP_RECOVER_FN uint64_t kzg_recover_tiles(unsigned log_n, unsigned log_l) {  // of one row
    const KzgRecoverTile t = kzg_recover_tile(log_n, log_l);
    return (uint64_t)1 << (log_n - t.tk_log - t.tj_log);
}
// Lane t < 2^(tk_log + tj_log) of tile q: the coset k and the value j it takes on the cell side and on the natural side, and the
// LDS slot of element (k, j) of the tile
struct KzgRecoverTileAt {
    uint64_t k, j;
    uint32_t slot;
};
ZKP_RECOVER_FN KzgRecoverTileAt kzg_recover_tile_at(unsigned log_n, unsigned log_l, uint64_t q, uint32_t t, bool cell_side) {
    const KzgRecoverTile tl = kzg_recover_tile(log_n, log_l);
    const unsigned log_r = log_n - log_l, kt_log = log_r - tl.tk_log;  // tiles along k
    const uint32_t kk = cell_side ? t >> tl.tj_log : t & ((1u << tl.tk_log) - 1);
    const uint32_t jj = cell_side ? t & ((1u << tl.tj_log) - 1) : t >> tl.tk_log;
    KzgRecoverTileAt a;
    a.k = ((q & (((uint64_t)1 << kt_log) - 1)) << tl.tk_log) + kk;
    a.j = ((q >> kt_log) << tl.tj_log) + jj;
    a.slot = kk * ((1u << tl.tj_log) + 1) + jj;
    return a;
}
constexpr uint32_t KZG_RECOVER_TILE_SLOTS = 2u << KZG_RECOVER_TILE_LOG;  // >= 2^tk_log (2^tj_log + 1) for every tile

}  // namespace zkp
