// kzg_evals_plan.hpp -- zkp_kzg_commit_evals_batch* and zkp_kzg_open_evals_batch* (kzg_evals_host.inc, kernels in kzg_evals.hpp) as a
// host-checkable plan: every index, size and grid of the field half, the groups of the MSMs and the bytes of an opener.  Plain C++17
// without HIP, so that tests/host/kzg_evals_plan.cpp walks the same functions with g++ alone over F_65537; under hipcc (ff.hpp
// included first) the kernels call the same index functions.
//
// A row holds the n = 2^log_n values f_i = f(w^e(i)) of a polynomial of degree < n, e(i) = i (natural order) or bitrev(i) (the
// order blobs are stored in).  The opening at z needs no transform.  With d_i = w^e(i) - z:
//   f(z) = (1 - z^n) / n * sum_i f_i w^e(i) / d_i                         (barycentric form on the roots of unity)
//   q_e(i) = (f_i - f(z)) / d_i                                          (the values of the quotient f - f(z) / (X - z) on the domain)
// and the proof is the MSM of q, in natural order, over the Lagrange-basis SRS.  When z = w^m is in the domain (at most one d of a
// row is zero) f(z) = f at w^m, the other q are as above, and
//   q_m = -w^(-m) sum_{j != m} q_j w^j
// (q(w^m) = f'(w^m), L_j'(w^m) = w^(j-m) / (w^m - w^j) for j != m, and sum_j L_j' = 0 gives L_m'(w^m) = -sum_{j != m} L_j'(w^m)).
//
// The n P inversions are Montgomery's trick in two levels: a lane multiplies its KZG_EVALS_CHUNK denominators, the KZG_EVALS_THREADS
// lane products of a workgroup are multiplied up a binary tree in LDS, ONE lane inverts the root, and the inverses come back down
// the tree and through the chunk.  A zero denominator is replaced by 1 by the lane that meets it, which also stores m in the row's
// word (preset to KZG_EVALS_NONE by the first step; one lane at most writes it).
//
// Rows shorter than a workgroup's span run SHORT workgroups: one workgroup per row, its lanes beyond the row idle (they hold 1).  A
// workgroup therefore never takes elements of two rows, whatever n.
//
// The sums (Fr has no atomic add): a workgroup sums its terms up the same tree and writes one partial per (row, workgroup); a
// finishing workgroup per row sums the row's partials in a fixed order -- lane t takes the partials t, t + KZG_EVALS_THREADS, ...,
// then the tree.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkp {

#ifdef ZKP_HD
#define ZKP_EVALS_FN ZKP_HD
#else
#define ZKP_EVALS_FN inline
#endif

constexpr unsigned KZG_EVALS_MIN_LOG = 1, KZG_EVALS_MAX_LOG = 24;
constexpr uint64_t KZG_EVALS_MAX_POLYS = 4096;
constexpr unsigned KZG_EVALS_THREADS = 256;     // workgroup of every kernel
constexpr unsigned KZG_EVALS_THREADS_LOG = 8;
constexpr unsigned KZG_EVALS_CHUNK = 4;         // denominators a lane multiplies before the tree (written out in the kernel)
constexpr unsigned KZG_EVALS_SPAN_LOG = 10;     // elements a workgroup inverts together: THREADS * CHUNK
constexpr uint32_t KZG_EVALS_NONE = 0xffffffffu;  // a row's word: z is not in the domain
constexpr int KZG_EVALS_NATURAL = 0, KZG_EVALS_BITREV = 1;
constexpr int KZG_EVALS_INVERSE = 0;  // the default of ZKP_KZG_EVALS_INVERSE (0: division steps, 1: the Fermat power): profiles/kzg_open_evals.md
constexpr unsigned KZG_EVALS_MSM_GROUP = 64, KZG_EVALS_MSM_GROUP_SPLIT = 32;  // rows of one msm_partial_batch: MSM_MAX_BATCH, and half of
                                                                              // it over an endomorphism-split handle (two bucket sets per row)
static_assert(KZG_EVALS_THREADS == 1u << KZG_EVALS_THREADS_LOG && KZG_EVALS_THREADS * KZG_EVALS_CHUNK == 1u << KZG_EVALS_SPAN_LOG,
              "the span of a workgroup");

inline bool kzg_evals_shape_ok(unsigned log_n) { return log_n >= KZG_EVALS_MIN_LOG && log_n <= KZG_EVALS_MAX_LOG; }

// bitrev(i) over log_n bits, 1 <= log_n <= 32
ZKP_EVALS_FN uint32_t kzg_evals_bitrev(unsigned log_n, uint32_t i) {
    uint32_t x = i;
    x = ((x >> 1) & 0x55555555u) | ((x & 0x55555555u) << 1);
    x = ((x >> 2) & 0x33333333u) | ((x & 0x33333333u) << 2);
    x = ((x >> 4) & 0x0f0f0f0fu) | ((x & 0x0f0f0f0fu) << 4);
    x = ((x >> 8) & 0x00ff00ffu) | ((x & 0x00ff00ffu) << 8);
    x = (x >> 16) | (x << 16);
    return x >> (32 - log_n);
}
// the exponent of the root whose value stands at position i of a row, and the position the value at w^e stands at (both orders
// are involutions)
ZKP_EVALS_FN uint32_t kzg_evals_exponent(int order, unsigned log_n, uint32_t i) { return order == KZG_EVALS_BITREV ? kzg_evals_bitrev(log_n, i) : i; }
ZKP_EVALS_FN uint32_t kzg_evals_position(int order, unsigned log_n, uint32_t e) { return kzg_evals_exponent(order, log_n, e); }

// ---- the geometry of the workgroups over a row ----
struct KzgEvalsGeom {
    uint32_t wg_elems;  // elements of a row one workgroup takes: min(n, 2^SPAN_LOG)
    uint32_t blocks;    // workgroups per row (grid.x; grid.y is the row): n / wg_elems
    uint32_t lanes;     // lanes of a workgroup that hold elements: max(wg_elems / CHUNK, 1); the others idle
};
ZKP_EVALS_FN KzgEvalsGeom kzg_evals_geom(unsigned log_n) {
    KzgEvalsGeom g;
    g.wg_elems = 1u << (log_n < KZG_EVALS_SPAN_LOG ? log_n : KZG_EVALS_SPAN_LOG);
    g.blocks = 1u << (log_n < KZG_EVALS_SPAN_LOG ? 0 : log_n - KZG_EVALS_SPAN_LOG);
    g.lanes = g.wg_elems >= KZG_EVALS_CHUNK ? g.wg_elems / KZG_EVALS_CHUNK : 1;
    return g;
}
// Position in the row of element k < CHUNK of lane t of workgroup b, or KZG_EVALS_NONE when the lane holds no such element.
// Consecutive lanes take consecutive positions (coalesced); the elements of a lane are `lanes` apart.
ZKP_EVALS_FN uint32_t kzg_evals_element(const KzgEvalsGeom& g, uint32_t b, uint32_t t, uint32_t k) {
    if (t >= g.lanes) return KZG_EVALS_NONE;
    const uint32_t j = t + k * g.lanes;
    return j < g.wg_elems ? b * g.wg_elems + j : KZG_EVALS_NONE;
}
// the partial sum of workgroup b of row p
ZKP_EVALS_FN uint64_t kzg_evals_partial_index(const KzgEvalsGeom& g, uint64_t p, uint32_t b) { return p * g.blocks + b; }
// element at position/exponent j of row p
ZKP_EVALS_FN uint64_t kzg_evals_row_index(unsigned log_n, uint64_t p, uint32_t j) { return (p << log_n) + j; }

// ---- the tree in LDS: a heap of 2 THREADS nodes, node 1 the root, the leaf of lane t at THREADS + t ----
ZKP_EVALS_FN uint32_t kzg_evals_leaf(uint32_t t) { return KZG_EVALS_THREADS + t; }

// ---- the launches of the field half, in order ----
enum KzgEvalsStepKind {
    KZG_EVALS_PRESET,   // the rows' words <- KZG_EVALS_NONE (a fill of P words)
    KZG_EVALS_INVERT,   // grid (blocks, P): d and 1/d of every element, the word of a row whose z is in the domain, the partials of y
    KZG_EVALS_Y,        // grid (1, P): y_p from the partials, or f at w^m
    KZG_EVALS_QUOTIENT, // grid (blocks, P): q in natural order except q_m, and the partials of q_m for a row with m set
    KZG_EVALS_QM        // grid (1, P): q_m of the rows with m set
};
constexpr unsigned KZG_EVALS_STEPS = 5;
struct KzgEvalsStep {
    KzgEvalsStepKind kind;
    uint32_t grid_x, grid_y;  // workgroups of KZG_EVALS_THREADS lanes (0: not a kernel)
};
inline KzgEvalsStep kzg_evals_step(unsigned log_n, uint64_t polys, unsigned i) {
    const KzgEvalsGeom g = kzg_evals_geom(log_n);
    switch (i) {
    case 0: return {KZG_EVALS_PRESET, 0, 0};
    case 1: return {KZG_EVALS_INVERT, g.blocks, (uint32_t)polys};
    case 2: return {KZG_EVALS_Y, 1, (uint32_t)polys};
    case 3: return {KZG_EVALS_QUOTIENT, g.blocks, (uint32_t)polys};
    default: return {KZG_EVALS_QM, 1, (uint32_t)polys};
    }
}

// ---- the MSMs: rows [first, first + count) of group k ----
struct KzgEvalsGroup {
    uint64_t first, count;
};
inline uint64_t kzg_evals_group_rows(bool split) { return split ? KZG_EVALS_MSM_GROUP_SPLIT : KZG_EVALS_MSM_GROUP; }
inline uint64_t kzg_evals_groups(uint64_t polys, bool split) { return (polys + kzg_evals_group_rows(split) - 1) / kzg_evals_group_rows(split); }
inline KzgEvalsGroup kzg_evals_group(uint64_t polys, bool split, uint64_t k) {
    const uint64_t per = kzg_evals_group_rows(split), first = k * per;
    return {first, polys - first < per ? polys - first : per};
}

// ---- the device workspace of an opener made for max_polys rows (byte offsets; every piece starts on a multiple of 32) ----
struct KzgEvalsSizes {
    size_t roots;     // n elements: w^j, j < n
    size_t dinv;      // max_polys rows of n: 1 / d by POSITION
    size_t rows;      // max_polys rows of n: the quotients in natural order (zkp_kzg_open_evals_batch*), or the rows of a
                      // bit-reversed handle gathered into natural order (zkp_kzg_commit_evals_batch*)
    size_t partial;   // max_polys x blocks elements: the partial sums of y
    size_t partial2;  // the same count: the partial sums of q_m
    size_t y;         // max_polys elements
    size_t hit;       // max_polys words
    size_t total;
};
inline KzgEvalsSizes kzg_evals_sizes(unsigned log_n, uint64_t max_polys) {
    const size_t n = (size_t)1 << log_n, P = (size_t)max_polys, blocks = kzg_evals_geom(log_n).blocks;
    KzgEvalsSizes s;
    s.roots = 0;
    s.dinv = s.roots + 32 * n;
    s.rows = s.dinv + 32 * n * P;
    s.partial = s.rows + 32 * n * P;
    s.partial2 = s.partial + 32 * blocks * P;
    s.y = s.partial2 + 32 * blocks * P;
    s.hit = s.y + 32 * P;
    s.total = (s.hit + 4 * P + 31) & ~(size_t)31;
    return s;
}

}  // namespace zkp
