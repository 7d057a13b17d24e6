// kzg_cells_plan.hpp -- the field half of zkp_kzg_verify_cells* (kzg_cells_host.inc, kernels in kzg_cells.hpp) as a host-checkable
// plan: the grouping of a batch of cells by coset and by commitment, the chunks the sums are cut into, every table the kernels
// index and the bytes of a verifier.  Plain C++17 without HIP, so that tests/host/kzg_cells_plan.cpp walks the same tables with g++
// alone over F_65537; under hipcc (ff.hpp included first) the kernels call the same index functions.
//
// n = 2^log_n points, cosets of l = 2^log_l, r = n / l of them; w the root of the transforms of n.  Cell i < N names the commitment
// m_i, the coset k_i (shift x_i = w^(k_i), c_i = x_i^l = (w^l)^(k_i)), l values e_i[j] = f(x_i w_l^j), a proof W_i and a weight
// rho_i.  The batch is accepted iff
//   e( sum rho_i W_i , [s^l]_2 )  ==  e( sum_m (sum_{i: m_i = m} rho_i) C_m  -  [ (sum rho_i I_i)(s) ]_1  +  sum rho_i c_i W_i ,  G_2 )
// with I_i the interpolant of e_i on its coset.  The interpolants need no transform of their own: I_i = F_i mod (X^l - c_i) for any
// F_i of degree < n with the values e_i on coset k_i, and for deg F < n
//   sum_{k<r} (F mod (X^l - rho^k)) = r (F mod X^l),   rho = w^l
// (write F = sum_q X^(q l) F_q with deg F_q < l: F mod (X^l - c) = sum_q c^q F_q, and sum_k rho^(k q) = r for q = 0, else 0 for
// q < r).  Take F_k the polynomial with the values A_k[k + j r] = sum_{i: k_i = k} rho_i e_i[j] on coset k and zero on every other
// coset: F_k mod (X^l - rho^k') is the interpolant sum of coset k for k' = k and 0 otherwise, so with A = sum_k A_k
//   sum_i rho_i I_i = r * (the first l coefficients of the inverse transform of size n of A).
//
// The sums: Fr has no atomic add, and one coset (or one commitment) may hold every cell of a batch.  The cells are therefore sorted
// (stable counting sorts, on the host, from the two host index arrays) by coset and by commitment; every segment of equal keys is
// cut into chunks of at most 2^chunk_log cells; a first kernel sums each chunk in cell order, a second sums the chunks of a segment
// in chunk order.  The order of every addition is fixed by the tables alone.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkp {

#ifdef ZKP_HD
#define ZKP_CELLS_FN ZKP_HD
#else
#define ZKP_CELLS_FN inline
#endif

constexpr unsigned KZG_CELLS_MAX_LOG = 23;        // the opener's range: log_l < log_n <= 23
constexpr unsigned KZG_CELLS_MAX_CHUNK_LOG = 16;  // the bounds of ZKP_KZG_CELLS_CHUNK_LOG (knobs.hpp)
constexpr unsigned KZG_CELLS_CHUNK_LOG = 4;       // the default: profiles/kzg_verify_cells.md
constexpr unsigned KZG_CELLS_THREADS = 256;       // workgroup of every kernel
constexpr uint64_t KZG_CELLS_MAX_COUNT = (uint64_t)1 << 30;  // cells or commitments of a verifier: ids are 32-bit words

inline bool kzg_cells_shape_ok(unsigned log_n, unsigned log_l) { return log_l < log_n && log_n <= KZG_CELLS_MAX_LOG; }

inline uint64_t kzg_cells_min(uint64_t a, uint64_t b) { return a < b ? a : b; }
// the most chunks `cells` cells in at most `segments` segments are cut into: ceil(len / 2^c) <= floor(len / 2^c) + 1 per segment
inline uint64_t kzg_cells_max_chunks(uint64_t cells, uint64_t segments, unsigned chunk_log) {
    return kzg_cells_min(cells, kzg_cells_min(segments, cells) + (cells >> chunk_log));
}

// What the tables of one call are made of, and where each begins in the table (32-bit words).  The table is packed for the call:
// one copy of `words` words carries it to the device.
struct KzgCellsTables {
    uint64_t cells, commits;  // N, M of the call
    uint64_t used;            // U: cosets that at least one cell names
    uint64_t chunks;          // C: chunks of the sort by coset
    uint64_t cchunks;         // CC: chunks of the sort by commitment
    size_t by_coset;          // [N] cell ids, sorted by coset, cells of a coset in batch order
    size_t chunk_start;       // [C + 1] positions in by_coset: chunk q is [chunk_start[q], chunk_start[q + 1])
    size_t used_coset;        // [U] the cosets in use, ascending
    size_t seg_chunk;         // [U + 1] chunk numbers: used coset u owns the chunks [seg_chunk[u], seg_chunk[u + 1])
    size_t cell_coset;        // [N] coset_index as the caller gave it
    size_t by_commit;         // [N] cell ids, sorted by commitment
    size_t cchunk_start;      // [CC + 1] positions in by_commit
    size_t cseg_chunk;        // [M + 1] chunk numbers: commitment m owns [cseg_chunk[m], cseg_chunk[m + 1]), none when no cell names it
    size_t words;             // of the whole table
};

// Byte offsets of the pieces of a verifier's device workspace, sized for max_cells and max_commits, and of its staging buffer
struct KzgCellsSizes {
    uint64_t max_used, max_chunks, max_cchunks;
    size_t table_words;  // the largest table of a call
    size_t a;            // n elements: the vector A, then its inverse transform
    size_t partial;      // max_chunks rows of l elements: the chunk sums
    size_t cpartial;     // max_cchunks elements: the chunk sums of the weights
    size_t interp;       // l elements: the coefficients of sum rho_i I_i (zkp_kzg_verify_cells*; the aggregate entry writes the caller's)
    size_t sc_right;     // max_commits + max_cells elements: [sum rho per commitment ..., rho_i c_i ...]
    size_t sc_left;      // the same count: [0 ..., rho_i ...]
    size_t report;       // two validation reports of 32 bytes: the commitments', the proofs'
    size_t table;        // table_words words
    size_t total;        // of the device workspace
    size_t stage_total;  // the pinned staging buffer: the table as it is copied
    size_t scratch_words;  // host words the sorts count in: max(r, max_commits) + 1
};
inline KzgCellsSizes kzg_cells_sizes(unsigned log_n, unsigned log_l, unsigned chunk_log, uint64_t max_cells, uint64_t max_commits) {
    const size_t n = (size_t)1 << log_n, l = (size_t)1 << log_l, r = n >> log_l;
    KzgCellsSizes s;
    s.max_used = kzg_cells_min(r, max_cells);
    s.max_chunks = kzg_cells_max_chunks(max_cells, r, chunk_log);
    s.max_cchunks = kzg_cells_max_chunks(max_cells, max_commits, chunk_log);
    s.table_words = (size_t)(3 * max_cells + (s.max_chunks + 1) + s.max_used + (s.max_used + 1) + (s.max_cchunks + 1) + (max_commits + 1));
    s.a = 0;
    s.partial = s.a + 32 * n;
    s.cpartial = s.partial + 32 * l * (size_t)s.max_chunks;
    s.interp = s.cpartial + 32 * (size_t)s.max_cchunks;
    s.sc_right = s.interp + 32 * l;
    s.sc_left = s.sc_right + 32 * (size_t)(max_commits + max_cells);
    s.report = s.sc_left + 32 * (size_t)(max_commits + max_cells);
    s.table = s.report + 64;
    s.total = (s.table + 4 * s.table_words + 31) & ~(size_t)31;
    s.stage_total = 4 * s.table_words;
    s.scratch_words = (size_t)(r > max_commits ? r : max_commits) + 1;
    return s;
}

// One stable counting sort with its chunks.  key[i] < keys for i < cells (the caller has checked).  count: keys + 1 words of scratch.
// Writes order[cells], chunk_start[chunks + 1] and, with `compact`, used[U] and seg[U + 1] over the keys in use (else seg[keys + 1]
// over all keys).
inline void kzg_cells_sort(const uint32_t* key, uint64_t cells, uint64_t keys, unsigned chunk_log, bool compact, uint32_t* count,
                           uint32_t* order, uint32_t* chunk_start, uint32_t* used, uint32_t* seg) {
    for (uint64_t k = 0; k <= keys; k++) count[k] = 0;
    for (uint64_t i = 0; i < cells; i++) count[key[i]]++;
    const uint64_t per = (uint64_t)1 << chunk_log;
    uint64_t at = 0, chunks = 0, segs = 0;
    for (uint64_t k = 0; k < keys; k++) {
        const uint64_t len = count[k];
        count[k] = (uint32_t)at;  // from here on: where the next cell of key k goes
        if (compact && !len) continue;
        if (compact) used[segs] = (uint32_t)k;
        seg[segs++] = (uint32_t)chunks;
        for (uint64_t off = 0; off < len; off += per) chunk_start[chunks++] = (uint32_t)(at + off);
        at += len;
    }
    seg[segs] = (uint32_t)chunks;
    chunk_start[chunks] = (uint32_t)at;
    for (uint64_t i = 0; i < cells; i++) order[count[key[i]]++] = (uint32_t)i;
}

// The tables of one call, written to `table` (at least sz.table_words words; the verifier's pinned staging buffer); `scratch`: at
// least sz.scratch_words words.  The caller has checked cells <= max_cells, commits <= max_commits, coset_index[i] < r and
// commit_index[i] < commits.
inline KzgCellsTables kzg_cells_tables(unsigned log_n, unsigned log_l, unsigned chunk_log, const uint32_t* commit_index,
                                       const uint32_t* coset_index, uint64_t cells, uint64_t commits, uint32_t* scratch, uint32_t* table) {
    const uint64_t r = (uint64_t)1 << (log_n - log_l);
    KzgCellsTables t;
    t.cells = cells;
    t.commits = commits;
    // the sizes of the sort by coset are known only once it has counted: count first (cheaply, in scratch), then lay the table out
    for (uint64_t k = 0; k < r; k++) scratch[k] = 0;
    for (uint64_t i = 0; i < cells; i++) scratch[coset_index[i]]++;
    const uint64_t per = (uint64_t)1 << chunk_log;
    t.used = t.chunks = 0;
    for (uint64_t k = 0; k < r; k++)
        if (scratch[k]) t.used++, t.chunks += (scratch[k] + per - 1) >> chunk_log;
    t.by_coset = 0;
    t.chunk_start = t.by_coset + (size_t)cells;
    t.used_coset = t.chunk_start + (size_t)t.chunks + 1;
    t.seg_chunk = t.used_coset + (size_t)t.used;
    t.cell_coset = t.seg_chunk + (size_t)t.used + 1;
    t.by_commit = t.cell_coset + (size_t)cells;
    t.cchunk_start = t.by_commit + (size_t)cells;
    kzg_cells_sort(coset_index, cells, r, chunk_log, true, scratch, table + t.by_coset, table + t.chunk_start, table + t.used_coset,
                   table + t.seg_chunk);
    for (uint64_t i = 0; i < cells; i++) table[t.cell_coset + i] = coset_index[i];
    // the sort by commitment: its chunk count decides where its last piece begins
    for (uint64_t m = 0; m <= commits; m++) scratch[m] = 0;
    for (uint64_t i = 0; i < cells; i++) scratch[commit_index[i]]++;
    t.cchunks = 0;
    for (uint64_t m = 0; m < commits; m++) t.cchunks += (scratch[m] + per - 1) >> chunk_log;
    t.cseg_chunk = t.cchunk_start + (size_t)t.cchunks + 1;
    t.words = t.cseg_chunk + (size_t)commits + 1;
    kzg_cells_sort(commit_index, cells, commits, chunk_log, false, scratch, table + t.by_commit, table + t.cchunk_start, nullptr,
                   table + t.cseg_chunk);
    return t;
}

// ---- the launches of one call, in order (the transform of A is run_ntt<Fr>(a, log_n, 1, inverse) between COMBINE and TAIL) ----
enum KzgCellsStepKind {
    KZG_CELLS_ZERO,       // A <- 0 (n elements): the cosets no cell names stay zero
    KZG_CELLS_AGGREGATE,  // lane t < C l: chunk q = t / l, j = t % l: partial[q l + j] = sum over the cells i of chunk q of rho_i e_i[j]
    KZG_CELLS_COMBINE,    // lane t < U l: u = t / l, j = t % l: A[used[u] + j r] = sum of partial[q l + j] over the chunks q of used coset u
    KZG_CELLS_NTT,        // A: the inverse transform of n
    KZG_CELLS_TAIL,       // lane j < l: interp[j] = r A[j]
    KZG_CELLS_SCALARS,    // lane t < N: proof_scalar[t] = rho_t (w^l)^(k_t); lane N + q, q < CC: cpartial[q] = sum of rho over chunk q
    KZG_CELLS_COMMITS     // lane m < M: commit_weight[m] = sum of cpartial over the chunks of commitment m (zero when it has none)
};
constexpr unsigned KZG_CELLS_STEPS = 7;
struct KzgCellsStep {
    KzgCellsStepKind kind;
    uint64_t lanes;  // of a kernel (0: not a kernel of this file)
};
inline KzgCellsStep kzg_cells_step(unsigned log_l, const KzgCellsTables& t, unsigned i) {
    const uint64_t l = (uint64_t)1 << log_l;
    switch (i) {
    case 0: return {KZG_CELLS_ZERO, 0};
    case 1: return {KZG_CELLS_AGGREGATE, t.chunks << log_l};
    case 2: return {KZG_CELLS_COMBINE, t.used << log_l};
    case 3: return {KZG_CELLS_NTT, 0};
    case 4: return {KZG_CELLS_TAIL, l};
    case 5: return {KZG_CELLS_SCALARS, t.cells + t.cchunks};
    default: return {KZG_CELLS_COMMITS, t.commits};
    }
}

// ---- the index arithmetic of the kernels ----
// element j of cell i in the caller's cell-major evaluations
ZKP_CELLS_FN uint64_t kzg_cells_eval_index(unsigned log_l, uint64_t cell, uint64_t j) { return (cell << log_l) + j; }
// element j of chunk row q
ZKP_CELLS_FN uint64_t kzg_cells_partial_index(unsigned log_l, uint64_t q, uint64_t j) { return (q << log_l) + j; }
// value j of coset k in the natural-order vector of n
ZKP_CELLS_FN uint64_t kzg_cells_a_index(unsigned log_r, uint64_t k, uint64_t j) { return k + (j << log_r); }

}  // namespace zkp
