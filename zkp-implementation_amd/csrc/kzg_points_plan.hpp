// kzg_points_plan.hpp -- the field half of zkp_kzg_verify_points* (kzg_points_host.inc, kernels in kzg_points.hpp) as a host-checkable
// plan: the grouping of a batch of point openings by commitment, every table the kernels index, the launches of a call and the bytes
// of a verifier.  Plain C++17 without HIP, so that tests/host/kzg_points_plan.cpp walks the same tables with g++ alone over F_65537.
//
// Opening i < N claims f_m(i)(z_i) = y_i with the proof W_i = [(f_m(i) - y_i) / (X - z_i)](s) and carries the weight r_i; m(i) =
// commit_index[i] < M, or i itself when the call gives no index (then M = N).  From (f - y)(s) = (s - z) q(s), weighted and summed,
//   e( sum_m (sum_{i: m(i) = m} r_i) C_m  +  sum_i (r_i z_i) W_i  -  (sum_i r_i y_i) G ,  G_2 )  ==  e( sum_i r_i W_i , [s]_2 ).
// Both sides are MSMs over the one point vector [C_0 .. C_(M-1), W_0 .. W_(N-1), G] of M + N + 1 points:
//   right scalars  [ sum r per commitment ... | r_i z_i ... | -sum r_i y_i ]      left scalars  [ 0 ... | r_i ... | 0 ]
// so the generator term rides in the same pass as one more point and no value comes back to the host before the two sums.
//
// The sums: Fr has no atomic add.  sum r_i y_i goes up a tree in LDS per workgroup and a last workgroup adds the workgroups' sums.
// The weights of a commitment are summed as the cell verifier sums them (kzg_cells_plan.hpp): the openings are sorted by commitment
// with kzg_cells_sort, every segment is cut into chunks of at most 2^chunk_log openings (ZKP_KZG_CELLS_CHUNK_LOG), one lane sums a
// chunk, then one lane per commitment sums its chunks (the cell verifier's own kernel).  With no index the sum of commitment i is
// r_i: the scalars kernel writes it.  Every sum is exact in Fr, so no output word depends on the chunking.
#pragma once
#include "kzg_cells_plan.hpp"

namespace zkp {

// the openings of a workgroup of the scalars kernel, and the workgroups that `openings` openings take
inline uint64_t kzg_points_blocks(uint64_t openings) { return (openings + KZG_CELLS_THREADS - 1) / KZG_CELLS_THREADS; }

// The tables of one call and where each begins in the packed table (32-bit words); none with the identity index
struct KzgPointsTables {
    uint64_t openings, commits;  // N, M of the call
    bool identity;               // no index: m(i) = i
    uint64_t cchunks;            // CC: chunks of the sort by commitment (0 with the identity index)
    size_t by_commit;            // [N] opening ids, sorted by commitment, openings of a commitment in batch order
    size_t cchunk_start;         // [CC + 1] positions in by_commit
    size_t cseg_chunk;           // [M + 1] chunk numbers: commitment m owns [cseg_chunk[m], cseg_chunk[m + 1]), none when nothing names it
    size_t words;                // of the whole table
};

// Byte offsets of the pieces of a verifier's device workspace, sized for max_openings and max_commits, and of its staging buffer
struct KzgPointsSizes {
    uint64_t max_cchunks, max_blocks;
    size_t table_words;    // the largest table of a call
    size_t cpartial;       // max_cchunks elements: the chunk sums of the weights
    size_t ypartial;       // max_blocks elements: the workgroups' sums of r_i y_i
    size_t sc_right;       // max_commits + max_openings + 1 elements: [sum r per commitment ..., r_i z_i ..., -sum r_i y_i]
    size_t sc_left;        // the same count: [0 ..., r_i ..., 0]
    size_t y;              // max_openings elements: the values of the blob form (zkp_kzg_verify_evals_batch_dev)
    size_t gen;            // 96 bytes: the generator of G1 as the entries take points
    size_t report;         // two validation reports of 32 bytes: the commitments', the proofs'
    size_t table;          // table_words words
    size_t total;          // of the device workspace
    size_t stage_total;    // the pinned staging buffer: the table as it is copied
    size_t scratch_words;  // host words the sort counts in: max_commits + 1
};
inline KzgPointsSizes kzg_points_sizes(unsigned chunk_log, uint64_t max_openings, uint64_t max_commits) {
    KzgPointsSizes s;
    s.max_cchunks = kzg_cells_max_chunks(max_openings, max_commits, chunk_log);
    s.max_blocks = kzg_points_blocks(max_openings);
    s.table_words = (size_t)(max_openings + (s.max_cchunks + 1) + (max_commits + 1));
    s.cpartial = 0;
    s.ypartial = s.cpartial + 32 * (size_t)s.max_cchunks;
    s.sc_right = s.ypartial + 32 * (size_t)s.max_blocks;
    s.sc_left = s.sc_right + 32 * (size_t)(max_commits + max_openings + 1);
    s.y = s.sc_left + 32 * (size_t)(max_commits + max_openings + 1);
    s.gen = s.y + 32 * (size_t)max_openings;
    s.report = s.gen + 96;
    s.table = s.report + 64;
    s.total = (s.table + 4 * s.table_words + 31) & ~(size_t)31;
    s.stage_total = 4 * s.table_words;
    s.scratch_words = (size_t)max_commits + 1;
    return s;
}

// The tables of one call, written to `table` (at least sz.table_words words); `scratch`: at least sz.scratch_words words.  The
// caller has checked openings <= max_openings, commits <= max_commits and commit_index[i] < commits; commit_index null: the
// identity index (commits == openings), which needs no table.
inline KzgPointsTables kzg_points_tables(unsigned chunk_log, const uint32_t* commit_index, uint64_t openings, uint64_t commits, uint32_t* scratch,
                                         uint32_t* table) {
    KzgPointsTables t;
    t.openings = openings;
    t.commits = commits;
    t.identity = commit_index == nullptr;
    t.cchunks = 0;
    t.by_commit = t.cchunk_start = t.cseg_chunk = t.words = 0;
    if (t.identity) return t;
    // the chunk count decides where the last piece begins: count first, in scratch
    for (uint64_t m = 0; m <= commits; m++) scratch[m] = 0;
    for (uint64_t i = 0; i < openings; i++) scratch[commit_index[i]]++;
    const uint64_t per = (uint64_t)1 << chunk_log;
    for (uint64_t m = 0; m < commits; m++) t.cchunks += (scratch[m] + per - 1) >> chunk_log;
    t.cchunk_start = t.by_commit + (size_t)openings;
    t.cseg_chunk = t.cchunk_start + (size_t)t.cchunks + 1;
    t.words = t.cseg_chunk + (size_t)commits + 1;
    kzg_cells_sort(commit_index, openings, commits, chunk_log, false, scratch, table + t.by_commit, table + t.cchunk_start, nullptr,
                   table + t.cseg_chunk);
    return t;
}

// ---- the launches of one call, in order ----
enum KzgPointsStepKind {
    KZG_POINTS_SCALARS,  // workgroup b, lane t, opening i = b THREADS + t < N: rz[i] = r_i z_i, r[i] = r_i (and commit_weight[i] = r_i with the
                         // identity index); ypartial[b] = the sum of r_i y_i over the workgroup, up a tree (lanes past N add zero)
    KZG_POINTS_FINISH,   // one workgroup: neg_sum = -(sum of ypartial[0 .. blocks)), lane t taking t, t + THREADS, ..., then the tree
    KZG_POINTS_CHUNKS,   // lane q < CC: cpartial[q] = the sum of r over chunk q of the sort by commitment, in the chunk's order
    KZG_POINTS_COMMITS   // lane m < M: commit_weight[m] = the sum of cpartial over the chunks of commitment m (zero when it has none)
};
constexpr unsigned KZG_POINTS_STEPS = 4;
struct KzgPointsStep {
    KzgPointsStepKind kind;
    uint64_t lanes;   // that have work
    uint64_t blocks;  // workgroups of KZG_CELLS_THREADS lanes launched (0: nothing to launch)
};
inline KzgPointsStep kzg_points_step(const KzgPointsTables& t, unsigned i) {
    switch (i) {
    case 0: return {KZG_POINTS_SCALARS, t.openings, kzg_points_blocks(t.openings)};
    case 1: return {KZG_POINTS_FINISH, KZG_CELLS_THREADS, 1};
    case 2: return {KZG_POINTS_CHUNKS, t.cchunks, kzg_points_blocks(t.cchunks)};
    default: return {KZG_POINTS_COMMITS, t.identity ? 0 : t.commits, t.identity ? 0 : kzg_points_blocks(t.commits)};
    }
}

// ---- the index arithmetic of the kernels ----
// the leaf of lane t in a workgroup's tree of 2 THREADS elements (node k has the children 2k and 2k + 1; the root is node 1)
ZKP_CELLS_FN uint32_t kzg_points_leaf(uint32_t t) { return KZG_CELLS_THREADS + t; }

// ---- the bisection of zkp_kzg_verify_points_find_bad: the slice [lo, hi) is known to fail; its lower half is tested next ----
inline uint64_t kzg_points_bisect_mid(uint64_t lo, uint64_t hi) { return lo + (hi - lo + 1) / 2; }
// the most further pairing checks a rejected batch of `openings` costs: ceil(log2 openings)
inline unsigned kzg_points_bisect_checks(uint64_t openings) {
    unsigned k = 0;
    while (((uint64_t)1 << k) < openings) k++;
    return k;
}

}  // namespace zkp
