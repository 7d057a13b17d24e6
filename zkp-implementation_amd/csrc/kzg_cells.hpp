// kzg_cells.hpp -- the kernels of zkp_kzg_verify_cells* and zkp_kzg_cells_aggregate_dev (driver: kzg_cells_host.inc; the equation,
// the tables and every size: kzg_cells_plan.hpp).  The transform of A is run_ntt<Fr>; what is here is the two-step weighted sums and
// the scalars of the two MSMs.  Fr elements are Montgomery residues in memory.  Every sum is taken in the order its table gives.
#pragma once
#include "ff.hpp"
#include "fr29.hpp"
#include "fr_pow2.hpp"
#include "kzg_cells_plan.hpp"

namespace zkp {

static_assert(KZG_CELLS_MAX_LOG == FR_POW2_BITS, "fr_pow2.hpp: a coset's index has KZG_CELLS_MAX_LOG bits");

// Lane t < chunks l: row q = t / l of the chunk sums, element j = t % l.  Consecutive lanes read consecutive 32-byte elements of a
// cell.  From l = 64 on a wave lies inside one chunk (`uniform`, a kernel argument): its chunk bounds, cell ids and weights are then
// formed from the first lane's index, so that they are loaded once per wave instead of once per lane.
__global__ __launch_bounds__(KZG_CELLS_THREADS) void cells_aggregate_kernel(const Fr* __restrict__ evals, const Fr* __restrict__ weights,
                                                                            const uint32_t* __restrict__ by_coset,
                                                                            const uint32_t* __restrict__ chunk_start, uint32_t log_l,
                                                                            uint32_t uniform, uint64_t lanes, Fr* __restrict__ partial) {
    const uint64_t t = (uint64_t)blockIdx.x * KZG_CELLS_THREADS + threadIdx.x;
    if (t >= lanes) return;
    uint32_t q = (uint32_t)(t >> log_l);
    if (uniform) q = __builtin_amdgcn_readfirstlane(q);
    const uint64_t j = t & (((uint64_t)1 << log_l) - 1);
    const uint32_t first = chunk_start[q], last = chunk_start[q + 1];
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t at = first; at < last; at++) {
        const uint32_t cell = by_coset[at];
        acc = acc + weights[cell] * evals[kzg_cells_eval_index(log_l, cell, j)];
    }
    partial[kzg_cells_partial_index(log_l, q, j)] = acc;
}

// Lane t < used l: used coset u = t / l, value j = t % l of A: the chunk rows of the coset, summed in chunk order
__global__ __launch_bounds__(KZG_CELLS_THREADS) void cells_combine_kernel(const Fr* __restrict__ partial, const uint32_t* __restrict__ used_coset,
                                                                          const uint32_t* __restrict__ seg_chunk, uint32_t log_l,
                                                                          uint32_t log_r, uint64_t lanes, Fr* __restrict__ a) {
    const uint64_t t = (uint64_t)blockIdx.x * KZG_CELLS_THREADS + threadIdx.x;
    if (t >= lanes) return;
    const uint64_t u = t >> log_l, j = t & (((uint64_t)1 << log_l) - 1);
    const uint32_t first = seg_chunk[u], last = seg_chunk[u + 1];
    Fr acc = partial[kzg_cells_partial_index(log_l, first, j)];  // (a coset in use has at least one chunk)
#pragma unroll 1
    for (uint32_t q = first + 1; q < last; q++) acc = acc + partial[kzg_cells_partial_index(log_l, q, j)];
    a[kzg_cells_a_index(log_r, used_coset[u], j)] = acc;
}

// interp[j] = r a[j], j < l: the coefficients of sum rho_i I_i from the inverse transform of A (r_mont: r as a residue)
__global__ __launch_bounds__(KZG_CELLS_THREADS) void cells_tail_kernel(const Fr* __restrict__ a, Fr r_mont, uint64_t l, Fr* __restrict__ interp) {
    const uint64_t j = (uint64_t)blockIdx.x * KZG_CELLS_THREADS + threadIdx.x;
    if (j < l) interp[j] = a[j] * r_mont;
}

// Lane t < cells: proof_scalar[t] = rho_t (w^l)^(k_t).  Lane cells + q, q < cchunks: the weights of chunk q of the sort by
// commitment, summed in the chunk's order.
__global__ __launch_bounds__(KZG_CELLS_THREADS) void cells_scalars_kernel(const Fr* __restrict__ weights, const uint32_t* __restrict__ cell_coset,
                                                                          const uint32_t* __restrict__ by_commit,
                                                                          const uint32_t* __restrict__ cchunk_start, FrPow2 rho, uint64_t cells,
                                                                          uint64_t cchunks, Fr* __restrict__ proof_scalar,
                                                                          Fr* __restrict__ cpartial) {
    const uint64_t t = (uint64_t)blockIdx.x * KZG_CELLS_THREADS + threadIdx.x;
    if (t < cells) {
        const uint32_t k = cell_coset[t];
        proof_scalar[t] = fr_pow2_mul(weights[t], rho, k);
    } else if (t - cells < cchunks) {
        const uint64_t q = t - cells;
        const uint32_t first = cchunk_start[q], last = cchunk_start[q + 1];
        Fr acc = Fr::zero();
#pragma unroll 1
        for (uint32_t at = first; at < last; at++) acc = acc + weights[by_commit[at]];
        cpartial[q] = acc;
    }
}

// commit_weight[m] = the chunk sums of commitment m in chunk order, zero for a commitment no cell names (m < commits)
__global__ __launch_bounds__(KZG_CELLS_THREADS) void cells_commits_kernel(const Fr* __restrict__ cpartial, const uint32_t* __restrict__ cseg_chunk,
                                                                          uint64_t commits, Fr* __restrict__ commit_weight) {
    const uint64_t m = (uint64_t)blockIdx.x * KZG_CELLS_THREADS + threadIdx.x;
    if (m >= commits) return;
    const uint32_t first = cseg_chunk[m], last = cseg_chunk[m + 1];
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t q = first; q < last; q++) acc = acc + cpartial[q];
    commit_weight[m] = acc;
}

}  // namespace zkp
