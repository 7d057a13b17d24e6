// kzg_points.hpp -- the kernels of zkp_kzg_verify_points* and zkp_kzg_points_aggregate_dev (driver: kzg_points_host.inc; the equation,
// the tables, the launches and every size: kzg_points_plan.hpp).  Fr elements are Montgomery residues in memory and in LDS.  No
// kernel uses an atomic: every sum is taken in the order its table, or the tree, gives.  In the two kernels with a tree no lane
// leaves early: the barriers are reached by all KZG_CELLS_THREADS of them.
#pragma once
#include "ff.hpp"
#include "fr29.hpp"
#include "kzg_cells.hpp"  // cells_commits_kernel
#include "kzg_points_plan.hpp"

namespace zkp {

// tree[1] <- the sum of the KZG_CELLS_THREADS leaves, pairs left to right, level by level (a fixed order; the shape of
// evals_tree_up in kzg_evals.hpp)
ZKP_DEV void points_tree_sum(Fr* tree, uint32_t t) {
    __syncthreads();  // the leaves are written
#pragma unroll 1
    for (uint32_t s = KZG_CELLS_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) tree[s + t] = tree[2 * (s + t)] + tree[2 * (s + t) + 1];
        __syncthreads();
    }
}

// KZG_POINTS_SCALARS: opening i = block THREADS + t.  The weight is made canonical once (r_i = weight * 1) and everything is formed
// from that, so every word written is canonical whatever the caller's limbs.  commit_weight: null unless the index is the identity.
__global__ __launch_bounds__(KZG_CELLS_THREADS) void points_scalars_kernel(const Fr* __restrict__ weights, const Fr* __restrict__ z,
                                                                           const Fr* __restrict__ y, uint64_t openings, Fr* __restrict__ out_rz,
                                                                           Fr* __restrict__ out_r, Fr* __restrict__ commit_weight,
                                                                           Fr* __restrict__ ypartial) {
    __shared__ Fr tree[2 * KZG_CELLS_THREADS];
    const uint32_t t = threadIdx.x;
    const uint64_t i = (uint64_t)blockIdx.x * KZG_CELLS_THREADS + t;
    Fr leaf = Fr::zero();
    if (i < openings) {
        const Fr r = weights[i] * Fr::one();
        out_r[i] = r;
        out_rz[i] = r * z[i];
        if (commit_weight) commit_weight[i] = r;
        leaf = r * y[i];
    }
    tree[kzg_points_leaf(t)] = leaf;
    points_tree_sum(tree, t);
    if (t == 0) ypartial[blockIdx.x] = tree[1];
}

// KZG_POINTS_FINISH: one workgroup.  neg_sum = -(ypartial[0] + ... + ypartial[blocks - 1]); zero for no workgroup at all.
__global__ __launch_bounds__(KZG_CELLS_THREADS) void points_finish_kernel(const Fr* __restrict__ ypartial, uint64_t blocks, Fr* __restrict__ neg_sum) {
    __shared__ Fr tree[2 * KZG_CELLS_THREADS];
    const uint32_t t = threadIdx.x;
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint64_t b = t; b < blocks; b += KZG_CELLS_THREADS) acc = acc + ypartial[b];
    tree[kzg_points_leaf(t)] = acc;
    points_tree_sum(tree, t);
    if (t == 0) *neg_sum = neg(tree[1]);
}

// KZG_POINTS_CHUNKS: lane q < cchunks: the weights of chunk q of the sort by commitment, made canonical, summed in the chunk's order
__global__ __launch_bounds__(KZG_CELLS_THREADS) void points_chunks_kernel(const Fr* __restrict__ weights, const uint32_t* __restrict__ by_commit,
                                                                          const uint32_t* __restrict__ cchunk_start, uint64_t cchunks,
                                                                          Fr* __restrict__ cpartial) {
    const uint64_t q = (uint64_t)blockIdx.x * KZG_CELLS_THREADS + threadIdx.x;
    if (q >= cchunks) return;
    const uint32_t first = cchunk_start[q], last = cchunk_start[q + 1];
    const Fr one = Fr::one();
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t at = first; at < last; at++) acc = acc + weights[by_commit[at]] * one;
    cpartial[q] = acc;
}

// KZG_POINTS_COMMITS is cells_commits_kernel (kzg_cells.hpp) as it is: the chunk sums of commitment m in chunk order, zero for a
// commitment no opening names.

}  // namespace zkp
