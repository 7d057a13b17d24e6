// kzg_evals.hpp -- the kernels of zkp_kzg_commit_evals_batch* and zkp_kzg_open_evals_batch* (driver: kzg_evals_host.inc; the
// formulas, every index, grid and size: kzg_evals_plan.hpp).  Fr elements are Montgomery residues in memory and in LDS.  Every
// workgroup has KZG_EVALS_THREADS lanes and no lane leaves early: the barriers are reached by all of them.
#pragma once
#include "ff.hpp"
#include "fr29.hpp"
#include "fr_inv.hpp"
#include "kzg_evals_plan.hpp"
#include "plonk.hpp"  // fr_inverse

namespace zkp {

// the one inversion of a workgroup, by ZKP_KZG_EVALS_INVERSE (0: division steps, 1: the Fermat power)
ZKP_DEV Fr evals_inverse(const Fr& a, int method) { return method ? fr_inverse(a) : fr_inverse_gcd(a); }

// tree[1] <- the combination of the KZG_EVALS_THREADS leaves, pairs left to right, level by level (a fixed order)
template <bool MUL>
ZKP_DEV void evals_tree_up(Fr* tree, uint32_t t) {
    __syncthreads();  // the leaves are written
#pragma unroll 1
    for (uint32_t s = KZG_EVALS_THREADS / 2; s >= 1; s >>= 1) {
        if (t < s) {
            const Fr a = tree[2 * (s + t)], b = tree[2 * (s + t) + 1];
            tree[s + t] = MUL ? a * b : a + b;
        }
        __syncthreads();
    }
}

// The denominator of the element at position i (KZG_EVALS_NONE: the lane holds none, 1), *zero set and the row's word written when
// it vanishes: at most one lane of a row meets that, so a plain store is enough
ZKP_DEV Fr evals_denominator(const Fr* __restrict__ roots, const Fr& z, int order, uint32_t log_n, uint32_t i, uint32_t* __restrict__ hit_word,
                             bool& zero) {
    zero = false;
    if (i == KZG_EVALS_NONE) return Fr::one();
    const uint32_t e = kzg_evals_exponent(order, log_n, i);
    Fr d = roots[e] - z;
    if (d.is_zero()) {
        zero = true;
        *hit_word = e;
        d = Fr::one();
    }
    return d;
}

// f_i w^e(i) / d_i of the element at position i (zero for none, and for the element whose d vanished)
ZKP_DEV Fr evals_term(const Fr* __restrict__ row, const Fr* __restrict__ roots, int order, uint32_t log_n, uint32_t i, bool skip, const Fr& dinv) {
    if (i == KZG_EVALS_NONE || skip) return Fr::zero();
    return row[i] * roots[kzg_evals_exponent(order, log_n, i)] * dinv;
}

// KZG_EVALS_INVERT: workgroup (b, p) takes wg_elems elements of row p.  dinv by position; partial[p blocks + b] = the sum of its terms.
// METHOD: the inversion (an instantiation each: together in one kernel their constants do not fit the scalar registers)
template <int METHOD>
__global__ __launch_bounds__(KZG_EVALS_THREADS) void evals_invert_kernel(const Fr* __restrict__ evals, const Fr* __restrict__ z,
                                                                         const Fr* __restrict__ roots, uint32_t log_n, int order,
                                                                         Fr* __restrict__ dinv, uint32_t* __restrict__ hit, Fr* __restrict__ partial) {
    __shared__ Fr tree[2 * KZG_EVALS_THREADS];
    static_assert(KZG_EVALS_CHUNK == 4, "the chunk is written out (arrays of field elements would live in scratch memory)");
    const KzgEvalsGeom g = kzg_evals_geom(log_n);
    const uint32_t t = threadIdx.x, b = blockIdx.x, p = blockIdx.y;
    const Fr zp = z[p] * Fr::one();  // canonical whatever the caller's limbs
    const uint32_t i0 = kzg_evals_element(g, b, t, 0), i1 = kzg_evals_element(g, b, t, 1), i2 = kzg_evals_element(g, b, t, 2),
                   i3 = kzg_evals_element(g, b, t, 3);
    bool z0, z1, z2, z3;
    const Fr v0 = evals_denominator(roots, zp, order, log_n, i0, hit + p, z0), v1 = evals_denominator(roots, zp, order, log_n, i1, hit + p, z1),
             v2 = evals_denominator(roots, zp, order, log_n, i2, hit + p, z2), v3 = evals_denominator(roots, zp, order, log_n, i3, hit + p, z3);
    const Fr p1 = v0 * v1, p2 = p1 * v2, p3 = p2 * v3;
    tree[kzg_evals_leaf(t)] = p3;
    evals_tree_up<true>(tree, t);
    if (t < 64) {  // the first wave, all of its lanes on the same value: the early exit of the division steps stays wave-uniform
        const Fr r = evals_inverse(tree[1], METHOD);
        if (t == 0) tree[1] = r;
    }
    __syncthreads();
    // down: the inverse of a child is its parent's times its sibling's product
#pragma unroll 1
    for (uint32_t s = 1; s < KZG_EVALS_THREADS; s <<= 1) {
        const bool on = t < 2 * s;
        const uint32_t c = 2 * s + t;
        Fr nv = Fr::zero();
        if (on) nv = tree[c >> 1] * tree[c ^ 1];
        __syncthreads();
        if (on) tree[c] = nv;
        __syncthreads();
    }
    Fr inv = tree[kzg_evals_leaf(t)];
    const Fr* row = evals + kzg_evals_row_index(log_n, p, 0);
    Fr* drow = dinv + kzg_evals_row_index(log_n, p, 0);
    Fr acc, x;
    x = inv * p2;
    if (i3 != KZG_EVALS_NONE) drow[i3] = x;
    acc = evals_term(row, roots, order, log_n, i3, z3, x);
    inv = inv * v3;
    x = inv * p1;
    if (i2 != KZG_EVALS_NONE) drow[i2] = x;
    acc = acc + evals_term(row, roots, order, log_n, i2, z2, x);
    inv = inv * v2;
    x = inv * v0;
    if (i1 != KZG_EVALS_NONE) drow[i1] = x;
    acc = acc + evals_term(row, roots, order, log_n, i1, z1, x);
    x = inv * v1;
    if (i0 != KZG_EVALS_NONE) drow[i0] = x;
    acc = acc + evals_term(row, roots, order, log_n, i0, z0, x);
    tree[kzg_evals_leaf(t)] = acc;  // (every lane has read its own leaf; the last barrier of the way down is behind all other reads)
    evals_tree_up<false>(tree, t);
    if (t == 0) partial[kzg_evals_partial_index(g, p, b)] = tree[1];
}

// tree[1] <- the sum of the `blocks` partials of row p: lane t takes t, t + THREADS, ..., then the tree
ZKP_DEV void evals_sum_partials(Fr* tree, const Fr* __restrict__ partial, const KzgEvalsGeom& g, uint32_t p, uint32_t t) {
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t j = t; j < g.blocks; j += KZG_EVALS_THREADS) acc = acc + partial[kzg_evals_partial_index(g, p, j)];
    tree[kzg_evals_leaf(t)] = acc;
    evals_tree_up<false>(tree, t);
}

// KZG_EVALS_Y: y_p = (1 - z^n) / n times the row's sum, or the row's own value at w^m (made canonical) when z = w^m
__global__ __launch_bounds__(KZG_EVALS_THREADS) void evals_y_kernel(const Fr* __restrict__ evals, const Fr* __restrict__ z,
                                                                    const Fr* __restrict__ partial, const uint32_t* __restrict__ hit,
                                                                    uint32_t log_n, int order, Fr ninv, Fr* __restrict__ y) {
    __shared__ Fr tree[2 * KZG_EVALS_THREADS];
    const KzgEvalsGeom g = kzg_evals_geom(log_n);
    const uint32_t t = threadIdx.x, p = blockIdx.y;
    evals_sum_partials(tree, partial, g, p, t);
    if (t != 0) return;
    const uint32_t m = hit[p];
    if (m != KZG_EVALS_NONE) {
        y[p] = evals[kzg_evals_row_index(log_n, p, kzg_evals_position(order, log_n, m))] * Fr::one();
        return;
    }
    Fr zn = z[p];
#pragma unroll 1
    for (uint32_t k = 0; k < log_n; k++) zn = sqr(zn);
    y[p] = (Fr::one() - zn) * ninv * tree[1];
}

// KZG_EVALS_QUOTIENT: q at its natural index for every element but the one at w^m; for a row with m set also the partial sums of
// q_j w^j, j != m
__global__ __launch_bounds__(KZG_EVALS_THREADS) void evals_quotient_kernel(const Fr* __restrict__ evals, const Fr* __restrict__ roots,
                                                                           const Fr* __restrict__ dinv, const Fr* __restrict__ y,
                                                                           const uint32_t* __restrict__ hit, uint32_t log_n, int order,
                                                                           Fr* __restrict__ quotient, Fr* __restrict__ partial2) {
    __shared__ Fr tree[2 * KZG_EVALS_THREADS];
    const KzgEvalsGeom g = kzg_evals_geom(log_n);
    const uint32_t t = threadIdx.x, b = blockIdx.x, p = blockIdx.y;
    const Fr yp = y[p];
    const uint32_t m = hit[p];
    const Fr* row = evals + kzg_evals_row_index(log_n, p, 0);
    const Fr* drow = dinv + kzg_evals_row_index(log_n, p, 0);
    Fr* qrow = quotient + kzg_evals_row_index(log_n, p, 0);
    Fr acc = Fr::zero();
#pragma unroll 1
    for (uint32_t k = 0; k < KZG_EVALS_CHUNK; k++) {
        const uint32_t i = kzg_evals_element(g, b, t, k);
        if (i == KZG_EVALS_NONE) continue;
        const uint32_t e = kzg_evals_exponent(order, log_n, i);
        if (e == m) continue;
        const Fr q = (row[i] - yp) * drow[i];
        qrow[e] = q;
        if (m != KZG_EVALS_NONE) acc = acc + q * roots[e];
    }
    if (m == KZG_EVALS_NONE) return;  // the whole workgroup: m is the row's
    tree[kzg_evals_leaf(t)] = acc;
    evals_tree_up<false>(tree, t);
    if (t == 0) partial2[kzg_evals_partial_index(g, p, b)] = tree[1];
}

// KZG_EVALS_QM: q_m = -w^(-m) sum_{j != m} q_j w^j for the rows with m set
__global__ __launch_bounds__(KZG_EVALS_THREADS) void evals_qm_kernel(const Fr* __restrict__ roots, const Fr* __restrict__ partial2,
                                                                     const uint32_t* __restrict__ hit, uint32_t log_n,
                                                                     Fr* __restrict__ quotient) {
    __shared__ Fr tree[2 * KZG_EVALS_THREADS];
    const KzgEvalsGeom g = kzg_evals_geom(log_n);
    const uint32_t t = threadIdx.x, p = blockIdx.y;
    const uint32_t m = hit[p];
    if (m == KZG_EVALS_NONE) return;  // the whole workgroup
    evals_sum_partials(tree, partial2, g, p, t);
    if (t != 0) return;
    const uint32_t back = (uint32_t)((((uint64_t)1 << log_n) - m) & (((uint64_t)1 << log_n) - 1));  // w^(-m) = w^(n - m)
    quotient[kzg_evals_row_index(log_n, p, m)] = neg(roots[back] * tree[1]);
}

// rows of a bit-reversed handle into natural order (the scalars of the commitments' MSM)
__global__ __launch_bounds__(KZG_EVALS_THREADS) void evals_gather_kernel(const Fr* __restrict__ in, uint32_t log_n, int order, Fr* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * KZG_EVALS_THREADS + threadIdx.x;
    if (i >> log_n) return;
    out[kzg_evals_row_index(log_n, blockIdx.y, kzg_evals_exponent(order, log_n, (uint32_t)i))] = in[kzg_evals_row_index(log_n, blockIdx.y, (uint32_t)i)];
}

// roots[j] = w^j, j < n (once, at creation)
__global__ __launch_bounds__(KZG_EVALS_THREADS) void evals_roots_kernel(Fr w, uint32_t log_n, Fr* __restrict__ roots) {
    const uint64_t j = (uint64_t)blockIdx.x * KZG_EVALS_THREADS + threadIdx.x;
    if (j >> log_n) return;
    roots[j] = pow_u64<FrParams>(w, j);
}

// Self-test of the two device inversions of Fr (zkp_selftest_fr_inverse_dev): one lane per element, 8 words in and out, one wave
// per workgroup.  method 0: fr_inverse_gcd; method 1: fr_inverse.
constexpr unsigned FR_INVERSE_SELFTEST_THREADS = 64;
__global__ __launch_bounds__(FR_INVERSE_SELFTEST_THREADS) void fr_inverse_selftest_kernel(const Fr* __restrict__ in, Fr* __restrict__ out, uint64_t n,
                                                                                         int method) {
    const uint64_t i = (uint64_t)blockIdx.x * FR_INVERSE_SELFTEST_THREADS + threadIdx.x;
    if (i >= n) return;
    out[i] = evals_inverse(in[i], method);
}

}  // namespace zkp
