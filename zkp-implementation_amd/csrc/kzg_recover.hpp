// kzg_recover.hpp -- the kernels of zkp_kzg_recover_cosets* (driver: kzg_recover_host.inc; every launch, index and size:
// kzg_recover_plan.hpp, whose header comment states the construction).  The transforms are run_ntt<Fr>; what is here is the product
// tree's leaves and pointwise passes, the masked multiply, the inversion and divide passes and the tail.  Fr elements are Montgomery
// residues in memory and in LDS.
#pragma once
#include "ff.hpp"
#include "fr29.hpp"
#include "fr_pow2.hpp"
#include "kzg_recover_plan.hpp"
#include "plonk.hpp"  // fr_inverse

namespace zkp {

static_assert(KZG_RECOVER_MAX_LOG == FR_POW2_BITS, "fr_pow2.hpp: a root's index has KZG_RECOVER_MAX_LOG bits");

// Workgroup q: the monic product of the factors (Y - root_j), j in [q per, (q + 1) per), per = 2^per_log <= blockDim.x <= 256 --
// schoolbook, one lane per coefficient, one factor per step.  After s factors the product is Y^s + sum_{k<s} c[k] Y^k; the factor
// (Y - a) makes c[k] <- c[k-1] - a c[k] for k <= s, with c[s] standing for the leading 1 and c[-1] = 0.  The pad root is 0.
__global__ __launch_bounds__(256) void recover_leaf_kernel(const uint32_t* __restrict__ roots, FrPow2 rho, uint32_t per_log,
                                                           Fr* __restrict__ x) {
    __shared__ Fr a[256];
    __shared__ Fr c[256];
    const uint32_t t = threadIdx.x, per = 1u << per_log;
    const uint64_t base = (uint64_t)blockIdx.x << per_log;
    if (t < per) {
        const uint32_t idx = roots[base + t];
        Fr v = Fr::zero();
        if (idx != KZG_RECOVER_PAD_ROOT) {
            v = Fr::one();
            v = fr_pow2_mul(v, rho, idx);
        }
        a[t] = v;
    }
    __syncthreads();
#pragma unroll 1
    for (uint32_t s = 0; s < per; s++) {
        Fr nv = Fr::zero();
        const bool on = t <= s;
        if (on) {
            const Fr hi = t == s ? Fr::one() : c[t];
            const Fr lo = t ? c[t - 1] : Fr::zero();
            nv = lo - a[s] * hi;
        }
        __syncthreads();
        if (on) c[t] = nv;
        __syncthreads();
    }
    if (t < per) x[base + t] = c[t];
}

// w[i] = the node's low coefficients below d, zero from d to 2d (i < total = 2R)
__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_pad_kernel(const Fr* __restrict__ x, Fr* __restrict__ w, uint32_t log_d,
                                                                          uint64_t total) {
    const uint64_t i = (uint64_t)blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    if (i >= total) return;
    const int64_t src = kzg_recover_pad_source(log_d, i);
    w[i] = src >= 0 ? x[src] : Fr::zero();
}

// The product of a pair of nodes in the transformed domain with the add-in of (A + B) Y^d: x[i] = a b + (-1)^i (a + b), i < total = R
__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_pair_kernel(const Fr* __restrict__ w, Fr* __restrict__ x, uint32_t log_2d,
                                                                           uint64_t total) {
    const uint64_t i = (uint64_t)blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    if (i >= total) return;
    const KzgRecoverPair p = kzg_recover_pair(log_2d, i);
    const Fr a = w[p.a], b = w[p.b];
    const Fr s = a + b, ab = a * b;
    x[i] = p.minus ? ab - s : ab + s;
}

// The coefficients of Zs, twice (k < r): x[pad + k] below m, the leading 1 at m, zero behind
__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_zs_kernel(const Fr* __restrict__ x, uint64_t pad, uint64_t m, uint64_t r,
                                                                         Fr* __restrict__ zs0, Fr* __restrict__ zs1) {
    const uint64_t k = (uint64_t)blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    if (k >= r) return;
    const Fr v = k < m ? x[pad + k] : k == m ? Fr::one() : Fr::zero();
    zs0[k] = v;
    zs1[k] = v;
}

// out_i = E_i Zs(rho^(i mod r)) on present cosets, 0 on missing ones, whose 32 bytes are not read
__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_mul_kernel(const Fr* __restrict__ evals, const uint8_t* __restrict__ present,
                                                                          const Fr* __restrict__ zs, uint32_t log_r, uint64_t n,
                                                                          Fr* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint64_t k = i & (((uint64_t)1 << log_r) - 1);
    out[i] = present[k] ? evals[i] * zs[k] : Fr::zero();
}

// z[i] <- z[i]^-1, i < r, none of them zero (g^n != 1): a lane inverts the product of its KZG_RECOVER_INV_CHUNK values once
// (Montgomery's trick) and unwinds it; a slot at or beyond r holds 1
__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_inv_kernel(Fr* __restrict__ z, uint64_t r, uint64_t lanes) {
    const uint64_t t = (uint64_t)blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    if (t >= lanes) return;
    static_assert(KZG_RECOVER_INV_CHUNK == 4, "the chunk is written out (arrays of field elements would live in scratch memory)");
    const uint64_t i0 = kzg_recover_inv_index(lanes, t, 0), i1 = kzg_recover_inv_index(lanes, t, 1), i2 = kzg_recover_inv_index(lanes, t, 2),
                   i3 = kzg_recover_inv_index(lanes, t, 3);
    const Fr v0 = z[i0], v1 = i1 < r ? z[i1] : Fr::one(), v2 = i2 < r ? z[i2] : Fr::one(), v3 = i3 < r ? z[i3] : Fr::one();
    const Fr p1 = v0 * v1, p2 = p1 * v2, p3 = p2 * v3;
    Fr inv = fr_inverse(p3);
    if (i3 < r) z[i3] = inv * p2;
    inv = inv * v3;
    if (i2 < r) z[i2] = inv * p1;
    inv = inv * v2;
    if (i1 < r) z[i1] = inv * v0;
    z[i0] = inv * v1;
}

// a[i] <- a[i] zinv[i mod r]
__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_div_kernel(Fr* __restrict__ a, const Fr* __restrict__ zinv, uint32_t log_r,
                                                                          uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    if (i >= n) return;
    a[i] = a[i] * zinv[i & (((uint64_t)1 << log_r) - 1)];
}

// The first len coefficients go out (and, where asked for, all n with zeros from len on: the input of the evaluations' transform);
// *inconsistent becomes 1 when a coefficient at an index >= len is not zero (one atomic per wave that saw one)
__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_tail_kernel(const Fr* __restrict__ a, uint64_t n, uint64_t len,
                                                                           Fr* __restrict__ out_coeffs, Fr* __restrict__ out_padded,
                                                                           uint32_t* __restrict__ inconsistent) {
    const uint64_t i = (uint64_t)blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    bool nz = false;
    if (i < n) {
        const Fr v = a[i];
        if (i < len) {
            out_coeffs[i] = v;
            if (out_padded) out_padded[i] = v;
        } else {
            nz = !v.is_zero();
            if (out_padded) out_padded[i] = Fr::zero();
        }
    }
    if (__any(nz) && (threadIdx.x & 63) == 0) atomicOr(inconsistent, 1u);
}

}  // namespace zkp
