// kzg_recover.hpp -- the kernels of zkp_kzg_recover_cosets* (driver: kzg_recover_host.inc; every launch, index and size:
// kzg_recover_plan.hpp, whose header comment states the construction).  The transforms are run_ntt<Fr>; what is here is the product
// tree's leaves and pointwise passes, the masked multiply, the inversion and divide passes and the tail, and behind them the forms
// of the multiply, the divide and the tail that take the rows of a batch (zkp_kzg_recover_cosets_batch*) with the transposition
// between natural order and cell layout.  Fr elements are Montgomery residues in memory and in LDS.
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

// ---- a batch of `polys` rows of n (zkp_kzg_recover_cosets_batch*) ----
// The pointwise passes as above with a row index: blockIdx.x covers the n indices, blockIdx.y a group of KZG_RECOVER_ROWS rows, and
// what depends on the index alone -- present[k], Zs(rho^k), Zs(g rho^k)^-1 -- is loaded once for the rows of the group.

__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_mul_batch_kernel(const Fr* __restrict__ evals, const uint8_t* __restrict__ present,
                                                                                const Fr* __restrict__ zs, uint32_t log_r, uint32_t log_n,
                                                                                uint32_t polys, Fr* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    if (i >> log_n) return;
    const uint64_t k = i & (((uint64_t)1 << log_r) - 1);
    const uint32_t p0 = blockIdx.y * KZG_RECOVER_ROWS, p1 = min(p0 + KZG_RECOVER_ROWS, polys);
    if (!present[k]) {
        for (uint32_t p = p0; p < p1; p++) out[kzg_recover_offset(KZG_RECOVER_NATURAL, log_n, log_n - log_r, p, i)] = Fr::zero();
        return;
    }
    const Fr z = zs[k];
#pragma unroll 1
    for (uint32_t p = p0; p < p1; p++) {
        const uint64_t at = kzg_recover_offset(KZG_RECOVER_NATURAL, log_n, log_n - log_r, p, i);
        out[at] = evals[at] * z;
    }
}

// One tile of a row between the layouts through LDS: `v` of the lane's element on the side it was read goes in, the value of the
// lane's element on the other side comes out.  Fr is eight 32-bit limbs; a plane per pair of limbs.
__device__ __forceinline__ Fr recover_tile_turn(uint64_t (*tile)[KZG_RECOVER_TILE_SLOTS], bool active, const Fr& v, uint32_t slot_in,
                                                uint32_t slot_out) {
    static_assert(sizeof(Fr) == 32, "a tile plane holds a quarter of an element");
    __syncthreads();  // the previous row's reads are done
    if (active) {
#pragma unroll
        for (int w = 0; w < 4; w++) tile[w][slot_in] = (uint64_t)v.l[2 * w] | ((uint64_t)v.l[2 * w + 1] << 32);
    }
    __syncthreads();
    Fr o = Fr::zero();
    if (active) {
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint64_t x = tile[w][slot_out];
            o.l[2 * w] = (uint32_t)x;
            o.l[2 * w + 1] = (uint32_t)(x >> 32);
        }
    }
    return o;
}

// The masked multiply with the evaluations in cell layout (row p: r cells of l contiguous values), transposed on the way: workgroup
// blockIdx.x takes tile q of the rows of its group, reads it cell side (value times Zs(rho^k), zero for a missing cell, whose bytes
// are not read) and stores it natural side.  zs == nullptr: the plain transposition (m = 0).
__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_mul_cells_kernel(const Fr* __restrict__ evals, const uint8_t* __restrict__ present,
                                                                                const Fr* __restrict__ zs, uint32_t log_n, uint32_t log_l,
                                                                                uint32_t polys, Fr* __restrict__ out) {
    __shared__ uint64_t tile[4][KZG_RECOVER_TILE_SLOTS];
    const KzgRecoverTile tl = kzg_recover_tile(log_n, log_l);
    const uint32_t t = threadIdx.x;
    const bool active = t < (1u << (tl.tk_log + tl.tj_log));
    const KzgRecoverTileAt c = kzg_recover_tile_at(log_n, log_l, blockIdx.x, t, true), d = kzg_recover_tile_at(log_n, log_l, blockIdx.x, t, false);
    const unsigned log_r = log_n - log_l;
    const bool have = active && (!zs || present[c.k]);
    Fr z = Fr::one();
    if (have && zs) z = zs[c.k];
    const uint32_t p0 = blockIdx.y * KZG_RECOVER_ROWS, p1 = min(p0 + KZG_RECOVER_ROWS, polys);
#pragma unroll 1
    for (uint32_t p = p0; p < p1; p++) {
        Fr v = Fr::zero();
        if (have) {
            v = evals[kzg_recover_offset(KZG_RECOVER_CELLS, log_n, log_l, p, c.k + (c.j << log_r))];
            if (zs) v = v * z;
        }
        const Fr o = recover_tile_turn(tile, active, v, c.slot, d.slot);
        if (active) out[kzg_recover_offset(KZG_RECOVER_NATURAL, log_n, log_l, p, d.k + (d.j << log_r))] = o;
    }
}

// KZG_RECOVER_CELLS_OUT: rows in natural order -> the caller's rows in cell layout, the same tiles the other way round
__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_cells_out_kernel(const Fr* __restrict__ in, uint32_t log_n, uint32_t log_l,
                                                                                uint32_t polys, Fr* __restrict__ out) {
    __shared__ uint64_t tile[4][KZG_RECOVER_TILE_SLOTS];
    const KzgRecoverTile tl = kzg_recover_tile(log_n, log_l);
    const uint32_t t = threadIdx.x;
    const bool active = t < (1u << (tl.tk_log + tl.tj_log));
    const KzgRecoverTileAt c = kzg_recover_tile_at(log_n, log_l, blockIdx.x, t, true), d = kzg_recover_tile_at(log_n, log_l, blockIdx.x, t, false);
    const unsigned log_r = log_n - log_l;
    const uint32_t p0 = blockIdx.y * KZG_RECOVER_ROWS, p1 = min(p0 + KZG_RECOVER_ROWS, polys);
#pragma unroll 1
    for (uint32_t p = p0; p < p1; p++) {
        Fr v = Fr::zero();
        if (active) v = in[kzg_recover_offset(KZG_RECOVER_NATURAL, log_n, log_l, p, d.k + (d.j << log_r))];
        const Fr o = recover_tile_turn(tile, active, v, d.slot, c.slot);
        if (active) out[kzg_recover_offset(KZG_RECOVER_CELLS, log_n, log_l, p, c.k + (c.j << log_r))] = o;
    }
}

__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_div_batch_kernel(Fr* __restrict__ a, const Fr* __restrict__ zinv, uint32_t log_r,
                                                                                uint32_t log_n, uint32_t polys) {
    const uint64_t i = (uint64_t)blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    if (i >> log_n) return;
    const Fr z = zinv[i & (((uint64_t)1 << log_r) - 1)];
    const uint32_t p0 = blockIdx.y * KZG_RECOVER_ROWS, p1 = min(p0 + KZG_RECOVER_ROWS, polys);
#pragma unroll 1
    for (uint32_t p = p0; p < p1; p++) {
        const uint64_t at = ((uint64_t)p << log_n) + i;
        a[at] = a[at] * z;
    }
}

// The tail of every row: len of the `stride` scalars of row p of out_coeffs (the rest is not written), the zero-padded row of
// out_padded where asked for (it may be `a` itself: a lane writes only what it has read), and the row's own word (one atomic per
// wave that saw a non-zero coefficient of that row)
__global__ __launch_bounds__(KZG_RECOVER_THREADS) void recover_tail_batch_kernel(const Fr* a, uint32_t log_n, uint64_t len, uint64_t stride,
                                                                                 uint32_t polys, Fr* __restrict__ out_coeffs, Fr* out_padded,
                                                                                 uint32_t* __restrict__ inconsistent) {
    const uint64_t i = (uint64_t)blockIdx.x * KZG_RECOVER_THREADS + threadIdx.x;
    const bool in = !(i >> log_n);
    const uint32_t p0 = blockIdx.y * KZG_RECOVER_ROWS, p1 = min(p0 + KZG_RECOVER_ROWS, polys);
#pragma unroll 1
    for (uint32_t p = p0; p < p1; p++) {
        bool nz = false;
        if (in) {
            const uint64_t at = ((uint64_t)p << log_n) + i;
            const Fr v = a[at];
            if (i < len) {
                out_coeffs[(uint64_t)p * stride + i] = v;
                if (out_padded && out_padded != a) out_padded[at] = v;
            } else {
                nz = !v.is_zero();
                if (out_padded) out_padded[at] = Fr::zero();
            }
        }
        if (__any(nz) && (threadIdx.x & 63) == 0) atomicOr(inconsistent + p, 1u);
    }
}

}  // namespace zkp
