// nova.hpp -- sparse R1CS kernels of Nova folding (nova/src/nifs/mod.rs, nova/src/r1cs/mod.rs) over Fr.
//
//   NIFS::compute_t    nifs/mod.rs:34-59   six dense matrix-vector products  -> one pass over the CSR rows (nova_cross_*)
//   is_r1cs_satisfied  r1cs/mod.rs:94-127  three products + vector compare    -> count of violated rows (nova_residual_*)
//   NIFS::fold_witness nifs/mod.rs:64-82   two element-wise passes            -> one pass (nova_fold_kernel)
//
// z = (W || x || u) (nifs_prover.rs:22-28) is never materialised: column c reads W[c], x[c - num_vars] or u (nova_z).
// Rows come in two lists built at create time (csrc/nova_host.inc): short rows, one lane each, and long rows, one wave each with the
// lanes striding over the row's entries and the partial sums added across the wave in LDS.  Both kernels write T[row] for the rows of
// their list only, so every row is in exactly one list.  All values are arkworks Montgomery residues (saturated 8 x 32-bit, ff.hpp).
#pragma once
#include "ff.hpp"

namespace zkp {

constexpr int NOVA_THREADS = 256;
constexpr int NOVA_WAVE = 64;
// A row whose A, B and C rows hold more than this many entries together goes to the wave-per-row list.  On one lane a row of k entries
// costs 2k products (k per z vector); on a wave it costs about 2k/64 products plus the cross-lane sum (6 levels of 6 additions).  The
// split is there so that the rare linear-combination rows of thousands of entries do not hold a wave of 63 finished short rows; the
// value 64 (one entry per lane) is a round starting point, not a measured optimum -- tune it only against tools/nova_bench.py.
constexpr uint32_t NOVA_LONG_ROW = 64;

struct NovaCsr {
    const uint64_t* rp;  // rows + 1
    const uint32_t* col;
    const Fr* val;
};
struct NovaZ {  // z = (W || x || u)
    const Fr* w;
    const Fr* x;
    Fr u;
};
struct NovaRows {
    NovaCsr m[3];  // A, B, C
    uint32_t nv, nio;
    const uint32_t* list;  // row indices of this launch
    uint32_t count;
};

ZKP_DEV Fr nova_z(const NovaZ& z, uint32_t c, uint32_t nv, uint32_t nio) {
    if (c < nv) return z.w[c];
    if (c - nv < nio) return z.x[c - nv];
    return z.u;
}

// acc[m][k] = sum over the entries e = first, first + step, ... of row `row` of matrix m of val[e] * z_k[col[e]]
template <int NZ>
ZKP_DEV void nova_row_dots(const NovaRows& R, const NovaZ* z, uint32_t row, uint32_t first, uint32_t step, Fr (&acc)[3][NZ]) {
#pragma unroll
    for (int m = 0; m < 3; m++) {
#pragma unroll
        for (int k = 0; k < NZ; k++) acc[m][k] = Fr::zero();
        const uint64_t hi = R.m[m].rp[row + 1];
        for (uint64_t e = R.m[m].rp[row] + first; e < hi; e += step) {
            const uint32_t c = R.m[m].col[e];
            const Fr v = R.m[m].val[e];
#pragma unroll
            for (int k = 0; k < NZ; k++) acc[m][k] = acc[m][k] + v * nova_z(z[k], c, R.nv, R.nio);
        }
    }
}

// Sum of acc over the 64 lanes of a one-wave workgroup; lane 0 receives the total
template <int NZ>
ZKP_DEV void nova_wave_sum(Fr (&acc)[3][NZ]) {
    __shared__ Fr red[3 * NZ][NOVA_WAVE];
    const uint32_t lane = threadIdx.x;
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int k = 0; k < NZ; k++) red[m * NZ + k][lane] = acc[m][k];
    for (uint32_t s = NOVA_WAVE / 2; s > 0; s >>= 1) {
        __syncthreads();
        if (lane < s) {
#pragma unroll
            for (int j = 0; j < 3 * NZ; j++) red[j][lane] = red[j][lane] + red[j][lane + s];
        }
    }
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 3; m++)
#pragma unroll
        for (int k = 0; k < NZ; k++) acc[m][k] = red[m * NZ + k][0];
}

// T = A z1 o B z2 + A z2 o B z1 - u1 C z2 - u2 C z1 (nifs/mod.rs:48-56)
ZKP_DEV Fr nova_t(const Fr (&acc)[3][2], const Fr& u1, const Fr& u2) {
    return acc[0][0] * acc[1][1] + acc[0][1] * acc[1][0] - u1 * acc[2][1] - u2 * acc[2][0];
}

struct NovaZPair {
    NovaZ z[2];
};

__global__ __launch_bounds__(NOVA_THREADS) void nova_cross_short_kernel(NovaRows R, NovaZPair zp, Fr* t) {
    const uint32_t i = blockIdx.x * NOVA_THREADS + threadIdx.x;
    if (i >= R.count) return;
    const uint32_t row = R.list[i];
    Fr acc[3][2];
    nova_row_dots<2>(R, zp.z, row, 0, 1, acc);
    t[row] = nova_t(acc, zp.z[0].u, zp.z[1].u);
}

__global__ __launch_bounds__(NOVA_WAVE) void nova_cross_long_kernel(NovaRows R, NovaZPair zp, Fr* t) {
    const uint32_t row = R.list[blockIdx.x];
    Fr acc[3][2];
    nova_row_dots<2>(R, zp.z, row, threadIdx.x, NOVA_WAVE, acc);
    nova_wave_sum<2>(acc);
    if (threadIdx.x == 0) t[row] = nova_t(acc, zp.z[0].u, zp.z[1].u);
}

// (A z)_i (B z)_i != u (C z)_i + E_i (r1cs/mod.rs:111-118)
ZKP_DEV bool nova_row_bad(const Fr (&acc)[3][1], const Fr& u, const Fr& e) { return !(acc[0][0] * acc[1][0] == u * acc[2][0] + e); }

__global__ __launch_bounds__(NOVA_THREADS) void nova_residual_short_kernel(NovaRows R, NovaZ z, const Fr* e,
                                                                           unsigned long long* bad) {
    const uint32_t i = blockIdx.x * NOVA_THREADS + threadIdx.x;
    if (i >= R.count) return;
    const uint32_t row = R.list[i];
    Fr acc[3][1];
    nova_row_dots<1>(R, &z, row, 0, 1, acc);
    if (nova_row_bad(acc, z.u, e[row])) atomicAdd(bad, 1ull);
}

__global__ __launch_bounds__(NOVA_WAVE) void nova_residual_long_kernel(NovaRows R, NovaZ z, const Fr* e, unsigned long long* bad) {
    const uint32_t row = R.list[blockIdx.x];
    Fr acc[3][1];
    nova_row_dots<1>(R, &z, row, threadIdx.x, NOVA_WAVE, acc);
    nova_wave_sum<1>(acc);
    if (threadIdx.x == 0 && nova_row_bad(acc, z.u, e[row])) atomicAdd(bad, 1ull);
}

// E = E1 + r T + r^2 E2 (i < rows), W = W1 + r W2 (i < nv).  Element i is read and written by one lane only, so the outputs may be
// E1 / W1 themselves (no __restrict__ here on purpose).
__global__ __launch_bounds__(NOVA_THREADS) void nova_fold_kernel(const Fr* e1, const Fr* t, const Fr* e2, Fr* e_out, uint64_t rows,
                                                                 const Fr* w1, const Fr* w2, Fr* w_out, uint64_t nv, Fr r, Fr r2) {
    const uint64_t i = (uint64_t)blockIdx.x * NOVA_THREADS + threadIdx.x;
    if (i < rows) e_out[i] = e1[i] + r * t[i] + r2 * e2[i];
    if (i < nv) w_out[i] = w1[i] + r * w2[i];
}

}  // namespace zkp
