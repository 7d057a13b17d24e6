// pairing.hip -- the pairing kernels behind zkp_pairing_check_batch* and zkp_selftest_fq12_dev / zkp_selftest_miller_dev (pairing.hpp),
// a translation unit of their own.  pairing_tower.hpp instantiated over the saturated Fq.
#include "pairing.hpp"

#include "fq28_inv.hpp"

#define PT_FN __device__ inline
#define PT_NOINLINE __noinline__
#include "pairing_tower.hpp"

namespace zkp {

namespace {

__device__ __noinline__ Fq fq_inverse_call(const Fq& a) { return fq_inverse_gcd(a); }

// the adapter of pairing_tower.hpp over ff.hpp's Fq: canonical Montgomery residues, radix 2^384
struct DevFqOps {
    typedef Fq T;
    static ZKP_DEV T zero() { return Fq::zero(); }
    static ZKP_DEV T one() { return Fq::one(); }
    static ZKP_DEV T lit(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint64_t w4, uint64_t w5) {
        const uint64_t w[6] = {w0, w1, w2, w3, w4, w5};
        Fq r;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            r.l[2 * i] = (uint32_t)w[i];
            r.l[2 * i + 1] = (uint32_t)(w[i] >> 32);
        }
        return r;
    }
    static ZKP_DEV T add(const T& a, const T& b) { return a + b; }
    static ZKP_DEV T sub(const T& a, const T& b) { return a - b; }
    static ZKP_DEV T mul(const T& a, const T& b) { return a * b; }
    static ZKP_DEV T neg(const T& a) { return zkp::neg(a); }
    static ZKP_DEV T inverse(const T& a) { return fq_inverse_call(a); }
    static ZKP_DEV bool is_zero(const T& a) { return a.is_zero(); }
    static ZKP_DEV bool eq(const T& a, const T& b) { return a == b; }
};
typedef tower::Fq2<DevFqOps> D2;
typedef tower::Fq12<DevFqOps> D12;

// the 12 coefficients in memory order (arkworks: c0.c0.c0, c0.c0.c1, c0.c1.c0, ...), three 16-byte words each: word q of the
// element at base[q * q_stride]
ZKP_DEV Fq* f12_coeff(D12& a, int c) {
    D2* f[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
    return (c & 1) ? &f[c >> 1]->c1 : &f[c >> 1]->c0;
}
ZKP_DEV D12 f12_load(const uint4* base, uint64_t q_stride) {
    D12 r;
#pragma unroll
    for (int c = 0; c < 12; c++) {
        Fq* e = f12_coeff(r, c);
#pragma unroll
        for (int w = 0; w < 3; w++) {
            const uint4 v = base[(uint64_t)(3 * c + w) * q_stride];
            e->l[4 * w] = v.x; e->l[4 * w + 1] = v.y; e->l[4 * w + 2] = v.z; e->l[4 * w + 3] = v.w;
        }
    }
    return r;
}
ZKP_DEV void f12_store(D12& a, uint4* base, uint64_t q_stride) {
#pragma unroll
    for (int c = 0; c < 12; c++) {
        const Fq* e = f12_coeff(a, c);
#pragma unroll
        for (int w = 0; w < 3; w++)
            base[(uint64_t)(3 * c + w) * q_stride] = make_uint4(e->l[4 * w], e->l[4 * w + 1], e->l[4 * w + 2], e->l[4 * w + 3]);
    }
}

}  // namespace

// One lane per check.  Memory is indexed by the lane id, the pair number and the step only, never by a computed value.
__global__ __launch_bounds__(PAIRING_THREADS) void pairing_miller_kernel(const uint4* __restrict__ lines, uint32_t q_inf_mask, int k,
                                                                        const uint4* __restrict__ p_xy, const uint8_t* __restrict__ p_inf, uint64_t n,
                                                                        uint4* __restrict__ f_out, uint64_t q_stride, uint64_t i_stride) {
    const uint64_t i = (uint64_t)blockIdx.x * PAIRING_THREADS + threadIdx.x;
    if (i >= n) return;
    uint32_t live = 0;  // bit j: pair j contributes
    for (int j = 0; j < k; j++) {
        const bool dead = ((q_inf_mask >> j) & 1) || (p_inf && p_inf[i * k + j]);
        live |= dead ? 0u : 1u << j;
    }
    const uint4* p = p_xy + 6 * i * (uint64_t)k;  // pair j: x at [6 j], y at [6 j + 3]
    D12 f = tower::f12_one<DevFqOps>();
#pragma unroll 1
    for (int s = 0; s < PAIRING_STEPS; s++)
        tower::miller_step<DevFqOps>(
            f, s, k,
            [&](int j) {
                const uint4* l = lines + 12 * ((uint64_t)j * PAIRING_STEPS + s);
                return tower::PreparedLine<DevFqOps>{{Fq::load(l), Fq::load(l + 3)}, {Fq::load(l + 6), Fq::load(l + 9)}};
            },
            [&](int j) { return neg(Fq::load(p + 6 * j)); }, [&](int j) { return Fq::load(p + 6 * j + 3); },
            [&](int j) { return ((live >> j) & 1) != 0; });
    f = tower::f12_conj(f);
    f12_store(f, f_out + i * i_stride, q_stride);
}

__global__ __launch_bounds__(PAIRING_THREADS) void pairing_final_exp_kernel(const uint4* __restrict__ f_in, uint64_t stride, uint64_t n,
                                                                           uint8_t* __restrict__ ok, uint4* __restrict__ out_fq12) {
    const uint64_t i = (uint64_t)blockIdx.x * PAIRING_THREADS + threadIdx.x;
    if (i >= n) return;
    D12 e = tower::final_exp(f12_load(f_in + i, stride));
    if (ok) ok[i] = tower::f12_is_one(e) ? 1 : 0;
    if (out_fq12) f12_store(e, out_fq12 + PAIRING_F12_VEC * i, 1);
}

template <int OP>
__global__ __launch_bounds__(PAIRING_THREADS) void selftest_fq12_kernel(const uint4* __restrict__ pa, const uint4* __restrict__ pb, uint4* __restrict__ po,
                                                                       uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * PAIRING_THREADS + threadIdx.x;
    if (i >= n) return;
    const D12 a = f12_load(pa + PAIRING_F12_VEC * i, 1);
    D12 r;
    if constexpr (OP == ST_FQ12_MUL) r = tower::f12_mul(a, f12_load(pb + PAIRING_F12_VEC * i, 1));
    if constexpr (OP == ST_FQ12_SQR) r = tower::f12_sqr(a);
    if constexpr (OP == ST_FQ12_MUL_LINE) {
        const D12 b = f12_load(pb + PAIRING_F12_VEC * i, 1);
        r = tower::f12_mul_line(a, b.c0.c0, b.c0.c1, b.c1.c1.c0);
    }
    if constexpr (OP == ST_FQ12_INVERSE) r = tower::f12_inverse(a);
    if constexpr (OP == ST_FQ12_FROB1) r = tower::f12_frobenius<DevFqOps, 1>(a);
    if constexpr (OP == ST_FQ12_FROB2) r = tower::f12_frobenius<DevFqOps, 2>(a);
    if constexpr (OP == ST_FQ12_FROB3) r = tower::f12_frobenius<DevFqOps, 3>(a);
    if constexpr (OP == ST_FQ12_CYCLO_SQR) r = tower::f12_cyclotomic_sqr(a);
    if constexpr (OP == ST_FQ12_FINAL_EXP) r = tower::final_exp(a);
    f12_store(r, po + PAIRING_F12_VEC * i, 1);
}

namespace {
unsigned pairing_grid(uint64_t n) { return (unsigned)((n + PAIRING_THREADS - 1) / PAIRING_THREADS); }
template <int OP = 0>
bool launch_fq12(int op, dim3 grid, hipStream_t s, const uint4* a, const uint4* b, uint4* out, uint64_t n) {
    if constexpr (OP < ST_FQ12_OPS) {
        if (op != OP) return launch_fq12<OP + 1>(op, grid, s, a, b, out, n);
        hipLaunchKernelGGL((selftest_fq12_kernel<OP>), grid, dim3(PAIRING_THREADS), 0, s, a, b, out, n);
        return true;
    }
    return false;
}
}  // namespace

bool selftest_fq12_launch(int op, hipStream_t s, const void* a, const void* b, void* out, uint64_t n) {
    return launch_fq12(op, dim3(pairing_grid(n)), s, reinterpret_cast<const uint4*>(a), reinterpret_cast<const uint4*>(b), reinterpret_cast<uint4*>(out), n);
}
void pairing_miller_launch(hipStream_t s, const void* lines, uint32_t q_inf_mask, int k, const void* p_xy, const uint8_t* p_inf, uint64_t n, void* f_out,
                           uint64_t q_stride, uint64_t i_stride) {
    hipLaunchKernelGGL(pairing_miller_kernel, dim3(pairing_grid(n)), dim3(PAIRING_THREADS), 0, s, reinterpret_cast<const uint4*>(lines), q_inf_mask, k,
                       reinterpret_cast<const uint4*>(p_xy), p_inf, n, reinterpret_cast<uint4*>(f_out), q_stride, i_stride);
}
void pairing_final_exp_launch(hipStream_t s, const void* f, uint64_t stride, uint64_t n, uint8_t* ok, void* out_fq12) {
    hipLaunchKernelGGL(pairing_final_exp_kernel, dim3(pairing_grid(n)), dim3(PAIRING_THREADS), 0, s, reinterpret_cast<const uint4*>(f), stride, n, ok,
                       reinterpret_cast<uint4*>(out_fq12));
}

}  // namespace zkp
