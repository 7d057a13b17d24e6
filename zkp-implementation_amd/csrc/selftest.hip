// selftest.hip -- the lane-level self-test kernels behind zkp_selftest_*_dev (selftest.hpp), a translation unit of their own.
#include "selftest.hpp"

#include "fr29.hpp"
#include "g1_28.hpp"
#include "glv.hpp"

namespace zkp {

template <int OP>
__global__ __launch_bounds__(ST_THREADS) void selftest_fq28_kernel(const uint4* __restrict__ in, uint4* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint4* p = in + 16 * i;
    const Fq28 a = Fq28::load(p), b = Fq28::load(p + 4), c = Fq28::load(p + 8), d = Fq28::load(p + 12);
    Fq28 r0 = Fq28::zero(), r1 = Fq28::zero();
    if constexpr (OP == ST_FQ28_MUL_INLINE) r0 = fq28_mul_inline(a, b);
    if constexpr (OP == ST_FQ28_MUL_CHAIN) r0 = fq28_mul_chain(a, b);
    if constexpr (OP == ST_FQ28_MUL_CHAIN2) fq28_mul_chain2(a, b, c, d, r0, r1);
    if constexpr (OP == ST_FQ28_SQR) r0 = sqr(a);
    if constexpr (OP == ST_FQ28_SQR_CHAIN) r0 = fq28_sqr_chain(a);
    if constexpr (OP == ST_FQ28_MUL2) r0 = fq28_mul2(a, b, c, d);
    if constexpr (OP == ST_FQ28_MUL2_CHAIN) r0 = fq28_mul2_chain(a, b, c, d);
    if constexpr (OP == ST_FQ28_NORMALISE) r0 = normalise(a);
    if constexpr (OP == ST_FQ28_SUB4) r0 = sub4(a, b);
    if constexpr (OP == ST_FQ28_SUB8) r0 = sub8(a, b);
    if constexpr (OP == ST_FQ28_SUB16) r0 = sub16(a, b);
    if constexpr (OP == ST_FQ28_SUB8W) r0 = sub8w(a, b);
    if constexpr (OP == ST_FQ28_NEG4) r0 = neg4(a);
    if constexpr (OP == ST_FQ28_IS_ZERO) r0.l[0] = tight_is_zero_mod_p(a) ? 1u : 0u;
    if constexpr (OP == ST_FQ28_FROM_SAT) {
        Fq s;
#pragma unroll
        for (int w = 0; w < 12; w++) s.l[w] = a.l[w];
        r0 = fq28_from_sat(s);
    }
    if constexpr (OP == ST_FQ28_MUL_CHAIN2_INPLACE) {
        r0 = a;
        r1 = c;
        fq28_mul_chain2_inplace(r0, b, r1, d);
    }
    r0.store(out + 8 * i);
    r1.store(out + 8 * i + 4);
}

// the record of a lane as plain words (the families below)
struct StRec {
    uint32_t w[ST_IN_WORDS];
    uint32_t o[ST_OUT_WORDS];
    ZKP_DEV void load(const uint32_t* in, uint64_t i) {
#pragma unroll
        for (int j = 0; j < ST_IN_WORDS; j++) w[j] = in[ST_IN_WORDS * i + j];
#pragma unroll
        for (int j = 0; j < ST_OUT_WORDS; j++) o[j] = 0;
    }
    ZKP_DEV void store(uint32_t* out, uint64_t i) const {
#pragma unroll
        for (int j = 0; j < ST_OUT_WORDS; j++) out[ST_OUT_WORDS * i + j] = o[j];
    }
    template <class T, int N>
    ZKP_DEV T get(int slot) const {
        T r;
#pragma unroll
        for (int j = 0; j < N; j++) r.l[j] = w[16 * slot + j];
        return r;
    }
    template <class T, int N>
    ZKP_DEV void put(int slot, const T& v) {
#pragma unroll
        for (int j = 0; j < N; j++) o[16 * slot + j] = v.l[j];
    }
};

template <int OP>
__global__ __launch_bounds__(ST_THREADS) void selftest_fr29_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n) return;
    StRec t;
    t.load(in, i);
    const Fr29 a = t.get<Fr29, 9>(0), b = t.get<Fr29, 9>(1);
    const Fr sa = t.get<Fr, 8>(0), sb = t.get<Fr, 8>(1);
    if constexpr (OP == ST_FR29_MUL) t.put<Fr29, 9>(0, a * b);
    if constexpr (OP == ST_FR29_MUL2) {
        Fr29 r0, r1;
        fr29_mul2(a, b, t.get<Fr29, 9>(2), t.get<Fr29, 9>(3), r0, r1);
        t.put<Fr29, 9>(0, r0);
        t.put<Fr29, 9>(1, r1);
    }
    if constexpr (OP == ST_FR29_TO_CANONICAL) t.put<Fr, 8>(0, fr29_to_canonical(a));
    if constexpr (OP == ST_FR29_FR_MUL) t.put<Fr, 8>(0, sa * sb);
    if constexpr (OP == ST_FR29_SUB_TIGHT) t.put<Fr29, 9>(0, sub_tight(a, b));
    if constexpr (OP == ST_FR29_SUB_WIDE8) t.put<Fr29, 9>(0, sub_wide8(a, b));
    if constexpr (OP == ST_FR29_NORMALISE) t.put<Fr29, 9>(0, normalise(a));
    if constexpr (OP == ST_FR29_PACK_TIGHT) t.put<Fr, 8>(0, fr29_pack_tight(a));
    if constexpr (OP == ST_FR29_FROM_SAT_SHL5) t.put<Fr29, 9>(0, fr29_from_sat_shl5(sa));
    if constexpr (OP == ST_FR29_TWIDDLE) t.put<Fr29, 9>(0, fr29_twiddle_from_mont(sa));
    if constexpr (OP == ST_FR29_FROM_SAT) t.put<Fr29, 9>(0, fr29_from_sat(sa));
    t.store(out, i);
}

// saturated Fp<P>: canonical operands.  ST_FP_MUL is the product the kernels call (Fq: the out-of-line body; Fr: through 29-bit limbs),
// ST_FP_MONT_MUL the generic CIOS form.
template <class P, int OP>
__global__ __launch_bounds__(ST_THREADS) void selftest_fp_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n) return;
    StRec t;
    t.load(in, i);
    const Fp<P> a = t.get<Fp<P>, P::N>(0), b = t.get<Fp<P>, P::N>(1);
    Fp<P> r;
    if constexpr (OP == ST_FP_ADD) r = a + b;
    if constexpr (OP == ST_FP_SUB) r = a - b;
    if constexpr (OP == ST_FP_NEG) r = neg(a);
    if constexpr (OP == ST_FP_DBL) r = dbl(a);
    if constexpr (OP == ST_FP_MUL) r = a * b;
    if constexpr (OP == ST_FP_MONT_MUL) r = mont_mul<P>(a, b);
    t.put<Fp<P>, P::N>(0, r);
    t.store(out, i);
}

template <int OP>
__global__ __launch_bounds__(ST_THREADS) void selftest_gl_kernel(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n) return;
    StRec t;
    t.load(in, i);
    const uint64_t a = (uint64_t)t.w[0] | ((uint64_t)t.w[1] << 32), b = (uint64_t)t.w[16] | ((uint64_t)t.w[17] << 32);
    Gl r = Gl::zero();
    if constexpr (OP == ST_GL_ADD) r = Gl{a} + Gl{b};
    if constexpr (OP == ST_GL_SUB) r = Gl{a} - Gl{b};
    if constexpr (OP == ST_GL_NEG) r = neg(Gl{a});
    if constexpr (OP == ST_GL_MUL) r = Gl{a} * Gl{b};
    if constexpr (OP == ST_GL_REDUCE128) r = gl_reduce128(a, b);
    t.o[0] = (uint32_t)r.v;
    t.o[1] = (uint32_t)(r.v >> 32);
    t.store(out, i);
}

// pa / po may be the same array (the in-place forms and a caller that feeds results back): no __restrict__ on them
template <int OP>
__global__ __launch_bounds__(ST_THREADS) void selftest_g1_kernel(const uint4* pa, const uint4* __restrict__ pb, uint4* po, uint32_t* __restrict__ flag,
                                                               uint64_t n, uint64_t st) {
    const uint64_t t = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if constexpr (OP == ST_G1_ADD_QUAD || OP == ST_G1_ADD_QUAD_INPLACE) {
        const uint64_t e = t >> 2;  // a quad is wholly inside or wholly outside n: all four lanes stay active
        if (e >= n) return;
        g1_28_add_quad(OP == ST_G1_ADD_QUAD ? pa + e : po + e, pb + e, po + e, st, (int)(t & 3));
        if ((t & 3) == 0) flag[e] = 0;
        return;
    } else {
        const uint64_t i = t;
        if (i >= n) return;
        uint32_t f = 0;
        if constexpr (OP == ST_G1_ADD_STREAM) g1_28_add_stream<false>(pa + i, pb + i, po + i, st);
        if constexpr (OP == ST_G1_ADD_STREAM_CHAIN) g1_28_add_stream<true>(pa + i, pb + i, po + i, st);
        if constexpr (OP == ST_G1_ADD_INPLACE) g1_28_add_stream_inplace<false>(po + i, pb + i, st);
        if constexpr (OP == ST_G1_ADD_INPLACE_CHAIN) g1_28_add_stream_inplace<true>(po + i, pb + i, st);
        if constexpr (OP == ST_G1_MADD || OP == ST_G1_MADD_CHAIN || OP == ST_G1_MMADD || OP == ST_G1_MMADD_CHAIN) {
            X28 acc = X28::load(pa + 16 * i);
            const A28 q = A28::load(pb + 16 * i);
            if constexpr (OP == ST_G1_MADD) g1_28_madd<false>(acc, q);
            if constexpr (OP == ST_G1_MADD_CHAIN) g1_28_madd<true>(acc, q);
            if constexpr (OP == ST_G1_MMADD) f = g1_28_mmadd<false>(acc, q) ? 1u : 0u;
            if constexpr (OP == ST_G1_MMADD_CHAIN) f = g1_28_mmadd<true>(acc, q) ? 1u : 0u;
            if constexpr (OP == ST_G1_MADD || OP == ST_G1_MADD_CHAIN) f = acc.is_inf() ? 1u : 0u;
            acc.store(po + 16 * i);
        }
        if constexpr (OP == ST_G1_ADD) {
            X28 a = X28::load(pa + 16 * i);
            const X28 b = X28::load(pb + 16 * i);
            g1_28_add(a, b);
            f = a.is_inf() ? 1u : 0u;
            a.store(po + 16 * i);
        }
        if constexpr (OP == ST_G1_DOUBLE) {
            const X28 r = g1_28_double(X28::load(pa + 16 * i));
            f = r.is_inf() ? 1u : 0u;
            r.store(po + 16 * i);
        }
        if constexpr (OP == ST_G1_DOUBLE_AFFINE) {
            const X28 r = g1_28_double_affine(A28::load(pa + 16 * i));
            f = r.is_inf() ? 1u : 0u;
            r.store(po + 16 * i);
        }
        flag[i] = f;
    }
}

__global__ __launch_bounds__(ST_THREADS) void selftest_glv_split_kernel(const Fr* __restrict__ in, uint32_t* __restrict__ out, uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n) return;
    const Fr k = from_mont(Fr::load(in + i));
    const GlvHalves h = glv_split(k.l);
#pragma unroll
    for (int j = 0; j < 4; j++) {
        out[8 * i + j] = h.k1[j];
        out[8 * i + 4 + j] = h.k2[j];
    }
}

// the operation number picks the instantiation
namespace {
template <int OP = 0>
bool launch_fq28(int op, dim3 grid, hipStream_t s, const uint4* in, uint4* out, uint64_t n) {
    if constexpr (OP < ST_FQ28_OPS) {
        if (op != OP) return launch_fq28<OP + 1>(op, grid, s, in, out, n);
        hipLaunchKernelGGL((selftest_fq28_kernel<OP>), grid, dim3(ST_THREADS), 0, s, in, out, n);
        return true;
    }
    return false;
}
template <int OP = 0>
bool launch_fr29(int op, dim3 grid, hipStream_t s, const uint32_t* in, uint32_t* out, uint64_t n) {
    if constexpr (OP < ST_FR29_OPS) {
        if (op != OP) return launch_fr29<OP + 1>(op, grid, s, in, out, n);
        hipLaunchKernelGGL((selftest_fr29_kernel<OP>), grid, dim3(ST_THREADS), 0, s, in, out, n);
        return true;
    }
    return false;
}
template <class P, int OP = 0>
bool launch_fp(int op, dim3 grid, hipStream_t s, const uint32_t* in, uint32_t* out, uint64_t n) {
    if constexpr (OP < ST_FP_OPS) {
        if (op != OP) return launch_fp<P, OP + 1>(op, grid, s, in, out, n);
        hipLaunchKernelGGL((selftest_fp_kernel<P, OP>), grid, dim3(ST_THREADS), 0, s, in, out, n);
        return true;
    }
    return false;
}
template <int OP = 0>
bool launch_gl(int op, dim3 grid, hipStream_t s, const uint32_t* in, uint32_t* out, uint64_t n) {
    if constexpr (OP < ST_GL_OPS) {
        if (op != OP) return launch_gl<OP + 1>(op, grid, s, in, out, n);
        hipLaunchKernelGGL((selftest_gl_kernel<OP>), grid, dim3(ST_THREADS), 0, s, in, out, n);
        return true;
    }
    return false;
}
template <int OP = 0>
bool launch_g1(int op, dim3 grid, hipStream_t s, const uint4* a, const uint4* b, uint4* out, uint32_t* flag, uint64_t n, uint64_t st) {
    if constexpr (OP < ST_G1_OPS) {
        if (op != OP) return launch_g1<OP + 1>(op, grid, s, a, b, out, flag, n, st);
        hipLaunchKernelGGL((selftest_g1_kernel<OP>), grid, dim3(ST_THREADS), 0, s, a, b, out, flag, n, st);
        return true;
    }
    return false;
}
}  // namespace

bool selftest_fq28_launch(int op, unsigned blocks, hipStream_t s, const void* in, void* out, uint64_t n) {
    return launch_fq28(op, dim3(blocks), s, reinterpret_cast<const uint4*>(in), reinterpret_cast<uint4*>(out), n);
}
bool selftest_fr29_launch(int op, unsigned blocks, hipStream_t s, const void* in, void* out, uint64_t n) {
    return launch_fr29(op, dim3(blocks), s, reinterpret_cast<const uint32_t*>(in), reinterpret_cast<uint32_t*>(out), n);
}
bool selftest_fp_launch(int field, int op, unsigned blocks, hipStream_t s, const void* in, void* out, uint64_t n) {
    const uint32_t* i = reinterpret_cast<const uint32_t*>(in);
    uint32_t* o = reinterpret_cast<uint32_t*>(out);
    return field == 0 ? launch_fp<FqParams>(op, dim3(blocks), s, i, o, n) : launch_fp<FrParams>(op, dim3(blocks), s, i, o, n);
}
bool selftest_gl_launch(int op, unsigned blocks, hipStream_t s, const void* in, void* out, uint64_t n) {
    return launch_gl(op, dim3(blocks), s, reinterpret_cast<const uint32_t*>(in), reinterpret_cast<uint32_t*>(out), n);
}
bool selftest_g1_launch(int op, unsigned blocks, hipStream_t s, const void* a, const void* b, void* out, void* flag, uint64_t n, uint64_t stride) {
    return launch_g1(op, dim3(blocks), s, reinterpret_cast<const uint4*>(a), reinterpret_cast<const uint4*>(b), reinterpret_cast<uint4*>(out),
                     reinterpret_cast<uint32_t*>(flag), n, stride);
}

void selftest_glv_split_launch(unsigned blocks, hipStream_t s, const void* in, void* out, uint64_t n) {
    hipLaunchKernelGGL(selftest_glv_split_kernel, dim3(blocks), dim3(ST_THREADS), 0, s, reinterpret_cast<const Fr*>(in),
                       reinterpret_cast<uint32_t*>(out), n);
}

}  // namespace zkp
