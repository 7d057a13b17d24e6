// selftest.hpp -- lane-level self-test kernels for the field and curve primitives (zkp_selftest_*_dev in include/zkp_hip.h).
//
// One lane per case, raw limbs in and out, no conversion on the way: the tests feed operands at the edges of each primitive's
// documented contract (tests/test_gpu_field_selftest.py) and compare the output words with the exact limb model
// (tests/model/limb_model.py).  Memory is indexed by the lane id only, never by a computed value: a wrong arithmetic result can only
// produce wrong output words.  The kernels (one per operation, a template parameter) are a translation unit of their own, selftest.hip:
// the device code of api.hip -- every other kernel's instructions and register budget -- is the same with and without them (compiled into
// api.hip they moved the register counts of unrelated kernels).  This header is what the two files share: the operation numbers and the
// launchers.  One wave per workgroup: the asm product forms use the fixed VGPRs v164..v167.
//
// Field families: every lane reads a record of 4 operand slots of 16 words (64 words) and writes 2 result slots of 16 words (32 words,
// unused words zero).  An operand occupies the first words of its slot: 14 limbs (Fq28), 9 limbs (Fr29), 12 / 8 words (saturated Fq / Fr),
// 2 words (Goldilocks, low word first).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zkp {

constexpr int ST_THREADS = 64;
constexpr int ST_IN_WORDS = 64, ST_OUT_WORDS = 32;

enum StFq28Op : int {
    ST_FQ28_MUL_INLINE = 0,  // r0 = fq28_mul_inline(a, b)
    ST_FQ28_MUL_CHAIN = 1,   // r0 = fq28_mul_chain(a, b)
    ST_FQ28_MUL_CHAIN2 = 2,  // fq28_mul_chain2(a, b, c, d, r0, r1)
    ST_FQ28_SQR = 3,         // r0 = sqr(a)
    ST_FQ28_SQR_CHAIN = 4,   // r0 = fq28_sqr_chain(a)
    ST_FQ28_MUL2 = 5,        // r0 = fq28_mul2(a, b, c, d)
    ST_FQ28_MUL2_CHAIN = 6,  // r0 = fq28_mul2_chain(a, b, c, d)
    ST_FQ28_NORMALISE = 7,   // r0 = normalise(a)
    ST_FQ28_SUB4 = 8,        // r0 = sub4(a, b)
    ST_FQ28_SUB8 = 9,
    ST_FQ28_SUB16 = 10,
    ST_FQ28_SUB8W = 11,
    ST_FQ28_NEG4 = 12,       // r0 = neg4(a)
    ST_FQ28_IS_ZERO = 13,    // r0 word 0 = tight_is_zero_mod_p(a)
    ST_FQ28_FROM_SAT = 14,   // r0 = fq28_from_sat(first 12 words of slot a)
    ST_FQ28_MUL_CHAIN2_INPLACE = 15,  // fq28_mul_chain2_inplace(a, b, c, d); r0 = a, r1 = c
    ST_FQ28_OPS = 16
};
enum StFr29Op : int {
    ST_FR29_MUL = 0,            // r0 = a * b
    ST_FR29_MUL2 = 1,           // fr29_mul2(a, b, c, d, r0, r1)
    ST_FR29_TO_CANONICAL = 2,   // r0 (8 words) = fr29_to_canonical(a)
    ST_FR29_FR_MUL = 3,         // r0 (8 words) = Fr operator*(a, b) on 8-word memory-form operands
    ST_FR29_SUB_TIGHT = 4,
    ST_FR29_SUB_WIDE8 = 5,
    ST_FR29_NORMALISE = 6,
    ST_FR29_PACK_TIGHT = 7,     // r0 (8 words) = fr29_pack_tight(a)
    ST_FR29_FROM_SAT_SHL5 = 8,  // r0 = fr29_from_sat_shl5(8 words of slot a)
    ST_FR29_TWIDDLE = 9,        // r0 = fr29_twiddle_from_mont(8 words of slot a)
    ST_FR29_FROM_SAT = 10,
    ST_FR29_OPS = 11
};
enum StFpOp : int { ST_FP_ADD = 0, ST_FP_SUB = 1, ST_FP_NEG = 2, ST_FP_DBL = 3, ST_FP_MUL = 4 /* operator* */, ST_FP_MONT_MUL = 5, ST_FP_OPS = 6 };
enum StGlOp : int { ST_GL_ADD = 0, ST_GL_SUB = 1, ST_GL_NEG = 2, ST_GL_MUL = 3, ST_GL_REDUCE128 = 4 /* a = lo, b = hi */, ST_GL_OPS = 5 };
// G1.  Register forms: point i of an array is the 16 uint4 at [16 i] (X, Y, ZZ, ZZZ; an affine point is the first 8).  Stream and quad
// forms: plane-major, chunk q of point i at [q * stride + i].  flag[i]: the return value of mmadd, is_inf() of the result otherwise.
enum StG1Op : int {
    ST_G1_MADD = 0,             // out = a; g1_28_madd<false>(out, b)      (b affine)
    ST_G1_MADD_CHAIN = 1,
    ST_G1_MMADD = 2,            // out = a; flag = g1_28_mmadd<false>(out, b)
    ST_G1_MMADD_CHAIN = 3,
    ST_G1_ADD = 4,              // out = a; g1_28_add(out, b)
    ST_G1_DOUBLE = 5,           // out = g1_28_double(a)
    ST_G1_DOUBLE_AFFINE = 6,    // out = g1_28_double_affine(a)           (a affine)
    ST_G1_ADD_STREAM = 7,       // g1_28_add_stream<false>(a, b, out)
    ST_G1_ADD_STREAM_CHAIN = 8,
    ST_G1_ADD_INPLACE = 9,      // g1_28_add_stream_inplace<false>(out, b): the first operand is what `out` holds
    ST_G1_ADD_INPLACE_CHAIN = 10,
    ST_G1_ADD_QUAD = 11,        // four lanes per case: g1_28_add_quad(a, b, out, stride, lane & 3)
    ST_G1_ADD_QUAD_INPLACE = 12,  // g1_28_add_quad(out, b, out, ...)
    ST_G1_OPS = 13
};

// launchers (selftest.hip): false for an unknown operation number.  `blocks` workgroups of ST_THREADS lanes.
bool selftest_fq28_launch(int op, unsigned blocks, hipStream_t s, const void* in, void* out, uint64_t n);
bool selftest_fr29_launch(int op, unsigned blocks, hipStream_t s, const void* in, void* out, uint64_t n);
bool selftest_fp_launch(int field, int op, unsigned blocks, hipStream_t s, const void* in, void* out, uint64_t n);
bool selftest_gl_launch(int op, unsigned blocks, hipStream_t s, const void* in, void* out, uint64_t n);
bool selftest_g1_launch(int op, unsigned blocks, hipStream_t s, const void* a, const void* b, void* out, void* flag, uint64_t n, uint64_t stride);
// glv_split (glv.hpp) of n Fr in memory form: 8 words per case, k1 then k2
void selftest_glv_split_launch(unsigned blocks, hipStream_t s, const void* in, void* out, uint64_t n);

}  // namespace zkp
