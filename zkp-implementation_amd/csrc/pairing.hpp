// pairing.hpp -- pairing-product checks on the GPU, one lane per check (zkp_pairing_check_batch* in include/zkp_hip.h).  This header is
// what api.hip and pairing.hip share: the sizes, the operation numbers of the self-test and the launchers.  The kernels are a
// translation unit of their own (pairing.hip), as the self-test kernels are: the device code of api.hip is the same with and
// without them.
//
// A check c is  prod_j e(P[c][j], Q_j) == 1  over k FIXED G2 points.  Their Miller walks are done once on the host
// (pairing_host.hpp prepare_g2_lines): per point 68 line steps of (lambda, lambda x_T - y_T), 272 Fq = 13056 bytes, uploaded at
// creation.  The device never touches G2 arithmetic or an inversion inside the loop:
//   pairing_miller_kernel     f = 1; per step: f <- f^2 once for the whole check (a doubling step), then f <- f * line_j(P_j) for every
//                             live pair -- the product of the k Miller functions shares its squarings.  Ends with conj.  The value is,
//                             bit for bit, the product of pairing_model.miller_loop(P_j, Q_j).
//   pairing_final_exp_kernel  E(f) = f^(3 (p^12 - 1) / r) by the x-chain of pairing_tower.hpp, then the verdict byte (E == 1) and,
//                             when asked, the 12 coefficients.  E IS THE CUBE OF WHAT zkp_pairing RETURNS (pairing_tower.hpp).
// Both instantiate pairing_tower.hpp over the saturated Fq of ff.hpp (exact, canonical, the ABI's memory form: no conversions).
//
// One lane per check means one check costs what a whole wave of them costs, and a single device check is SLOWER than the host's
// (profiles/pairing_dev.md): the entries here are for many independent checks.  The existing verifiers keep their host check.
//
// Registers: an Fq12 is 144 VGPRs.  Every tower operation from the Fq2 product up is a real call (PT_NOINLINE), operands by reference
// to the lane's private memory, so the Fq12 values live in the lane's stack frame (scratch memory, which the hardware interleaves
// lane-minor: adjacent lanes touch adjacent words) and not in registers.  The kernels' register counts are the maximum over that
// call graph -- close to the whole file of 512, so one wave per SIMD, and kilobytes of scratch per lane: the tools/kernel_regs.py figures
// are in profiles/pairing_dev.md.  Between the two kernels f travels coefficient-major, lane-minor: 16-byte word q of check i at
// [q * stride + i].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace zkp {

constexpr int PAIRING_THREADS = 64;
constexpr int PAIRING_MAX_K = 8;
constexpr int PAIRING_STEPS = 68;
constexpr size_t PAIRING_LINE_WORDS = 68 * 24;         // u64 words of one prepared G2 point
constexpr size_t PAIRING_LINE_BYTES = 8 * PAIRING_LINE_WORDS;
constexpr size_t PAIRING_F12_BYTES = 576;              // 12 Fq
constexpr size_t PAIRING_F12_VEC = 36;                 // as 16-byte words

enum StFq12Op : int {
    ST_FQ12_MUL = 0,        // out = a * b
    ST_FQ12_SQR = 1,        // out = a^2
    ST_FQ12_MUL_LINE = 2,   // out = a * line, the line read from b: (A, B, C) = (b.c0.c0, b.c0.c1, b.c1.c1.c0)
    ST_FQ12_INVERSE = 3,    // out = 1 / a (0 -> 0)
    ST_FQ12_FROB1 = 4,      // out = a^p
    ST_FQ12_FROB2 = 5,
    ST_FQ12_FROB3 = 6,
    ST_FQ12_CYCLO_SQR = 7,  // Granger-Scott squaring (the square only for a in the cyclotomic subgroup)
    ST_FQ12_FINAL_EXP = 8,  // out = E(a)
    ST_FQ12_OPS = 9
};

// launchers (pairing.hip).  Operands of the self-test: n x 72 limbs each, arkworks memory order.
bool selftest_fq12_launch(int op, hipStream_t s, const void* a, const void* b, void* out, uint64_t n);
// lines: k x PAIRING_LINE_WORDS; q_inf_mask bit j: Q_j is the identity.  p_xy: n x k x 12 limbs, p_inf: n x k flags or null.
// f_out word q of check i at [q * q_stride + i * i_stride]  (workspace: q_stride = the lane stride, i_stride = 1; ABI: 1 and 36)
void pairing_miller_launch(hipStream_t s, const void* lines, uint32_t q_inf_mask, int k, const void* p_xy, const uint8_t* p_inf, uint64_t n,
                           void* f_out, uint64_t q_stride, uint64_t i_stride);
// f as the Miller kernel left it in the workspace (stride); ok and out_fq12 (n x 72 limbs) nullable
void pairing_final_exp_launch(hipStream_t s, const void* f, uint64_t stride, uint64_t n, uint8_t* ok, void* out_fq12);

}  // namespace zkp
