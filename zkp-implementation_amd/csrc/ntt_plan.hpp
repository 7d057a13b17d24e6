// ntt_plan.hpp -- the shape of a transform (ntt_host.inc): the per-field constants of the pass kernels (NttOps<F> inherits them), how
// many passes of which radix, the geometry of every launch and the tables it reads.  Pure arithmetic on (field, log_n, allow_wide, knob
// values): plain C++17 without HIP and without the environment, so that tests/host/ntt_plan_table.cpp checks it with g++ alone.  Also
// the two index maps that the kernels of ntt.hpp share with the plan of the sharded transform (ntt_shard_plan.hpp): NttRemap and
// PermuteSpec; under hipcc (ff.hpp included first) the kernels call the same functions.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace zkp {

#ifdef ZKP_HD
#define ZKP_NTTPLAN_FN ZKP_HD
#else
#define ZKP_NTTPLAN_FN inline
#endif

#ifndef ZKP_GL_LOG_T
#define ZKP_GL_LOG_T 4
#endif
#ifndef ZKP_GL_THREADS
#define ZKP_GL_THREADS 512
#endif
#ifndef ZKP_GL_MAX_PASS_LOG
#define ZKP_GL_MAX_PASS_LOG 9
#endif
struct NttFrConsts {
    static constexpr int MAX_PASS_LOG = 8;   // radix of one pass of a multi-pass transform (2^9: 72 KiB tiles, one workgroup
                                             // per CU -- 2^26 in three passes measured 12.8 ms against 10.9 ms in four)
    static constexpr int THREADS = 256;      // workgroup size of the pass kernels
    static constexpr int LOG_T = 2;          // 4 x 32 B = 128 B runs (one cache line); 1024-element tiles = 36 KiB of
                                             // LDS, so 4 workgroups (4 waves/SIMD) fit a CU
    static constexpr int MAX_TILE_LOG = 11;  // single-pass limit: 2048 elements x 36 B = 72 KiB of LDS
    // A radix-2^9 pass with tiles of TWO columns (64-byte runs, the same 36 KiB of LDS and one element-quad per thread as a radix-2^8
    // pass with four columns) and a radix-2^10 pass with single-column tiles (32-byte runs), where they save a whole pass (plan_ntt)
    static constexpr int WIDE_PASS_LOG = 10;
    static constexpr int log_t_of(int log_r) { return log_r <= MAX_PASS_LOG ? LOG_T : log_r == 9 ? 1 : 0; }
    // largest transform a wide radix is used for: 2^9 always, 2^10 (32-byte runs) only while the data is cache-resident
    static constexpr int wide_max_log_n(int log_r) { return log_r <= 9 ? 64 : 20; }
    static constexpr int PAD = 0;            // 36-byte elements already spread over the LDS banks
    static constexpr bool PASS0_MATRIX = true;  // see pass0_uses_matrix
    static constexpr size_t ELEM_BYTES = 36, TW_BYTES = 36;  // an element in LDS (NttOps::E: nine 29-bit limbs) and a twiddle (NttOps::W)
};
struct NttGlConsts {
    // 16 x 8 B = 128 B runs; radix <= 2^9 so that 2^26 takes three passes (64 KiB tiles); 512 threads keep enough loads
    // in flight per tile.  Measured 2^20 / 2^24 / 2^26: (T 32, radix 2^8, 256 threads) 0.068 / 0.567 / 2.04 ms,
    // (16, 2^8, 512) 0.045 / 0.417 / 2.18, (16, 2^9, 512) 0.045 / 0.430 / 1.82, (16, 2^9, 1024) 0.048 / 0.451 / 1.75.
    static constexpr int LOG_T = ZKP_GL_LOG_T;
    static constexpr int MAX_PASS_LOG = ZKP_GL_MAX_PASS_LOG;
    static constexpr int THREADS = ZKP_GL_THREADS;
    static constexpr int MAX_TILE_LOG = 13;  // 8192 elements = 64 KiB
    // no wider radices for Goldilocks: radix 2^10 / 2^11 with 8 / 4-column tiles (two passes instead of three for 2^19 .. 2^22)
    // measured slower at every size (2^19 0.033 -> 0.060 ms, 2^22 0.112 -> 0.129 ms: the padded last-pass tile grows to 73 / 82 KiB
    // and the runs shrink to 64 / 32 bytes; profiles/r02_l_ntt_wide_pass.md)
    static constexpr int WIDE_PASS_LOG = MAX_PASS_LOG;
    static constexpr int log_t_of(int) { return LOG_T; }
    static constexpr int wide_max_log_n(int) { return 0; }
    static constexpr int PAD = 1;            // +1 element per row keeps the transposing LDS writes conflict-light
    static constexpr bool PASS0_MATRIX = false;  // memory-bound: a product is cheaper than 8 more bytes per element
    static constexpr size_t ELEM_BYTES = 8, TW_BYTES = 8;
};

// One launch of ntt_pass_strided: view [2^log_outer][2^log_r][inner], one workgroup per tile of 2^log_r x 2^log_t elements
struct NttStridedShape {
    uint32_t log_r, log_outer, log_t;
    uint64_t inner, tiles;
    size_t lds;           // bytes: the tile and the radix twiddles
    uint64_t direct_len;  // != 0: the inter-pass twiddles omega_M^e come from a direct table of M entries, not from the two-level table of omega_N
};
template <class C>
NttStridedShape strided_shape(uint64_t total, uint32_t log_r, uint32_t log_outer, uint64_t inner, int log_t) {
    const size_t R = (size_t)1 << log_r;
    return NttStridedShape{log_r, log_outer, (uint32_t)log_t, inner, (total >> log_r) >> log_t, C::ELEM_BYTES * (R << log_t) + C::TW_BYTES * (R / 2), 0};
}

struct NttShape {
    unsigned log_n;
    int passes, r[4];       // log_n = r[0] + .. + r[passes-1]
    uint32_t h, nlo, nhi;   // multi-pass: the two-level table omega_N^e = lo[e & (2^h - 1)] * hi[e >> h] and its sizes
    bool lo_ninv;           // ... and a second lo table times 1/n (inverse plans: pass 0 applies the 1/n for free)
    NttStridedShape strided[3];  // passes 0 .. passes-2
    struct { uint32_t log_r, log_r0, log_m, log_r1, t_log; size_t stride, lds; uint64_t tiles; } last;  // NttLastParams, ntt_pass_last
};

// Pass 0 of a multi-pass transform reads its inter-pass twiddles omega_N^(k_0 i) from a matrix shaped like the data ([k_0][i], one
// coalesced 32-byte load per element) instead of forming each one as the product of a low and a high table entry: one field product
// less per element, 2-4.5 % of a transform up to 2^24 = matrix_max_log's default (KNOB_NTT_TW_MATRIX_MAX_LOG, read per call); above,
// 1 % for 1 GiB and more per direction is not worth the memory (profiles/r02_m_ntt_twiddle_matrix.md)
template <class C>
bool pass0_uses_matrix(unsigned log_n, int passes, unsigned matrix_max_log) { return passes > 1 && C::PASS0_MATRIX && log_n <= matrix_max_log; }

// A transform of 2^log_n elements.  allow_wide: the launch has at least 2^19 elements; no_wide: the value of KNOB_NTT_NO_WIDE_PASS
template <class C>
NttShape plan_ntt(unsigned log_n, int inverse, bool allow_wide, bool no_wide) {
    NttShape s{};
    s.log_n = log_n;
    s.passes = (int)log_n <= C::MAX_TILE_LOG ? 1 : (int)((log_n + C::MAX_PASS_LOG - 1) / C::MAX_PASS_LOG);
    // wide passes where they save a whole pass: 2^25 5.84 -> 4.42 ms, fifteen 2^18 transforms 2.11 -> 1.98 ms (profiles/r02_l_ntt_wide_pass.md).
    // Not for a lone small transform: 2^17 would be 128 tiles on 256 CUs (0.047 against 0.042 ms), hence allow_wide.
    if (s.passes > 1 && allow_wide && !no_wide) {
        for (int maxr = C::MAX_PASS_LOG + 1; maxr <= C::WIDE_PASS_LOG; maxr++) {  // the narrowest radix that saves a pass
            if ((int)log_n > C::wide_max_log_n(maxr)) break;  // radix 2^10: 2^19 0.102 -> 0.092 ms, but 2^28 45.1 -> 48.3 ms
            s.passes = std::min(s.passes, (int)((log_n + maxr - 1) / maxr));
        }
    }
    const int P = s.passes, base = (int)log_n / P, rem = (int)log_n % P;
    for (int p = 0; p < P; p++) s.r[p] = base + (p < rem ? 1 : 0);
    if (P > 1) {
        s.h = (log_n + 1) / 2;
        s.nlo = 1u << s.h;
        s.nhi = 1u << (log_n - s.h);
        s.lo_ninv = inverse != 0;
    }
    uint32_t log_outer = 0;
    for (int p = 0; p + 1 < P; log_outer += s.r[p++]) {
        s.strided[p] = strided_shape<C>(1ull << log_n, s.r[p], log_outer, (1ull << log_n) >> (log_outer + s.r[p]), C::log_t_of(s.r[p]));
        // passes 1 .. P-2 work on sub-problems of size M_p = n >> (r_0 + .. + r_{p-1}): a direct table up to 2^17
        if (p > 0 && log_n - log_outer <= 17) s.strided[p].direct_len = 1ull << (log_n - log_outer);
    }
    auto& l = s.last;
    l.log_r = s.r[P - 1];
    l.log_r0 = P > 1 ? s.r[0] : 0;
    for (int p = 1; p + 1 < P; p++) l.log_m += s.r[p];
    l.log_r1 = P == 4 ? s.r[1] : l.log_m;
    l.t_log = std::min<uint32_t>((uint32_t)C::log_t_of((int)l.log_r), l.log_r0);
    const size_t R = (size_t)1 << l.log_r, T = (size_t)1 << l.t_log;
    l.stride = T > 1 ? T + C::PAD : 1;
    l.lds = C::ELEM_BYTES * (R * l.stride) + C::TW_BYTES * (R / 2);
    l.tiles = (1ull << (l.log_r0 - l.t_log)) << l.log_m;
    return s;
}

// Transforms of length 2^log_len along axis 0 of a row-major matrix [2^log_len][cols] (run_ntt_axis0): one or two strided passes,
// the last one over rows that are 2^log_outer apart
struct NttAxis0Shape {
    const char* error;  // the message of a refusal, else null
    int passes;
    uint32_t col_bits;
    NttStridedShape pass[2];
};
template <class C>
NttAxis0Shape plan_ntt_axis0(unsigned log_len, size_t cols) {
    NttAxis0Shape s{};
    if (log_len == 0 || log_len > 2 * (unsigned)C::MAX_PASS_LOG) return s.error = "axis-0 transform length out of range", s;
    if (cols == 0 || (cols & (cols - 1)) || cols < (1u << C::LOG_T)) return s.error = "cols must be a power of two >= 4", s;
    while ((1ull << s.col_bits) < cols) s.col_bits++;
    const uint64_t total = (uint64_t)cols << log_len;
    s.passes = log_len <= (unsigned)C::MAX_PASS_LOG ? 1 : 2;
    const uint32_t r0 = s.passes == 1 ? log_len : (log_len + 1) / 2, r1 = log_len - r0;
    s.pass[0] = strided_shape<C>(total, r0, 0, (uint64_t)cols << r1, C::LOG_T);
    if (s.passes == 2) s.pass[1] = strided_shape<C>(total, r1, r0, cols, C::LOG_T);
    return s;
}

// The twiddle of a four-step transform multiplies element k of row (column) first + i by omega_{2^tw_log_n}^((first + i) k): its
// exponent (first + count - 1) * (2^log_len - 1) must stay below 2^tw_log_n.  tw_log_n == 0: no twiddle.
inline bool four_step_exponent_ok(unsigned tw_log_n, uint64_t first, uint64_t count, unsigned log_len) {
    return tw_log_n <= 32 && (tw_log_n == 0 || (((first + count - 1) * ((1ull << log_len) - 1)) >> tw_log_n) == 0);
}

// Gathered input layout (first pass of a transform only): logical element e of transform b lives at physical element
//   b * batch_stride + (e mod 2^lo_bits) + ((e >> lo_bits) mod 2^mid_bits) * mid_stride + (e >> (lo_bits + mid_bits)) * hi_stride.
// This is how the row transforms of the multi-GPU four-step NTT read what the all-to-all delivered -- [source rank][my row]
// [that rank's columns] blocks, possibly in several column chunks -- without a transpose pass (zkp_hip/dist.py).
struct NttRemap {
    uint32_t on;  // 0: contiguous transforms, element e of transform b at b * n + e
    uint32_t lo_bits, mid_bits;
    uint64_t mid_stride, hi_stride, batch_stride;
};
ZKP_NTTPLAN_FN uint64_t ntt_phys(const NttRemap& r, uint64_t b, uint64_t n, uint64_t e) {
    if (!r.on) return b * n + e;
    const uint64_t lo = e & ((1ull << r.lo_bits) - 1), rest = e >> r.lo_bits;
    return b * r.batch_stride + lo + (rest & ((1ull << r.mid_bits) - 1)) * r.mid_stride + (rest >> r.mid_bits) * r.hi_stride;
}

// Index permutation of 32-byte elements between two strided views of up to four power-of-two dimensions (most significant
// first): element (i0, i1, i2, i3) moves from in[sum i_k in_stride_k] to out[sum i_k out_stride_k] (fr_permute_kernel, ntt.hpp)
struct PermuteSpec {
    uint32_t bits[4];
    uint64_t in_stride[4], out_stride[4];  // in elements
};
struct PermuteIndex {
    uint64_t src, dst;
};
ZKP_NTTPLAN_FN PermuteIndex permute_index(const PermuteSpec& s, uint64_t e) {  // e < 2^(bits[0] + .. + bits[3])
    PermuteIndex x = {0, 0};
    for (int d = 3; d >= 0; d--) {
        const uint64_t i = e & ((1ull << s.bits[d]) - 1);
        e >>= s.bits[d];
        x.src += i * s.in_stride[d];
        x.dst += i * s.out_stride[d];
    }
    return x;
}

}  // namespace zkp
