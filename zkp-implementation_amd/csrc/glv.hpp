// glv.hpp -- the BLS12-381 G1 endomorphism phi(x, y) = (beta x, y) = [lambda](x, y) and the scalar split that goes with it.
//
// z = -0xd201000000010000, lambda = z^2 - 1 (127.43 bits), lambda^2 + lambda + 1 = r, so (r - 1) div lambda = lambda + 1.  A canonical
// scalar k < r splits by plain Euclidean division, k2 = k div lambda, k1 = k mod lambda: k1 < lambda and k2 <= lambda + 1, both below
// 0.674 * 2^128 -- no signs, no lattice rounding.  Then [k]P = [k1]P + phi([k2]P), which is what the endomorphism-split MSM
// (zkp_g1_bases_precompute_glv) uses: two 128-bit scalar vectors over planes that cover 129 bits instead of 256.
// beta is the cube root of unity in Fq that belongs to lambda (the other one belongs to lambda^2): tests/test_glv_cpu.py pins the pair.
//
// Plain C++17 without HIP, so that tests/host/glv_split.cpp checks it with g++ alone; under hipcc (ff.hpp included first) the same
// function is the one msm_digits_glv_kernel and zkp_selftest_glv_split_dev call.
#pragma once
#include <stdint.h>

namespace zkp {

#ifdef ZKP_HD
#define ZKP_GLV_FN ZKP_HD
#else
#define ZKP_GLV_FN inline
#endif

struct GlvParams {
    // lambda = 0xac45a4010001a40200000000ffffffff
    static constexpr uint32_t LAMBDA[4] = {0xffffffffu, 0x00000000u, 0x0001a402u, 0xac45a401u};
    // mu = floor(2^256 / lambda) = 0x17c6becf1e01faadd63f6e522f6cfee30 (129 bits)
    static constexpr uint32_t MU[5] = {0xf6cfee30u, 0x63f6e522u, 0xe01faaddu, 0x7c6becf1u, 0x00000001u};
    // beta, canonical, little-endian u64 limbs (the form HFq::load takes)
    static constexpr uint64_t BETA[6] = {0x8bfd00000000aaacULL, 0x409427eb4f49fffdULL, 0x897d29650fb85f9bULL,
                                         0xaa0d857d89759ad4ULL, 0xec02408663d4de85ULL, 0x1a0111ea397fe699ULL};
    static constexpr unsigned COVER_BITS = 129;  // slices of a half must cover this many bits: see msm_slice_offsets (msm_plan.hpp)
};

struct GlvHalves {
    uint32_t k1[4], k2[4];  // canonical, little-endian words
};

// k = k1 + lambda k2 for a canonical k < r (8 words).  Barrett: q = floor(k mu / 2^256) is k div lambda or one less (mu is rounded
// down, so k mu / 2^256 lies in (k / lambda - 1, k / lambda]); the remainder k - q lambda is then below 2 lambda < 2^129 and five words
// of it are exact.  Two corrective steps are written out, the second can only fire for an input that is not below r.
ZKP_GLV_FN GlvHalves glv_split(const uint32_t* k) {
    uint32_t t[13];
#pragma unroll
    for (int i = 0; i < 13; i++) t[i] = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 5; j++) {
            const uint64_t acc = (uint64_t)k[i] * GlvParams::MU[j] + t[i + j] + carry;
            t[i + j] = (uint32_t)acc;
            carry = acc >> 32;
        }
        t[i + 5] = (uint32_t)carry;
    }
    uint32_t q[4] = {t[8], t[9], t[10], t[11]};  // (t[12] = 0: q <= lambda + 1 < 2^128 for k < r)
    uint32_t m[5] = {0, 0, 0, 0, 0};             // q lambda mod 2^160
#pragma unroll
    for (int i = 0; i < 4; i++) {
        uint64_t carry = 0;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            if (i + j < 5) {
                const uint64_t acc = (uint64_t)q[i] * GlvParams::LAMBDA[j] + m[i + j] + carry;
                m[i + j] = (uint32_t)acc;
                carry = acc >> 32;
            }
        }
        if (i + 4 < 5) m[i + 4] = (uint32_t)carry;
    }
    uint32_t rem[5];
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < 5; i++) {
        c += (int64_t)k[i] - (int64_t)m[i];
        rem[i] = (uint32_t)c;
        c >>= 32;
    }
#pragma unroll
    for (int step = 0; step < 2; step++) {
        uint32_t d[5];
        int64_t b = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) {
            b += (int64_t)rem[i] - (int64_t)(i < 4 ? GlvParams::LAMBDA[i] : 0u);
            d[i] = (uint32_t)b;
            b >>= 32;
        }
        const bool ge = b == 0;  // no borrow: rem >= lambda
        uint64_t inc = ge ? 1u : 0u;
#pragma unroll
        for (int i = 0; i < 5; i++) rem[i] = ge ? d[i] : rem[i];
#pragma unroll
        for (int i = 0; i < 4; i++) {
            inc += q[i];
            q[i] = (uint32_t)inc;
            inc >>= 32;
        }
    }
    GlvHalves h;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        h.k1[i] = rem[i];
        h.k2[i] = q[i];
    }
    return h;
}

}  // namespace zkp
