// The endomorphism split on the host (csrc/glv.hpp, csrc/msm_plan.hpp), g++ only: tests/test_glv_cpu.py.
//   1. glv_split at the edges of its corrective steps and on 10^5 random scalars: k1 + lambda k2 = k and k1 < lambda (the Euclidean
//      division is unique, so the two conditions pin both halves), k2 <= lambda + 1
//   2. msm_slice_offsets: the 129-bit rule for every width 9..24, the 256-bit rule against the offsets spelled out in the header, and
//      the digit recoding of msm_digits (copied here) on both halves of every edge value: no carry out of the top slice
//   3. plan_msm over split planes: two bucket sets per MSM, 32 MSMs per batch, workspaces no smaller than a plain batch of 2 x count
// Also the program to run under -fsanitize=address,undefined.
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "glv.hpp"
#include "msm_plan.hpp"
using namespace zkp;

typedef unsigned __int128 u128;
struct U256 {
    uint64_t l[4];
};
static const u128 LAMBDA = ((u128)0xac45a4010001a402ULL << 64) | 0x00000000ffffffffULL;
static const U256 R_MOD = {{0xffffffff00000001ULL, 0x53bda402fffe5bfeULL, 0x3339d80809a1d805ULL, 0x73eda753299d7d48ULL}};

static U256 from128(u128 v) { return U256{{(uint64_t)v, (uint64_t)(v >> 64), 0, 0}}; }
static U256 add(const U256& a, const U256& b) {
    U256 r;
    u128 c = 0;
    for (int i = 0; i < 4; i++) {
        c += (u128)a.l[i] + b.l[i];
        r.l[i] = (uint64_t)c;
        c >>= 64;
    }
    return r;
}
static U256 sub(const U256& a, const U256& b) {
    U256 r;
    uint64_t borrow = 0;
    for (int i = 0; i < 4; i++) {
        const u128 d = (u128)a.l[i] - b.l[i] - borrow;
        r.l[i] = (uint64_t)d;
        borrow = (uint64_t)(d >> 64) & 1;
    }
    return r;
}
static U256 mul128(u128 a, u128 b) {  // 128 x 128 -> 256
    const uint64_t x[2] = {(uint64_t)a, (uint64_t)(a >> 64)}, y[2] = {(uint64_t)b, (uint64_t)(b >> 64)};
    uint64_t r[4] = {0, 0, 0, 0};
    for (int i = 0; i < 2; i++) {
        uint64_t carry = 0;
        for (int j = 0; j < 2; j++) {
            const u128 t = (u128)x[i] * y[j] + r[i + j] + carry;
            r[i + j] = (uint64_t)t;
            carry = (uint64_t)(t >> 64);
        }
        r[i + 2] = carry;
    }
    return U256{{r[0], r[1], r[2], r[3]}};
}
static U256 shl(uint64_t v, uint32_t by) {  // v * 2^by, by < 192
    U256 r = {{0, 0, 0, 0}};
    r.l[by / 64] = v << (by % 64);
    if (by % 64) r.l[by / 64 + 1] = v >> (64 - by % 64);
    return r;
}
static bool less(const U256& a, const U256& b) {
    for (int i = 3; i >= 0; i--)
        if (a.l[i] != b.l[i]) return a.l[i] < b.l[i];
    return false;
}
static bool equal(const U256& a, const U256& b) { return !less(a, b) && !less(b, a); }

static u128 half(const uint32_t* w) { return (u128)w[0] | (u128)w[1] << 32 | (u128)w[2] << 64 | (u128)w[3] << 96; }

// the edge values of the issue: 0, 1, lambda - 1 .. lambda + 1, m lambda - 1 .. m lambda + 1 for m = 2, 2^64, lambda - 1, lambda, lambda + 1
// (the last is r - 1), r - 1, r - 2
static std::vector<U256> edges() {
    std::vector<U256> v;
    const U256 one = from128(1);
    v.push_back(from128(0));
    v.push_back(one);
    for (u128 m : {(u128)1, (u128)2, (u128)1 << 64, LAMBDA - 1, LAMBDA, LAMBDA + 1}) {
        const U256 ml = mul128(m, LAMBDA);
        v.push_back(sub(ml, one));
        v.push_back(ml);
        if (less(add(ml, one), R_MOD)) v.push_back(add(ml, one));  // ((lambda + 1) lambda + 1 = r is no scalar)
    }
    v.push_back(sub(R_MOD, one));
    v.push_back(sub(R_MOD, from128(2)));
    return v;
}

static int check_split(const U256& k, const char* what) {
    uint32_t w[8];
    for (int i = 0; i < 8; i++) w[i] = (uint32_t)(k.l[i / 2] >> (32 * (i & 1)));
    const GlvHalves h = glv_split(w);
    const u128 k1 = half(h.k1), k2 = half(h.k2);
    const bool ok = equal(add(from128(k1), mul128(k2, LAMBDA)), k) && k1 < LAMBDA && k2 <= LAMBDA + 1;
    if (!ok) printf("glv_split wrong (%s): k = %016llx%016llx%016llx%016llx\n", what, (unsigned long long)k.l[3], (unsigned long long)k.l[2],
                    (unsigned long long)k.l[1], (unsigned long long)k.l[0]);
    return ok ? 0 : 1;
}

// msm_digits_kernel's recoding (csrc/msm.hpp, msm_recode) of a 128-bit value; returns the carry left after the top slice
static uint32_t recode(u128 v, const MsmSlices& s, std::vector<int64_t>* digits) {
    uint32_t k[8] = {(uint32_t)v, (uint32_t)(v >> 32), (uint32_t)(v >> 64), (uint32_t)(v >> 96), 0, 0, 0, 0};
    uint32_t carry = 0;
    digits->clear();
    for (uint32_t w = 0; w < s.planes; w++) {
        const uint32_t lo = s.off[w], width = (uint32_t)s.off[w + 1] - lo, limb = lo >> 5, sh = lo & 31;
        uint64_t x = 0;
        for (int q = 0; q < 8; q++) {
            if (q == (int)limb) x |= (uint64_t)k[q];
            if (q == (int)limb + 1) x |= (uint64_t)k[q] << 32;
        }
        const uint32_t u = ((uint32_t)(x >> sh) & ((1u << width) - 1)) + carry;
        if (u > (1u << (width - 1))) {
            digits->push_back(-(int64_t)((1u << width) - u));
            carry = 1;
        } else {
            digits->push_back(u);
            carry = 0;
        }
    }
    return carry;
}

static int check_slices() {
    int bad = 0;
    const std::vector<U256> ed = edges();
    for (uint32_t w = 9; w <= 24; w++) {
        const MsmSlices s = msm_slice_offsets(GlvParams::COVER_BITS, w, 1);
        uint32_t wmin = 99, wmax = 0;
        for (uint32_t k = 0; k < s.planes; k++) {
            const uint32_t width = (uint32_t)s.off[k + 1] - s.off[k];
            wmin = std::min(wmin, width), wmax = std::max(wmax, width);
        }
        if (s.planes != (129 + w - 1) / w || s.off[0] != 0 || s.off[s.planes] < 129 || wmax - wmin > 1 || wmax > s.widest || s.widest > w) {
            printf("129-bit slices wrong at %u bits: planes %u top %u widths %u..%u widest %u\n", w, s.planes, s.off[s.planes], wmin, wmax, s.widest);
            bad++;
        }
        for (const U256& k : ed) {
            uint32_t kw[8];
            for (int i = 0; i < 8; i++) kw[i] = (uint32_t)(k.l[i / 2] >> (32 * (i & 1)));
            const GlvHalves h = glv_split(kw);
            for (u128 v : {half(h.k1), half(h.k2)}) {
                std::vector<int64_t> d;
                const uint32_t carry = recode(v, s, &d);
                // reassemble: sum d_s 2^off[s] over the positive digits = v + the same over the negative ones
                U256 pos = from128(0), neg = from128(0);
                for (uint32_t q = 0; q < s.planes; q++) (d[q] < 0 ? neg : pos) = add(d[q] < 0 ? neg : pos, shl((uint64_t)(d[q] < 0 ? -d[q] : d[q]), s.off[q]));
                const bool ok = carry == 0 && equal(pos, add(neg, from128(v)));
                if (!ok) {
                    printf("recoding wrong at %u bits: carry %u\n", w, carry);
                    bad++;
                }
            }
        }
    }
    // the examples of the issue and of include/zkp_hip.h
    const MsmSlices s22 = msm_slice_offsets(129, 22, 1), s20 = msm_slice_offsets(129, 20, 1);
    const uint16_t e22[7] = {0, 22, 44, 66, 87, 108, 129}, e20[8] = {0, 19, 38, 57, 75, 93, 111, 129};
    if (s22.planes != 6 || memcmp(s22.off, e22, sizeof e22) || s20.planes != 7 || s20.widest != 19 || memcmp(s20.off, e20, sizeof e20) ||
        msm_slice_offsets(129, 16, 1).planes != 9 || msm_slice_offsets(129, 12, 1).planes != 11) {
        printf("129-bit examples wrong\n");
        bad++;
    }
    // 256 bits: what zkp_g1_bases_precompute has always produced (include/zkp_hip.h: 16 tiles exactly, 19 -> 14 slices of 18/19,
    // 20 -> 13 of 19/20, 22 -> 12 of 21/22)
    const uint16_t p16[17] = {0, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240, 256};
    const uint16_t p19[15] = {0, 19, 38, 57, 76, 94, 112, 130, 148, 166, 184, 202, 220, 238, 256};
    const uint16_t p20[14] = {0, 20, 40, 60, 80, 100, 120, 140, 160, 180, 199, 218, 237, 256};
    const uint16_t p22[13] = {0, 22, 44, 66, 88, 109, 130, 151, 172, 193, 214, 235, 256};
    struct { uint32_t w, planes, widest; const uint16_t* off; } plain[] = {{16, 16, 16, p16}, {19, 14, 19, p19}, {20, 13, 20, p20}, {22, 12, 22, p22}};
    for (const auto& e : plain) {
        const MsmSlices s = msm_slice_offsets(256, e.w, 1);
        if (s.planes != e.planes || s.widest != e.widest || memcmp(s.off, e.off, 2 * (e.planes + 1))) {
            printf("256-bit slices wrong at %u bits\n", e.w);
            bad++;
        }
    }
    // ZKP_MSM_BALANCE_FROM above the overshoot: uniform slices, as before
    const MsmSlices u20 = msm_slice_offsets(256, 20, 8);
    if (u20.planes != 13 || u20.widest != 20 || u20.off[13] != 260) bad++, printf("uniform slices wrong\n");
    return bad;
}

static int check_plans() {
    int bad = 0;
    const struct { uint64_t n; uint32_t w; } sizes[] = {{64, 12}, {1u << 12, 14}, {1u << 20, 20}};
    for (const auto& sz : sizes) {
        const MsmSlices s = msm_slice_offsets(GlvParams::COVER_BITS, sz.w, 1);
        for (size_t count : {1, 3, 32, 33}) {
            MsmBases split{sz.n, s.widest, s.planes, s.off, 1}, plain{sz.n, s.widest, s.planes, s.off, 0};
            MsmPlan a, b;
            const int rc = plan_msm(split, count, sz.n, nullptr, 2048, &a);
            if (count == 33) {
                if (rc != ZKP_E_ARG || !strstr(a.error, "32 MSMs")) bad++, printf("a batch of 33 was not refused\n");
                continue;
            }
            if (rc != ZKP_OK || plan_msm(plain, 2 * count, sz.n, nullptr, 2048, &b) != ZKP_OK) {
                printf("plan refused: n %llu count %zu\n", (unsigned long long)sz.n, count);
                bad++;
                continue;
            }
            const size_t *x = &a.bytes.digits, *y = &b.bytes.digits;
            bool ok = a.g.nwin == 2 * count && a.g.glv == 1 && b.g.glv == 0 && a.g.n == b.g.n && a.g.n == (uint64_t)s.planes * a.range &&
                      a.nwin1 == s.planes && a.g.nb == 1u << (s.widest - 1);
            for (size_t k = 0; k < sizeof(MsmSizes) / sizeof(size_t); k++) ok = ok && x[k] >= y[k];
            if (!ok) bad++, printf("split plan wrong: n %llu count %zu\n", (unsigned long long)sz.n, count);
        }
    }
    return bad;
}

int main(int argc, char** argv) {
    int bad = 0, cases = 0;
    for (const U256& k : edges()) bad += check_split(k, "edge"), cases++;
    const int nrand = argc > 1 ? atoi(argv[1]) : 100000;
    std::mt19937_64 g(0x61c);
    for (int it = 0; it < nrand;) {
        U256 k{{g(), g(), g(), g() >> 1}};
        if (!less(k, R_MOD)) continue;
        bad += check_split(k, "random"), cases++, it++;
    }
    printf("glv_split: %d cases, %d failures\n", cases, bad);
    const int bs = check_slices();
    printf("slices: %d failures\n", bs);
    const int bp = check_plans();
    printf("plans: %d failures\n", bp);
    return bad || bs || bp ? 1 : 0;
}
