// plane_div (csrc/msm_plan.hpp), the reciprocal division msm_accumulate_run locates the plane of an entry with, against `/`.
// g++ -std=c++17 -I zkp-implementation_amd/csrc tests/host/locate_div.cpp
#include <cstdint>
#include <cstdio>

#include "msm_plan.hpp"

using namespace zkp;

static uint64_t failures = 0, checked = 0;

static void check(const PlaneDiv& d, uint32_t pt) {
    const uint32_t got = plane_div(d, pt), want = pt / d.ns;
    checked++;
    if (got != want && failures++ < 10) printf("MISMATCH ns=%u pt=%u: got %u want %u\n", d.ns, pt, got, want);
}

int main() {
    const uint32_t TOP = 0x7fffffffu;  // entries and scalar counts stay below 2^31 (the sign of a digit is bit 31 of an entry)
    const uint32_t sizes[] = {1u, 2u, 3u, 1000u, 1024u, 65539u, (1u << 17) + 5u, 1u << 20, 1u << 24, TOP};
    uint64_t rng = 0x9e3779b97f4a7c15ull;
    for (uint32_t ns : sizes) {
        const PlaneDiv d = plane_div_make(ns);
        check(d, 0);
        check(d, ns - 1);
        check(d, ns);
        check(d, TOP);
        for (uint64_t k = 1; k <= 35; k++) {  // the plane boundaries of up to 35 planes
            for (int64_t o = -1; o <= 1; o++) {
                const int64_t pt = (int64_t)(k * ns) + o;
                if (pt >= 0 && pt <= (int64_t)TOP) check(d, (uint32_t)pt);
            }
        }
        for (int i = 0; i < 1000000; i++) {
            rng ^= rng << 13;
            rng ^= rng >> 7;
            rng ^= rng << 17;
            check(d, (uint32_t)(rng >> 33));
        }
    }
    printf("locate_div: %llu checks, %llu failures\n", (unsigned long long)checked, (unsigned long long)failures);
    return failures ? 1 : 0;
}
