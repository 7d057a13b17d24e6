// csrc/g1_ntt_plan.hpp on its own, g++ only (tests/test_g1_ntt_cpu.py builds it with -fsanitize=address,undefined):
//   g1_ntt_plan              every log_n 0..24: each stage takes every pair of points exactly once, the load maps and the opener's
//                            slot maps are what the construction needs, workspace sizes and launch splits agree; for log_n <= 8 the
//                            staged transform over F_257 (which has 256-th roots of unity) equals the definition, both directions
//   g1_ntt_plan dump LOG_N   the tables of one size as text, for the comparison with tests/model/g1_ntt_model.py
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "g1_ntt_plan.hpp"
using namespace zkp;

static int fails = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            if (fails++ < 20) {          \
                printf("FAIL " __VA_ARGS__); \
                printf("\n");            \
            }                            \
        }                                \
    } while (0)

static const uint32_t P = 257;
static uint32_t powmod(uint32_t b, uint32_t e) {
    uint32_t r = 1;
    for (b %= P; e; e >>= 1, b = b * b % P)
        if (e & 1) r = r * b % P;
    return r;
}

// the kernels' order of operations over F_257: bit-reversed load, stages in place, n^-1 in the last stage of an inverse
static std::vector<uint32_t> staged(const std::vector<uint32_t>& in, unsigned log_n, bool inverse) {
    const uint32_t n = 1u << log_n;
    uint32_t w = powmod(3, 256 >> log_n);  // 3 generates F_257^*
    if (inverse) w = powmod(w, P - 2);
    const G1NttLoadMap map = g1_ntt_load_plain(log_n);
    std::vector<uint32_t> v(n);
    for (uint32_t i = 0; i < n; i++) v[map.rev_log ? g1_ntt_bitrev(i, map.rev_log) : i] = in[(size_t)g1_ntt_load_source(map, i)];
    const uint32_t ninv = inverse ? powmod(n, P - 2) : 1;
    for (unsigned s = 0; s < log_n; s++) {
        const uint32_t c = s == log_n - 1 ? ninv : 1;
        for (uint32_t i = 0; i < n / 2; i++) v[i] = v[i] * c % P;
        for (uint32_t i = 0; i < n / 2; i++) {
            const G1NttButterfly b = g1_ntt_butterfly(log_n, s, i);
            const uint32_t t = v[b.hi] * (c * powmod(w, b.exp) % P) % P;
            const uint32_t a = v[b.lo];
            v[b.lo] = (a + t) % P;
            v[b.hi] = (a + P - t) % P;
        }
    }
    return v;
}

static void check_transform(unsigned log_n) {
    const uint32_t n = 1u << log_n;
    std::vector<uint32_t> in(n);
    uint32_t x = 12345 + log_n;
    for (uint32_t& e : in) e = (x = x * 1103515245u + 12345u) % P;
    for (int inverse = 0; inverse < 2; inverse++) {
        uint32_t w = powmod(3, 256 >> log_n);
        if (inverse) w = powmod(w, P - 2);
        const std::vector<uint32_t> got = staged(in, log_n, inverse != 0);
        for (uint32_t i = 0; i < n; i++) {
            uint32_t sum = 0;
            for (uint32_t j = 0; j < n; j++) sum = (sum + powmod(w, (uint32_t)((uint64_t)i * j % 256)) * in[j]) % P;
            if (inverse) sum = sum * powmod(n, P - 2) % P;
            CHECK(got[i] == sum, "transform log_n=%u inverse=%d output %u: %u != %u", log_n, inverse, i, got[i], sum);
        }
    }
}

static void check_size(unsigned log_n) {
    const uint64_t n = (uint64_t)1 << log_n;
    std::vector<uint8_t> seen(n);
    for (unsigned s = 0; s < log_n; s++) {
        std::fill(seen.begin(), seen.end(), 0);
        const uint32_t half = 1u << s;
        bool ok = true;
        for (uint32_t i = 0; i < n / 2; i++) {
            const G1NttButterfly b = g1_ntt_butterfly(log_n, s, i);
            if (b.hi >= n || b.hi != b.lo + half || (b.lo & half) || b.exp >= n / 2 || b.exp != ((b.lo & (half - 1)) << (log_n - 1 - s)) ||
                seen[b.lo] || seen[b.hi]) {
                ok = false;
                break;
            }
            seen[b.lo] = seen[b.hi] = 1;
        }
        CHECK(ok, "log_n=%u stage %u: a pair is out of range, has the wrong twiddle or is taken twice", log_n, s);
    }
    {   // the plain load is a permutation of the n points
        const G1NttLoadMap m = g1_ntt_load_plain(log_n);
        std::fill(seen.begin(), seen.end(), 0);
        bool ok = m.count == n;
        for (uint64_t i = 0; ok && i < n; i++) {
            const uint32_t d = g1_ntt_bitrev((uint32_t)i, m.rev_log);
            ok = g1_ntt_load_source(m, i) == (int64_t)i && d < n && !seen[d] && g1_ntt_bitrev(d, m.rev_log) == i;
            if (ok) seen[d] = 1;
        }
        CHECK(ok, "log_n=%u: the plain load is no permutation", log_n);
    }
    {   // launches cover the lanes once, none is longer than the table
        for (uint64_t lanes : {(uint64_t)0, n / 2, n, 2 * n}) {
            uint64_t sum = 0;
            const G1NttSizes sz = g1_ntt_sizes(log_n, lanes);
            for (uint64_t k = 0; k < g1_ntt_launches(lanes); k++) {
                const uint64_t c = g1_ntt_launch_lanes(lanes, k);
                CHECK(c > 0 && c <= G1_NTT_LAUNCH && c * G1_NTT_POINT_BYTES <= sz.table, "log_n=%u lanes=%llu launch %llu", log_n,
                      (unsigned long long)lanes, (unsigned long long)k);
                sum += c;
            }
            CHECK(sum == lanes && g1_ntt_launch_lanes(lanes, g1_ntt_launches(lanes)) == 0, "log_n=%u: launches do not add up", log_n);
            CHECK(sz.points == G1_NTT_POINT_BYTES * n && sz.table >= G1_NTT_POINT_BYTES && sz.total == sz.points + sz.table &&
                      sz.points % 256 == 0, "log_n=%u: sizes", log_n);
        }
    }
    if (log_n >= 1 && log_n + 1 <= G1_NTT_MAX_LOG) {  // an opener of all n points: the coset construction with log_l = 0
        const uint64_t d = n - 1;
        const G1NttLoadMap sm = g1_coset_srs_map(log_n, 0, 0), hm = g1_coset_slice_map(log_n, 0);
        bool ok = g1_coset_shape_ok(log_n, 0) && sm.count == 2 * n && sm.rev_log == log_n + 1 && hm.count == n && hm.rev_log == log_n;
        for (uint64_t j = 0; ok && j < 2 * n; j++) ok = g1_ntt_load_source(sm, j) == (j < d ? (int64_t)(d - 1 - j) : -1);
        for (uint64_t i = 0; ok && i < n; i++) ok = g1_ntt_load_source(hm, i) == (i < d ? (int64_t)(d - 1 + i) : -1);
        CHECK(ok && 2 * d - 2 < 2 * n, "log_n=%u: opener maps", log_n);  // (the largest index of u that is read)
        for (uint64_t len : {(uint64_t)1, (uint64_t)2, n / 2 + 1, n - 1, n}) {
            if (len < 1 || len > n) continue;
            bool cok = true;
            for (uint64_t t : {(uint64_t)0, (uint64_t)1, len - 2, len - 1, len, d - 1, d, 2 * n - 1}) {
                if (t >= 2 * n) continue;
                cok = cok && g1_coset_coeff_source(log_n, 0, len, 0, t) == (t + 1 < len ? (int64_t)(t + 1) : -1);
            }
            CHECK(cok, "log_n=%u len=%llu: coefficient slots", log_n, (unsigned long long)len);
        }
        for (unsigned group_log = 0; group_log <= G1_COSET_MAX_GROUP_LOG; group_log++) {  // (no group size changes anything at l = 1)
            const G1CosetSizes os = g1_coset_sizes(log_n, 0, group_log);
            CHECK(os.srs_hat == 512 * n && os.partial == 0 && os.work == 512 * n && os.slice == 256 * n && os.scalars == 64 * n &&
                      os.table == g1_ntt_sizes(log_n + 1, 2 * n).table &&
                      os.total == os.srs_hat + os.work + os.slice + os.scalars + os.table, "log_n=%u: opener sizes", log_n);
        }
    }
}

static void dump(unsigned log_n) {
    const uint64_t n = (uint64_t)1 << log_n;
    for (unsigned s = 0; s < log_n; s++)
        for (uint32_t i = 0; i < n / 2; i++) {
            const G1NttButterfly b = g1_ntt_butterfly(log_n, s, i);
            printf("b %u %u %u %u %u\n", s, i, b.lo, b.hi, b.exp);
        }
    for (uint64_t i = 0; i < n; i++) printf("r %llu %u\n", (unsigned long long)i, g1_ntt_bitrev((uint32_t)i, log_n));
    if (log_n < 1) return;
    const G1NttLoadMap sm = g1_coset_srs_map(log_n, 0, 0), hm = g1_coset_slice_map(log_n, 0);  // all openings: log_l = 0
    for (uint64_t j = 0; j < 2 * n; j++) printf("s %llu %lld\n", (unsigned long long)j, (long long)g1_ntt_load_source(sm, j));
    for (uint64_t i = 0; i < n; i++) printf("h %llu %lld\n", (unsigned long long)i, (long long)g1_ntt_load_source(hm, i));
    for (uint64_t len = 1; len <= n; len++)
        for (uint64_t t = 0; t < 2 * n; t++)
            printf("g %llu %llu %lld\n", (unsigned long long)len, (unsigned long long)t, (long long)g1_coset_coeff_source(log_n, 0, len, 0, t));
}

int main(int argc, char** argv) {
    if (argc == 3 && !strcmp(argv[1], "dump")) {
        dump((unsigned)atoi(argv[2]));
        return 0;
    }
    for (unsigned log_n = 0; log_n <= G1_NTT_MAX_LOG; log_n++) check_size(log_n);
    for (unsigned log_n = 0; log_n <= 8; log_n++) check_transform(log_n);
    printf("g1 ntt plan: sizes 0..%u, %d failures\n", G1_NTT_MAX_LOG, fails);
    return fails ? 1 : 0;
}
