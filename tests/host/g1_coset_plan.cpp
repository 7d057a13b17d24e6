// The coset-opening part of csrc/g1_ntt_plan.hpp on its own, g++ only (tests/test_g1_coset_plan_cpu.py builds it with
// -fsanitize=address,undefined):
//   g1_coset_plan                          every (log_n <= 10, log_l < log_n): the l slice maps load every SRS index 0 .. n-l-1 exactly
//                                          once and none beyond, the rows of g hold every coefficient l .. len-1 exactly once and none
//                                          below l, the groups partition the l terms for every group size (l below it included), the
//                                          launches cover every term once within G1_NTT_LAUNCH, the fold sums every partial once, the sizes
//                                          agree; and the whole pipeline over F_65537 (scalars standing in for points, S_k = s^k) with
//                                          exactly these maps equals the division recurrence q_t = f_{t+l} + x_k^l q_{t+l} for every coset.
//                                          Launch splits are also checked at the sizes where they happen (log_n up to 23).
//   g1_coset_plan dump LOG_N LOG_L GROUP   the tables of one shape as text, for the comparison with tests/model/g1_coset_model.py
#include <algorithm>
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

typedef unsigned long long ull;
static const uint64_t P = 65537;  // 3 generates F_65537^*, of order 2^16
static uint64_t powmod(uint64_t b, uint64_t e) {
    uint64_t r = 1;
    for (b %= P; e; e >>= 1, b = b * b % P)
        if (e & 1) r = r * b % P;
    return r;
}
static uint64_t root(unsigned log_n) { return powmod(3, 65536 >> log_n); }

// the stages as the kernels run them, over a vector that was loaded bit-reversed; no scaling (the driver folds it into the scalars)
static void stages(std::vector<uint64_t>& v, unsigned log_n, bool inverse) {
    const uint64_t n = (uint64_t)1 << log_n;
    uint64_t w = root(log_n);
    if (inverse) w = powmod(w, P - 2);
    std::vector<uint64_t> tw(n / 2 ? n / 2 : 1, 1);
    for (uint64_t i = 1; i < n / 2; i++) tw[i] = tw[i - 1] * w % P;
    for (unsigned s = 0; s < log_n; s++)
        for (uint32_t i = 0; i < n / 2; i++) {
            const G1NttButterfly b = g1_ntt_butterfly(log_n, s, i);
            const uint64_t t = v[b.hi] * tw[b.exp] % P, a = v[b.lo];
            v[b.lo] = (a + t) % P;
            v[b.hi] = (a + P - t) % P;
        }
}
static std::vector<uint64_t> load(const std::vector<uint64_t>& src, const G1NttLoadMap& m) {
    std::vector<uint64_t> v(m.count);
    for (uint64_t i = 0; i < m.count; i++) {
        const int64_t s = g1_ntt_load_source(m, i);
        v[m.rev_log ? g1_ntt_bitrev((uint32_t)i, m.rev_log) : i] = s >= 0 ? src[(size_t)s] : 0;
    }
    return v;
}

static const unsigned GROUPS[] = {0, 1, 2, 3};
static std::vector<uint64_t> lengths(uint64_t n, uint64_t l) {
    std::vector<uint64_t> out;
    for (uint64_t len : {(uint64_t)1, l, l + 1, n - 1, n})
        if (len >= 1 && len <= n && std::find(out.begin(), out.end(), len) == out.end()) out.push_back(len);
    return out;
}

static void check_maps(unsigned log_n, unsigned log_l) {
    const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l;
    CHECK(g1_coset_shape_ok(log_n, log_l), "(%u,%u): shape refused", log_n, log_l);
    {   // SRS indices over the l slices
        std::vector<uint32_t> seen(n, 0);
        bool ok = true;
        for (uint64_t b = 0; b < l; b++) {
            const G1NttLoadMap m = g1_coset_srs_map(log_n, log_l, b);
            ok = ok && m.count == 2 * r && m.finite == r - 1 && m.rev_log == log_n - log_l + 1 && m.step == -(int32_t)l &&
                 m.src0 == (int64_t)((r - 2) * l + b);
            for (uint64_t j = 0; j < m.count; j++) {
                const int64_t s = g1_ntt_load_source(m, j);
                if (s < 0) continue;
                if ((uint64_t)s >= n) ok = false;
                else seen[(size_t)s]++;
            }
        }
        for (uint64_t k = 0; k < n; k++) ok = ok && seen[k] == (k < n - l ? 1u : 0u);
        CHECK(ok, "(%u,%u): the slices do not load every SRS point 0 .. n-l-1 exactly once", log_n, log_l);
    }
    for (uint64_t len : lengths(n, l)) {  // coefficient indices over the l rows
        std::vector<uint32_t> seen(n, 0);
        bool ok = true;
        for (uint64_t b = 0; b < l; b++)
            for (uint64_t t = 0; t < 2 * r; t++) {
                const int64_t s = g1_coset_coeff_source(log_n, log_l, len, b, t);
                if (s < 0) continue;
                if ((uint64_t)s >= len || (uint64_t)s != (t + 1) * l + b) ok = false;
                else seen[(size_t)s]++;
            }
        for (uint64_t k = 0; k < n; k++) ok = ok && seen[k] == (k >= l && k < len ? 1u : 0u);
        CHECK(ok, "(%u,%u) len=%llu: the rows of g do not hold every coefficient l .. len-1 exactly once", log_n, log_l, (ull)len);
    }
    {   // the slice of u
        const G1NttLoadMap hm = g1_coset_slice_map(log_n, log_l);
        bool ok = hm.count == r && hm.rev_log == log_n - log_l;
        for (uint64_t i = 0; ok && i < r; i++) ok = g1_ntt_load_source(hm, i) == (i < r - 1 ? (int64_t)(r - 2 + i) : -1);
        CHECK(ok && 2 * (r - 2) < 2 * r, "(%u,%u): slice map", log_n, log_l);
    }
    if (log_l == 0) {  // all n openings, d = n - 1 SRS points: the closed forms of zkp_kzg_open_all (tests/host/g1_ntt_plan.cpp has them too)
        const uint64_t d = n - 1;
        const G1NttLoadMap sm = g1_coset_srs_map(log_n, 0, 0), hm = g1_coset_slice_map(log_n, 0);
        bool ok = sm.count == 2 * n && sm.rev_log == log_n + 1 && hm.count == n && hm.rev_log == log_n;
        for (uint64_t j = 0; ok && j < 2 * n; j++) ok = g1_ntt_load_source(sm, j) == (j < d ? (int64_t)(d - 1 - j) : -1);  // source d-1-j
        for (uint64_t i = 0; ok && i < n; i++) ok = g1_ntt_load_source(hm, i) == (i < d ? (int64_t)(d - 1 + i) : -1);      // slice d-1+i
        CHECK(ok && 2 * d - 2 < 2 * n, "(%u,0): the maps of all openings", log_n);
        for (uint64_t len = 1; len <= n; len++) {
            bool cok = true;
            for (uint64_t t = 0; t < 2 * n; t++) cok = cok && g1_coset_coeff_source(log_n, 0, len, 0, t) == (t + 1 < len ? (int64_t)(t + 1) : -1);
            CHECK(cok, "(%u,0) len=%llu: slot t of g is not coefficient t + 1", log_n, (ull)len);
        }
        for (unsigned group_log : GROUPS) {
            const G1CosetSizes sz = g1_coset_sizes(log_n, 0, group_log);
            const G1CosetMac m = g1_coset_mac(log_n, 0, group_log);
            CHECK(sz.srs_hat == 512 * n && sz.partial == 0 && sz.work == 512 * n && sz.slice == 256 * n && sz.scalars == 64 * n &&
                      sz.table == g1_ntt_sizes(log_n + 1, 2 * n).table && sz.total == sz.srs_hat + sz.work + sz.slice + sz.scalars + sz.table,
                  "(%u,0) B=2^%u: the sizes of all openings", log_n, group_log);
            CHECK(m.terms == 1 && m.groups == 1 && m.lanes == 2 * n && m.launch_lanes == G1_NTT_LAUNCH && g1_coset_fold_steps(m) == 0,
                  "(%u,0) B=2^%u: one term per lane, no fold", log_n, group_log);
        }
    }
}

// groups, launches, fold and sizes of one shape and group size; `elements`: also walk every term (small shapes)
static void check_mac(unsigned log_n, unsigned log_l, unsigned group_log, bool elements) {
    const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l;
    const unsigned log_m = log_n - log_l + 1;
    const G1CosetMac m = g1_coset_mac(log_n, log_l, group_log);
    CHECK(m.terms == (l < ((uint64_t)1 << group_log) ? l : (uint64_t)1 << group_log) && m.terms * m.groups == l && m.lanes == m.groups * 2 * r &&
              m.launch_lanes * m.terms == G1_NTT_LAUNCH, "(%u,%u) B=2^%u: groups", log_n, log_l, group_log);
    uint64_t sum = 0;
    const G1CosetSizes sz = g1_coset_sizes(log_n, log_l, group_log);
    for (uint64_t k = 0; k < g1_coset_mac_launches(m); k++) {
        const uint64_t c = g1_coset_mac_launch_lanes(m, k);
        CHECK(c > 0 && c * m.terms <= G1_NTT_LAUNCH && c * m.terms * G1_NTT_POINT_BYTES <= sz.table && c <= 0xffffffffu,
              "(%u,%u) B=2^%u: launch %llu holds more terms than the table", log_n, log_l, group_log, (ull)k);
        sum += c;
    }
    CHECK(sum == m.lanes && g1_coset_mac_launch_lanes(m, g1_coset_mac_launches(m)) == 0, "(%u,%u) B=2^%u: launches do not add up", log_n, log_l,
          group_log);
    if (elements) {  // every element (b, k) of the 2n is the term of exactly one (lane, j), within its lane's output and group
        std::vector<uint8_t> seen(2 * n, 0);
        bool ok = true;
        for (uint64_t k = 0, first = 0; k < g1_coset_mac_launches(m); first += g1_coset_mac_launch_lanes(m, k), k++)
            for (uint64_t lane = first; lane < first + g1_coset_mac_launch_lanes(m, k); lane++)
                for (uint32_t j = 0; j < m.terms; j++) {
                    const uint64_t e = g1_coset_mac_element(log_m, m.terms, lane, j);
                    const uint64_t b = e >> log_m, out = e & (2 * r - 1);
                    if (e >= 2 * n || seen[e] || out != (lane & (2 * r - 1)) || b / m.terms != lane >> log_m || b % m.terms != j) ok = false;
                    else seen[e] = 1;
                }
        for (uint64_t e = 0; e < 2 * n; e++) ok = ok && seen[e];
        CHECK(ok, "(%u,%u) B=2^%u: the lanes' terms do not partition the 2n products", log_n, log_l, group_log);
    }
    {   // fold: the partials left halve down to one, every step stays inside what the step before left
        uint64_t left = m.groups;
        const unsigned steps = g1_coset_fold_steps(m);
        for (unsigned i = 0; i < steps; i++) {
            const G1CosetFoldStep f = g1_coset_fold_step(log_n, log_l, m, i);
            CHECK(f.half * 2 == left && f.lanes == f.half * 2 * r && f.last == (i + 1 == steps), "(%u,%u) B=2^%u: fold step %u", log_n, log_l,
                  group_log, i);
            left = f.half;
        }
        CHECK(left == 1 && (steps == 0) == (m.groups == 1), "(%u,%u) B=2^%u: the fold does not end at one sum", log_n, log_l, group_log);
    }
    CHECK(sz.srs_hat == 512 * n && sz.partial == (m.groups > 1 ? 256 * m.lanes : 0) && sz.work == 512 * r && sz.slice == 256 * r &&
              sz.scalars == 64 * n && sz.table == 256 * (2 * n < G1_NTT_LAUNCH ? 2 * n : G1_NTT_LAUNCH) && sz.table <= ((size_t)64 << 20) &&
              sz.table >= g1_ntt_sizes(log_m, r).table &&  // (the stages of u and of a slice multiply r lanes at most)
              sz.total == sz.srs_hat + sz.partial + sz.work + sz.slice + sz.scalars + sz.table,
          "(%u,%u) B=2^%u: sizes", log_n, log_l, group_log);
}

// the whole pipeline over F_65537 with these maps against the division recurrence, for every coset
static void check_pipeline(unsigned log_n, unsigned log_l) {
    const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l;
    const unsigned log_r = log_n - log_l, log_m = log_r + 1;
    const uint64_t s = 4242 + 17 * log_n + log_l, w = root(log_n), ninv = powmod(2 * r, P - 2);
    std::vector<uint64_t> srs(n);
    srs[0] = 1;
    for (uint64_t k = 1; k < n; k++) srs[k] = srs[k - 1] * s % P;
    std::vector<uint64_t> s_hat(2 * n);  // slice b at [b 2r, (b + 1) 2r), as the opener keeps it
    for (uint64_t b = 0; b < l; b++) {
        std::vector<uint64_t> v = load(srs, g1_coset_srs_map(log_n, log_l, b));
        stages(v, log_m, false);
        std::copy(v.begin(), v.end(), s_hat.begin() + b * 2 * r);
    }
    uint64_t x = 99 + log_n * 31 + log_l;
    for (uint64_t len : lengths(n, l)) {
        std::vector<uint64_t> f(len);
        for (uint64_t& e : f) e = (x = (x * 1103515245u + 12345u) & 0x7fffffffu) % P;
        std::vector<uint64_t> g_hat(2 * n);
        for (uint64_t b = 0; b < l; b++) {
            std::vector<uint64_t> v(2 * r);
            for (uint64_t t = 0; t < 2 * r; t++) {
                const int64_t src = g1_coset_coeff_source(log_n, log_l, len, b, t);
                v[g1_ntt_bitrev((uint32_t)t, log_m)] = src >= 0 ? f[(size_t)src] : 0;
            }
            stages(v, log_m, false);
            for (uint64_t k = 0; k < 2 * r; k++) g_hat[b * 2 * r + k] = v[k] * ninv % P;
        }
        std::vector<uint64_t> want(r);  // q_k(s) by the recurrence
        for (uint64_t k = 0; k < r; k++) {
            const uint64_t c = powmod(w, k * l % n);  // x_k^l
            std::vector<uint64_t> q(n, 0);
            uint64_t acc = 0;
            for (int64_t t = (int64_t)n - (int64_t)l - 1; t >= 0; t--) {
                const uint64_t hi = (uint64_t)t + l;
                q[(size_t)t] = ((hi < len ? f[hi] : 0) + c * (hi < n ? q[hi] : 0)) % P;
                acc = (acc + q[(size_t)t] * srs[(size_t)t]) % P;
            }
            want[k] = acc;
        }
        for (unsigned group_log : GROUPS) {
            const G1CosetMac m = g1_coset_mac(log_n, log_l, group_log);
            std::vector<uint64_t> partial(m.lanes), u(2 * r, 0);
            for (uint64_t k = 0, first = 0; k < g1_coset_mac_launches(m); first += g1_coset_mac_launch_lanes(m, k), k++)
                for (uint64_t lane = first; lane < first + g1_coset_mac_launch_lanes(m, k); lane++) {
                    uint64_t acc = 0;
                    for (uint32_t j = 0; j < m.terms; j++) {
                        const uint64_t e = g1_coset_mac_element(log_m, m.terms, lane, j);
                        acc = (acc + g_hat[e] * s_hat[e]) % P;
                    }
                    partial[lane] = acc;
                }
            if (m.groups == 1)
                for (uint64_t k = 0; k < 2 * r; k++) u[g1_ntt_bitrev((uint32_t)k, log_m)] = partial[k];
            for (unsigned i = 0; i < g1_coset_fold_steps(m); i++) {
                const G1CosetFoldStep fs = g1_coset_fold_step(log_n, log_l, m, i);
                for (uint64_t q = 0; q < fs.lanes; q++) {
                    const uint64_t sum = (partial[q] + partial[q + fs.lanes]) % P;
                    if (fs.last) u[g1_ntt_bitrev((uint32_t)q, log_m)] = sum;
                    else partial[q] = sum;
                }
            }
            stages(u, log_m, true);
            std::vector<uint64_t> h = load(u, g1_coset_slice_map(log_n, log_l));
            stages(h, log_r, false);
            bool ok = true;
            for (uint64_t k = 0; k < r; k++) ok = ok && h[k] == want[k];
            CHECK(ok, "(%u,%u) len=%llu B=2^%u: the pipeline is not the division recurrence", log_n, log_l, (ull)len, group_log);
            if (len <= l)
                for (uint64_t k = 0; k < r; k++) CHECK(h[k] == 0, "(%u,%u) len=%llu: a proof of len <= l is not the identity", log_n, log_l, (ull)len);
        }
    }
}

static void dump(unsigned log_n, unsigned log_l, unsigned group_log) {
    const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l;
    const unsigned log_m = log_n - log_l + 1;
    for (uint64_t b = 0; b < l; b++) {
        const G1NttLoadMap m = g1_coset_srs_map(log_n, log_l, b);
        for (uint64_t j = 0; j < m.count; j++) printf("s %llu %llu %lld\n", (ull)b, (ull)j, (long long)g1_ntt_load_source(m, j));
    }
    for (uint64_t len : lengths(n, l))
        for (uint64_t b = 0; b < l; b++)
            for (uint64_t t = 0; t < 2 * r; t++)
                printf("g %llu %llu %llu %lld\n", (ull)len, (ull)b, (ull)t, (long long)g1_coset_coeff_source(log_n, log_l, len, b, t));
    const G1NttLoadMap hm = g1_coset_slice_map(log_n, log_l);
    for (uint64_t i = 0; i < r; i++) printf("h %llu %lld\n", (ull)i, (long long)g1_ntt_load_source(hm, i));
    const G1CosetMac m = g1_coset_mac(log_n, log_l, group_log);
    printf("m %u %llu %llu %llu\n", m.terms, (ull)m.groups, (ull)m.lanes, (ull)m.launch_lanes);
    for (uint64_t lane = 0; lane < m.lanes; lane++)
        for (uint32_t j = 0; j < m.terms; j++) printf("e %llu %u %llu\n", (ull)lane, j, (ull)g1_coset_mac_element(log_m, m.terms, lane, j));
    for (unsigned i = 0; i < g1_coset_fold_steps(m); i++) {
        const G1CosetFoldStep f = g1_coset_fold_step(log_n, log_l, m, i);
        printf("f %u %llu %llu %d\n", i, (ull)f.half, (ull)f.lanes, f.last ? 1 : 0);
    }
    const G1CosetSizes sz = g1_coset_sizes(log_n, log_l, group_log);
    printf("z %zu %zu %zu %zu %zu %zu %zu\n", sz.srs_hat, sz.partial, sz.work, sz.slice, sz.scalars, sz.table, sz.total);
}

int main(int argc, char** argv) {
    if (argc == 5 && !strcmp(argv[1], "dump")) {
        dump((unsigned)atoi(argv[2]), (unsigned)atoi(argv[3]), (unsigned)atoi(argv[4]));
        return 0;
    }
    unsigned shapes = 0;
    for (unsigned log_n = 1; log_n <= 10; log_n++)
        for (unsigned log_l = 0; log_l < log_n; log_l++, shapes++) {
            check_maps(log_n, log_l);
            for (unsigned group_log : GROUPS) check_mac(log_n, log_l, group_log, true);
            check_pipeline(log_n, log_l);
        }
    for (unsigned log_n : {17u, 18u, 20u, 23u})  // where a pass takes more than one launch
        for (unsigned log_l : {0u, 1u, 6u, 10u, log_n - 1})
            for (unsigned group_log : GROUPS) check_mac(log_n, log_l, group_log, log_n <= 18);
    // all openings: n = 2^18 is the smallest whose 2n products take two launches (the suite's test_open_all_two_launches)
    CHECK(g1_coset_mac_launches(g1_coset_mac(17, 0, 0)) == 1 && g1_coset_mac_launches(g1_coset_mac(18, 0, 0)) == 2, "(18,0): two launches");
    {   // (18, 10), the suite's launch-splitting case: 2^19 terms in two launches, and with groups of 8 lane 2^15 -- the first of the
        // second launch -- begins a group
        const G1CosetMac m = g1_coset_mac(18, 10, 3);
        CHECK(g1_coset_mac_launches(m) == 2 && m.launch_lanes == (1u << 15) && (m.launch_lanes & 511) == 0, "(18,10): two launches");
        CHECK(g1_coset_mac_launches(g1_coset_mac(18, 10, 0)) == 2, "(18,10) B=1: two launches");
    }
    CHECK(!g1_coset_shape_ok(5, 5) && !g1_coset_shape_ok(5, 6) && !g1_coset_shape_ok(24, 6) && g1_coset_shape_ok(23, 6) && g1_coset_shape_ok(1, 0),
          "shape limits");
    printf("g1 coset plan: %u shapes, %d failures\n", shapes, fails);
    return fails ? 1 : 0;
}
