// The batch part of csrc/g1_ntt_plan.hpp on its own, g++ only (tests/test_g1_coset_batch_plan_cpu.py builds it with
// -fsanitize=address,undefined).  Every shape of log_n <= 7, every group size 0 .. 3 and n_polys in {1, 2, 3, 5}, on openers made for
// max_polys = n_polys, 5, 64 and 4096 and -- for the launch cutting -- on the table a max_polys = 1 opener has:
//   - every (polynomial, group, output) is taken by exactly one lane of exactly one launch of the multiply-accumulate pass;
//   - every table index of a launch is below the table's capacity (the place where G1_NTT_LAUNCH alone would overrun it: checked too);
//   - every partial, u and h index is below its capacity and inside its polynomial's range;
//   - the fold steps consume each partial once;
//   - g1_coset_sizes(.., 1) is what the sizes were before there was a batch, and max_polys scales the per-call vectors only;
//   - the whole pipeline over F_65537 (scalars standing in for points, S_k = s^k): row p of the batch, whose coefficient rows lie
//     `stride` apart with poison between them, equals the single-polynomial pipeline of polynomial p, which tests/host/g1_coset_plan.cpp
//     pins against the division recurrence.
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

// the stages as the kernels run them over the 2^log_n slots at v[off ..], loaded bit-reversed; no scaling
static void stages(std::vector<uint64_t>& v, size_t off, unsigned log_n, bool inverse) {
    const uint64_t n = (uint64_t)1 << log_n;
    uint64_t w = root(log_n);
    if (inverse) w = powmod(w, P - 2);
    std::vector<uint64_t> tw(n / 2 ? n / 2 : 1, 1);
    for (uint64_t i = 1; i < n / 2; i++) tw[i] = tw[i - 1] * w % P;
    for (unsigned s = 0; s < log_n; s++)
        for (uint32_t i = 0; i < n / 2; i++) {
            const G1NttButterfly b = g1_ntt_butterfly(log_n, s, i);
            const uint64_t t = v[off + b.hi] * tw[b.exp] % P, a = v[off + b.lo];
            v[off + b.lo] = (a + t) % P;
            v[off + b.hi] = (a + P - t) % P;
        }
}
// a natural-order transform of the 2^log_n slots at v[off ..], as run_ntt<Fr> gives it
static void transform(std::vector<uint64_t>& v, size_t off, unsigned log_n) {
    const uint64_t n = (uint64_t)1 << log_n;
    std::vector<uint64_t> t(n);
    for (uint64_t i = 0; i < n; i++) t[g1_ntt_bitrev((uint32_t)i, log_n)] = v[off + i];
    stages(t, 0, log_n, false);
    std::copy(t.begin(), t.end(), v.begin() + off);
}

static const unsigned GROUPS[] = {0, 1, 2, 3};
static const uint64_t POLYS[] = {1, 2, 3, 5};

// the sizes as they were before the batch: one polynomial, a table of min(2n, G1_NTT_LAUNCH) entries
static void check_sizes(unsigned log_n, unsigned log_l, unsigned group_log) {
    const uint64_t n = (uint64_t)1 << log_n, r = n >> log_l;
    const G1CosetMac m = g1_coset_mac(log_n, log_l, group_log);
    const size_t partial = m.groups > 1 ? 256 * m.lanes : 0, table = 256 * (2 * n < G1_NTT_LAUNCH ? 2 * n : G1_NTT_LAUNCH);
    for (int dflt = 0; dflt < 2; dflt++) {
        const G1CosetSizes s = dflt ? g1_coset_sizes(log_n, log_l, group_log) : g1_coset_sizes(log_n, log_l, group_log, 1);
        CHECK(s.srs_hat == 512 * n && s.partial == partial && s.work == 512 * r && s.slice == 256 * r && s.scalars == 64 * n && s.table == table &&
                  s.table == g1_ntt_sizes(log_n + 1, 2 * n).table && s.total == 512 * n + partial + 768 * r + 64 * n + table,
              "(%u,%u) B=2^%u: the sizes of one polynomial changed", log_n, log_l, group_log);
    }
    for (uint64_t mp : {(uint64_t)2, (uint64_t)3, (uint64_t)5, (uint64_t)4096}) {
        const G1CosetSizes s = g1_coset_sizes(log_n, log_l, group_log, mp);
        const uint64_t entries = g1_coset_table_entries(log_n, mp);
        CHECK(s.srs_hat == 512 * n && s.partial == mp * partial && s.work == mp * 512 * r && s.slice == mp * 256 * r && s.scalars == mp * 64 * n &&
                  entries == (mp * 2 * n < G1_NTT_LAUNCH ? mp * 2 * n : G1_NTT_LAUNCH) && s.table == 256 * entries &&
                  s.table <= ((size_t)64 << 20) && s.total == s.srs_hat + s.partial + s.work + s.slice + s.scalars + s.table,
              "(%u,%u) B=2^%u max_polys=%llu: sizes", log_n, log_l, group_log, (ull)mp);
        // a grid row of the stages of u parks r entries, of h r / 2: at least one row fits, or the launches of a row are cut at G1_NTT_LAUNCH
        CHECK(std::min<uint64_t>(entries, G1_NTT_LAUNCH) >= std::min<uint64_t>(r, G1_NTT_LAUNCH), "(%u,%u): the table is shorter than a row of stages", log_n,
              log_l);
    }
}

// lanes, launches, table, partial and u indices of a batch of n_polys on an opener of max_polys whose table has tcap entries
static void check_batch(unsigned log_n, unsigned log_l, unsigned group_log, uint64_t n_polys, uint64_t max_polys, uint64_t tcap) {
    const uint64_t n = (uint64_t)1 << log_n, r = n >> log_l;
    const unsigned log_m = log_n - log_l + 1;
    const G1CosetBatch b = g1_coset_batch(log_n, log_l, group_log, n_polys, tcap);
    const G1CosetMac& m = b.one;
    const uint64_t lanes1 = m.lanes;
#define WHERE "(%u,%u) B=2^%u polys=%llu/%llu tcap=%llu: "
#define ARGS log_n, log_l, group_log, (ull)n_polys, (ull)max_polys, (ull)tcap
    CHECK(((uint64_t)1 << b.lanes_log) == lanes1 && b.lanes == n_polys * lanes1 && b.launch_lanes >= 1 && b.launch_lanes * m.terms <= tcap &&
              b.launch_lanes * m.terms <= G1_NTT_LAUNCH && lanes1 * m.terms == 2 * n,
          WHERE "lanes", ARGS);
    // (polynomial, group, output) -> how many lanes took it; per launch the table entries its lanes park
    std::vector<uint32_t> seen(n_polys * lanes1, 0);
    std::vector<uint8_t> scalar_seen(n_polys * 2 * n, 0);
    uint64_t sum = 0, first = 0;
    bool ok = true, table_ok = true, dst_ok = true;
    for (uint64_t k = 0; k < g1_coset_batch_launches(b); k++) {
        const uint64_t cnt = g1_coset_batch_launch_lanes(b, k);
        CHECK(cnt > 0 && cnt <= 0xffffffffu && first == k * b.launch_lanes, WHERE "launch %llu", ARGS, (ull)k);
        std::vector<uint8_t> entry(tcap, 0);
        for (uint64_t lane = 0; lane < cnt; lane++) {
            const uint64_t L = first + lane;
            const G1CosetOf of = g1_coset_of(b.lanes_log, L);
            if (of.p >= n_polys || of.in >= lanes1 || of.p * lanes1 + of.in != L) { ok = false; continue; }
            seen[of.p * lanes1 + of.in]++;  // of.in = group * 2r + output
            for (uint32_t j = 0; j < m.terms; j++) {
                const uint64_t t = (uint64_t)j * cnt + lane;  // the kernel's table entry
                if (t >= tcap || entry[t]) table_ok = false;
                else entry[t] = 1;
                // the term's scalar, by the batch lane as the kernel takes it, and its point: those of lane of.in of one polynomial
                const uint64_t se = g1_coset_mac_element(log_m, m.terms, L, j), e = g1_coset_batch_srs(log_n, se);
                if (e != g1_coset_mac_element(log_m, m.terms, of.in, j) || se != of.p * 2 * n + e || scalar_seen[se]) ok = false;
                else scalar_seen[se] = 1;
            }
            if (m.groups == 1) {  // the lane writes its polynomial's u
                const G1CosetOf out = g1_coset_of(log_m, L);  // 2r lanes per polynomial: as the kernel finds its slot
                const uint64_t d = g1_coset_batch_u(log_m, out.p, out.in);
                if (out.p != of.p || out.in != of.in || d >= max_polys * 2 * r || d < of.p * 2 * r || d >= (of.p + 1) * 2 * r) dst_ok = false;
            } else if (L >= max_polys * lanes1) dst_ok = false;  // its partial sum, slot L
        }
        sum += cnt;
        first += cnt;
    }
    for (uint32_t c : seen) ok = ok && c == 1;
    for (uint8_t c : scalar_seen) ok = ok && c == 1;
    CHECK(ok && sum == b.lanes && g1_coset_batch_launch_lanes(b, g1_coset_batch_launches(b)) == 0,
          WHERE "the launches do not take every (polynomial, group, output) and every scalar once", ARGS);
    CHECK(table_ok, WHERE "a table entry beyond the capacity, or shared by two lanes of a launch", ARGS);
    CHECK(dst_ok, WHERE "a lane writes outside its polynomial", ARGS);
    {   // the fold: every partial of every polynomial is added in exactly once, every step stays inside its polynomial
        std::vector<uint32_t> weight(max_polys * lanes1, 0), u(max_polys * 2 * r, 0);
        for (uint64_t L = 0; L < n_polys * lanes1; L++) weight[L] = 1;
        bool fok = true;
        for (unsigned i = 0; i < g1_coset_fold_steps(m); i++) {
            const G1CosetFoldStep f = g1_coset_fold_step(log_n, log_l, m, i);
            const unsigned step_log = g1_coset_fold_step_log(log_n, log_l, m, i);
            fok = fok && ((uint64_t)1 << step_log) == f.lanes;
            for (uint64_t j = 0; j < n_polys * f.lanes; j++) {
                const G1CosetFoldLane fl = g1_coset_fold_lane(b.lanes_log, step_log, j);
                if (fl.p >= n_polys || fl.lo < fl.p * lanes1 || fl.hi >= (fl.p + 1) * lanes1 || fl.hi != fl.lo + f.lanes || fl.in >= f.lanes) { fok = false; continue; }
                const uint32_t s = weight[fl.lo] + weight[fl.hi];
                weight[fl.hi] = 0;
                if (f.last) {
                    const uint64_t d = g1_coset_batch_u(log_m, fl.p, fl.in);
                    if (d < fl.p * 2 * r || d >= (fl.p + 1) * 2 * r || u[d]) fok = false;
                    else u[d] = s;
                    weight[fl.lo] = 0;
                } else weight[fl.lo] = s;
            }
        }
        if (m.groups > 1) {
            for (uint64_t d = 0; d < max_polys * 2 * r; d++) fok = fok && u[d] == (d < n_polys * 2 * r ? m.groups : 0);
            for (uint32_t x : weight) fok = fok && x == 0;
        }
        CHECK(fok, WHERE "the fold does not add every partial of a polynomial into its output once", ARGS);
    }
    {   // the slices h out of u
        const G1NttLoadMap map = g1_coset_slice_map(log_n, log_l);
        std::vector<uint8_t> hs(max_polys * r, 0);
        bool sok = map.count == r && ((uint64_t)1 << map.rev_log) == r;
        for (uint64_t i = 0; i < n_polys * r; i++) {
            const G1CosetSlice c = g1_coset_batch_slice(map, log_m, i);
            const uint64_t p = i >> map.rev_log;
            if (c.dst < p * r || c.dst >= (p + 1) * r || hs[c.dst]) sok = false;
            else hs[c.dst] = 1;
            if (c.src >= 0 && ((uint64_t)c.src < p * 2 * r || (uint64_t)c.src >= (p + 1) * 2 * r)) sok = false;
            if ((c.src < 0) != (g1_ntt_load_source(map, i & (r - 1)) < 0)) sok = false;
        }
        CHECK(sok, WHERE "the slices of h", ARGS);
    }
#undef WHERE
#undef ARGS
}

// one polynomial by the functions of the single path, as tests/host/g1_coset_plan.cpp walks them: the r proofs
static std::vector<uint64_t> single(const std::vector<uint64_t>& f, const std::vector<uint64_t>& s_hat, unsigned log_n, unsigned log_l,
                                    unsigned group_log) {
    const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l, len = f.size();
    const unsigned log_r = log_n - log_l, log_m = log_r + 1;
    const uint64_t ninv = powmod(2 * r, P - 2);
    std::vector<uint64_t> g_hat(2 * n);
    for (uint64_t b = 0; b < l; b++) {
        for (uint64_t t = 0; t < 2 * r; t++) {
            const int64_t src = g1_coset_coeff_source(log_n, log_l, len, b, t);
            g_hat[b * 2 * r + t] = src >= 0 ? f[(size_t)src] : 0;
        }
        transform(g_hat, b * 2 * r, log_m);
    }
    for (uint64_t& x : g_hat) x = x * ninv % P;
    const G1CosetMac m = g1_coset_mac(log_n, log_l, group_log);
    std::vector<uint64_t> partial(m.lanes), u(2 * r, 0);
    for (uint64_t lane = 0; lane < m.lanes; lane++) {
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
    stages(u, 0, log_m, true);
    const G1NttLoadMap hm = g1_coset_slice_map(log_n, log_l);
    std::vector<uint64_t> h(r);
    for (uint64_t i = 0; i < r; i++) {
        const int64_t s = g1_ntt_load_source(hm, i);
        h[g1_ntt_bitrev((uint32_t)i, hm.rev_log)] = s >= 0 ? u[(size_t)s] : 0;
    }
    stages(h, 0, log_r, false);
    return h;
}

// the batch driver's walk over F_65537 against `single` of every row
static void check_pipeline(unsigned log_n, unsigned log_l, unsigned group_log, uint64_t n_polys, uint64_t max_polys) {
    const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l;
    const unsigned log_r = log_n - log_l, log_m = log_r + 1;
    const uint64_t s = 4242 + 17 * log_n + log_l, ninv = powmod(2 * r, P - 2);
    std::vector<uint64_t> srs(n, 1);
    for (uint64_t k = 1; k < n; k++) srs[k] = srs[k - 1] * s % P;
    std::vector<uint64_t> s_hat(2 * n);
    for (uint64_t b = 0; b < l; b++) {
        const G1NttLoadMap sm = g1_coset_srs_map(log_n, log_l, b);
        for (uint64_t j = 0; j < sm.count; j++) {
            const int64_t src = g1_ntt_load_source(sm, j);
            s_hat[b * 2 * r + g1_ntt_bitrev((uint32_t)j, sm.rev_log)] = src >= 0 ? srs[(size_t)src] : 0;
        }
        stages(s_hat, b * 2 * r, log_m, false);
    }
    uint64_t x = 99 + log_n * 31 + log_l + 7 * n_polys;
    for (uint64_t len : {l, l + 1 < n ? l + 1 : n, n}) {
        // rows `stride` apart with poison between them; row p keeps len - p (n / 4 + 1) coefficients, zeros behind (the last row is all zero)
        const uint64_t stride = len + 3;
        std::vector<uint64_t> coeffs(n_polys * stride, 54321);
        std::vector<std::vector<uint64_t>> rows(n_polys, std::vector<uint64_t>(len, 0));
        for (uint64_t p = 0; p < n_polys; p++) {
            const uint64_t cut = p * (n / 4 + 1), keep = n_polys > 1 && p + 1 == n_polys ? 0 : len > cut ? len - cut : 1;
            for (uint64_t i = 0; i < len; i++) coeffs[p * stride + i] = rows[p][i] = i < keep ? (x = (x * 1103515245u + 12345u) & 0x7fffffffu) % P : 0;
        }
        const G1CosetBatch b = g1_coset_batch(log_n, log_l, group_log, n_polys, g1_coset_table_entries(log_n, max_polys));
        const G1CosetMac& m = b.one;
        std::vector<uint64_t> g(max_polys * 2 * n, 11111), partial(max_polys * m.lanes, 22222), u(max_polys * 2 * r, 33333), h(max_polys * r, 44444);
        for (uint64_t i = 0; i < n_polys * 2 * n; i++) {  // gather
            const G1CosetOf of = g1_coset_of(log_n + 1, i);
            const int64_t src = g1_coset_batch_coeff_source(log_n, log_l, len, stride, of.p, of.in);
            CHECK(src < 0 || ((uint64_t)src >= of.p * stride && (uint64_t)src < of.p * stride + len), "(%u,%u): a coefficient outside its row", log_n, log_l);
            g[i] = src >= 0 ? coeffs[(size_t)src] : 0;
        }
        for (uint64_t row = 0; row < n_polys * l; row++) transform(g, row * 2 * r, log_m);  // one batch of n_polys l rows
        for (uint64_t i = 0; i < n_polys * 2 * n; i++) g[i] = g[i] * ninv % P;              // split
        for (uint64_t k = 0, first = 0; k < g1_coset_batch_launches(b); first += g1_coset_batch_launch_lanes(b, k), k++)
            for (uint64_t L = first; L < first + g1_coset_batch_launch_lanes(b, k); L++) {
                const G1CosetOf of = g1_coset_of(b.lanes_log, L);
                uint64_t acc = 0;
                for (uint32_t j = 0; j < m.terms; j++) {
                    // as the kernel: the scalar by the batch lane, the point by the lane within its polynomial
                    acc = (acc + g[g1_coset_mac_element(log_m, m.terms, L, j)] * s_hat[g1_coset_mac_element(log_m, m.terms, of.in, j)]) % P;
                }
                if (m.groups == 1) u[g1_coset_batch_u(log_m, of.p, of.in & (2 * r - 1))] = acc;
                else partial[L] = acc;
            }
        for (unsigned i = 0; i < g1_coset_fold_steps(m); i++) {
            const G1CosetFoldStep fs = g1_coset_fold_step(log_n, log_l, m, i);
            const unsigned step_log = g1_coset_fold_step_log(log_n, log_l, m, i);
            for (uint64_t j = 0; j < n_polys * fs.lanes; j++) {
                const G1CosetFoldLane fl = g1_coset_fold_lane(b.lanes_log, step_log, j);
                const uint64_t sum = (partial[fl.lo] + partial[fl.hi]) % P;
                if (fs.last) u[g1_coset_batch_u(log_m, fl.p, fl.in)] = sum;
                else partial[fl.lo] = sum;
            }
        }
        for (uint64_t p = 0; p < n_polys; p++) stages(u, p * 2 * r, log_m, true);  // grid row p of the stages
        const G1NttLoadMap hm = g1_coset_slice_map(log_n, log_l);
        for (uint64_t i = 0; i < n_polys * r; i++) {
            const G1CosetSlice c = g1_coset_batch_slice(hm, log_m, i);
            h[c.dst] = c.src >= 0 ? u[(size_t)c.src] : 0;
        }
        for (uint64_t p = 0; p < n_polys; p++) stages(h, p * r, log_r, false);
        for (uint64_t p = 0; p < n_polys; p++) {
            const std::vector<uint64_t> want = single(rows[p], s_hat, log_n, log_l, group_log);
            bool ok = true, zero = true;
            for (uint64_t k = 0; k < r; k++) {
                ok = ok && h[p * r + k] == want[k];
                zero = zero && h[p * r + k] == 0;
            }
            CHECK(ok, "(%u,%u) len=%llu B=2^%u polys=%llu/%llu: row %llu of the batch is not the single pipeline", log_n, log_l, (ull)len, group_log,
                  (ull)n_polys, (ull)max_polys, (ull)p);
            if (len <= l || (n_polys > 1 && p + 1 == n_polys)) CHECK(zero, "(%u,%u) row %llu: not r identities", log_n, log_l, (ull)p);
        }
        for (uint64_t i = n_polys * r; i < max_polys * r; i++) CHECK(h[i] == 44444, "(%u,%u): h beyond the batch was written", log_n, log_l);
        for (uint64_t i = n_polys * 2 * r; i < max_polys * 2 * r; i++) CHECK(u[i] == 33333, "(%u,%u): u beyond the batch was written", log_n, log_l);
    }
}

int main() {
    unsigned shapes = 0, cases = 0;
    for (unsigned log_n = 1; log_n <= 7; log_n++)
        for (unsigned log_l = 0; log_l < log_n; log_l++, shapes++)
            for (unsigned group_log : GROUPS) {
                check_sizes(log_n, log_l, group_log);
                for (uint64_t n_polys : POLYS) {
                    for (uint64_t max_polys : {n_polys, (uint64_t)5, n_polys == 5 ? G1_COSET_MAX_POLYS : (uint64_t)64})
                        check_batch(log_n, log_l, group_log, n_polys, max_polys, g1_coset_table_entries(log_n, max_polys));
                    // the table of a max_polys = 1 opener: a batch cut for it stays inside it ...
                    const uint64_t small = g1_coset_table_entries(log_n, 1);
                    check_batch(log_n, log_l, group_log, n_polys, n_polys, small);
                    // ... which the single path's cut, G1_NTT_LAUNCH terms whatever the table holds, would not
                    const G1CosetMac m = g1_coset_mac(log_n, log_l, group_log);
                    const uint64_t lanes = n_polys * m.lanes, naive = lanes < m.launch_lanes ? lanes : m.launch_lanes;
                    CHECK(n_polys == 1 ? naive * m.terms <= small : naive * m.terms > small, "(%u,%u) B=2^%u polys=%llu: the naive cut", log_n, log_l,
                          group_log, (ull)n_polys);
                    check_pipeline(log_n, log_l, group_log, n_polys, n_polys);
                    if (n_polys == 3) check_pipeline(log_n, log_l, group_log, n_polys, 5);
                    cases++;
                }
            }
    // where the table is full: (10, 6) with 129 polynomials is two launches, the second of one polynomial (the suite's GPU case), and
    // with one polynomial the launches of the single path
    for (unsigned group_log : GROUPS) {
        const G1CosetBatch b = g1_coset_batch(10, 6, group_log, 129, g1_coset_table_entries(10, 129));
        CHECK(g1_coset_batch_launches(b) == 2 && g1_coset_batch_launch_lanes(b, 1) == b.one.lanes && b.launch_lanes * b.one.terms == G1_NTT_LAUNCH,
              "(10,6) x 129 B=2^%u: two launches, one polynomial in the second", group_log);
        check_batch(10, 6, group_log, 129, 129, g1_coset_table_entries(10, 129));
        for (unsigned log_n : {17u, 18u, 20u}) {
            const G1CosetMac m = g1_coset_mac(log_n, 6, group_log);
            const G1CosetBatch one = g1_coset_batch(log_n, 6, group_log, 1, g1_coset_table_entries(log_n, 1));
            bool same = g1_coset_batch_launches(one) == g1_coset_mac_launches(m);
            for (uint64_t k = 0; k <= g1_coset_mac_launches(m); k++) same = same && g1_coset_batch_launch_lanes(one, k) == g1_coset_mac_launch_lanes(m, k);
            CHECK(same, "(%u,6) B=2^%u: one polynomial is not cut as the single path was", log_n, group_log);
        }
    }
    printf("g1 coset batch plan: %u shapes, %u cases, %d failures\n", shapes, cases, fails);
    return fails ? 1 : 0;
}
