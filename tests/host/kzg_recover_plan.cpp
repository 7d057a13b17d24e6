// csrc/kzg_recover_plan.hpp on its own, g++ only (tests/test_kzg_recover_plan_cpu.py builds it with -fsanitize=address,undefined).
// For every log_n <= 10, every log_l < log_n, leaf_log in {1, 2, the default} and m in {0, 1, 2^t - 1, 2^t, 2^t + 1, r / 2, r - 1}
// (t = leaf_log) it walks the step list the driver walks:
//   - the leaf launch takes every entry of the padded root list exactly once, in workgroups of at most 256 lanes;
//   - every range a step reads or writes lies inside the stated workspace, the ranges a step reads and writes are the same range or
//     do not overlap, and the pieces of the workspace do not overlap each other;
//   - the inversion pass takes each of the r values exactly once;
//   - the whole pipeline over F_65537 (3 generates its 2^16 roots of unity, the coset shift 7 is a generator too), run with exactly
//     these steps, offsets and index functions, gives back the polynomial the evaluations came from, flags altered input where the
//     present cells are more than enough, and does not read what stands at a missing position.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kzg_recover_plan.hpp"
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
static const uint64_t P = 65537;
static uint64_t powmod(uint64_t b, uint64_t e) {
    uint64_t r = 1;
    for (b %= P; e; e >>= 1, b = b * b % P)
        if (e & 1) r = r * b % P;
    return r;
}
static uint64_t root(unsigned log_n) { return powmod(3, 65536 >> log_n); }
static const uint64_t G = 7;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 33;
}

// `batch` transforms of 2^log, contiguous, in place, natural order in and out, as zkp_ntt_fr: forward multiplies element i by shift^i
// first; inverse divides by the size and then element i by shift^i
static void ntt(uint64_t* v, unsigned log, uint64_t batch, bool inverse, uint64_t shift) {
    const uint64_t n = (uint64_t)1 << log;
    uint64_t w = root(log);
    if (inverse) w = powmod(w, P - 2);
    std::vector<uint64_t> a(n);
    for (uint64_t b = 0; b < batch; b++, v += n) {
        uint64_t s = 1;
        for (uint64_t i = 0; i < n; i++, s = s * shift % P) a[i] = inverse ? v[i] : v[i] * s % P;
        for (uint64_t i = 0, j = 0; i < n; i++) {  // bit reversal
            if (i < j) std::swap(a[i], a[j]);
            uint64_t bit = n >> 1;
            for (; bit && (j & bit); bit >>= 1) j ^= bit;
            j |= bit;
        }
        for (uint64_t half = 1; half < n; half *= 2) {
            const uint64_t wl = powmod(w, n / (2 * half));
            for (uint64_t blk = 0; blk < n; blk += 2 * half) {
                uint64_t t = 1;
                for (uint64_t j = 0; j < half; j++, t = t * wl % P) {
                    const uint64_t x = a[blk + j], y = a[blk + j + half] * t % P;
                    a[blk + j] = (x + y) % P;
                    a[blk + j + half] = (x + P - y) % P;
                }
            }
        }
        const uint64_t ninv = powmod(n, P - 2), sinv = powmod(shift, P - 2);
        s = 1;
        for (uint64_t i = 0; i < n; i++, s = s * sinv % P) v[i] = inverse ? a[i] * ninv % P * s % P : a[i];
    }
}

struct Result {
    std::vector<uint64_t> coeffs, evals;
    bool inconsistent;
};

// The driver's walk.  Field elements of the workspace are one word each at byte offset / 32; the root list and the mask are kept aside
// (their byte ranges are checked like the others).
static Result run(unsigned log_n, unsigned log_l, unsigned leaf_log, const std::vector<uint64_t>& evals, const std::vector<uint8_t>& present,
                  uint64_t len) {
    const uint64_t n = (uint64_t)1 << log_n, r = n >> log_l;
    uint64_t m = 0;
    for (uint64_t k = 0; k < r; k++) m += present[k] ? 0 : 1;
    const KzgRecoverPlan p = kzg_recover_plan(log_n, log_l, leaf_log, m);
    const KzgRecoverSizes& z = p.sz;
    CHECK(p.roots >= m && (m == 0 || p.roots < 2 * m || p.roots == 1) && p.pad == p.roots - m && p.roots <= r, "(%u,%u) m %llu: %llu roots", log_n,
          log_l, (ull)m, (ull)p.roots);
    CHECK(m == 0 || (p.leaves << p.leaf_roots_log) == p.roots, "leaves");
    CHECK(p.leaf_roots_log <= KZG_RECOVER_MAX_LEAF_LOG && p.leaf_roots_log + p.levels == p.root_log, "levels");
    // the pieces of the workspace, in order, disjoint, inside total; the staging buffer likewise
    const size_t piece[8] = {z.vec, z.zs0, z.zs1, z.x, z.w, z.roots, z.mask, z.total};
    const size_t bytes[7] = {32 * n, 32 * r, 32 * r, 32 * r, 64 * r, 4 * r, r};
    for (int i = 0; i < 7; i++) CHECK(piece[i] + bytes[i] <= piece[i + 1] && piece[i] % (i < 5 ? 32 : 4) == 0, "piece %d of the workspace", i);
    CHECK(z.stage_roots + 4 * r <= z.stage_mask && z.stage_mask + r <= z.stage_total, "staging buffer");
    std::vector<uint64_t> ws(z.total / 32, 0xDEAD);
    std::vector<uint32_t> roots(p.roots);
    {
        uint64_t at = 0;
        for (uint64_t k = 0; k < r; k++)
            if (!present[k]) roots[at++] = (uint32_t)k;
        for (; at < p.roots; at++) roots[at] = KZG_RECOVER_PAD_ROOT;
    }
    const uint64_t rho = root(log_n - log_l), gl = powmod(G, (uint64_t)1 << log_l);
    Result res;
    res.coeffs.assign(len, 0xDEAD);
    res.evals.assign(n, 0xDEAD);
    res.inconsistent = false;
    unsigned level_steps = 0;
    for (unsigned i = 0; i < p.steps; i++) {
        const KzgRecoverStep s = kzg_recover_step(p, i);
        CHECK(s.in + s.in_bytes <= z.total && s.out + s.out_bytes <= z.total, "step %u (kind %d) leaves the workspace", i, (int)s.kind);
        CHECK((s.in == s.out && s.in_bytes == s.out_bytes) || s.in + s.in_bytes <= s.out || s.out + s.out_bytes <= s.in || !s.in_bytes ||
                  !s.out_bytes,
              "step %u (kind %d): ranges overlap", i, (int)s.kind);
        uint64_t* in = ws.data() + s.in / 32;
        uint64_t* out = ws.data() + s.out / 32;
        switch (s.kind) {
        case KZG_RECOVER_LEAF: {
            const uint64_t per = (uint64_t)1 << s.log;
            CHECK(s.in == z.roots && s.in_bytes == 4 * p.roots && s.lanes >= per && s.lanes <= 256 && s.lanes % 64 == 0 && s.batch == p.leaves,
                  "leaf launch");
            std::vector<int> taken(p.roots, 0);
            for (uint64_t q = 0; q < s.batch; q++) {
                std::vector<uint64_t> c(per, 0);
                for (uint64_t step = 0; step < per; step++) {
                    const uint64_t e = q * per + step;
                    taken[e]++;
                    const uint64_t a = roots[e] == KZG_RECOVER_PAD_ROOT ? 0 : powmod(rho, roots[e]);
                    std::vector<uint64_t> nv(step + 1);
                    for (uint64_t t = 0; t <= step; t++) nv[t] = ((t ? c[t - 1] : 0) + P - a * (t == step ? 1 : c[t]) % P) % P;
                    std::copy(nv.begin(), nv.end(), c.begin());
                }
                for (uint64_t t = 0; t < per; t++) out[q * per + t] = c[t];
            }
            for (uint64_t e = 0; e < p.roots; e++) CHECK(taken[e] == 1, "root entry %llu enters %d leaves", (ull)e, taken[e]);
            break;
        }
        case KZG_RECOVER_PAD:
            level_steps++;
            CHECK(s.lanes == 2 * p.roots && s.out_bytes == 64 * p.roots, "pad lanes");
            for (uint64_t k = 0; k < s.lanes; k++) {
                const int64_t src = kzg_recover_pad_source(s.log, k);
                CHECK(src < (int64_t)p.roots, "pad source");
                out[k] = src >= 0 ? in[src] : 0;
            }
            break;
        case KZG_RECOVER_TREE_FWD:
            CHECK((s.batch << s.log) == 2 * p.roots, "forward tree transforms");
            ntt(in, s.log, s.batch, false, 1);
            break;
        case KZG_RECOVER_PAIR:
            CHECK(s.lanes == p.roots && (s.batch << s.log) == p.roots, "pair lanes");
            for (uint64_t k = 0; k < s.lanes; k++) {
                const KzgRecoverPair pr = kzg_recover_pair(s.log, k);
                CHECK(pr.a < 2 * p.roots && pr.b < 2 * p.roots && pr.a != pr.b, "pair sources");
                const uint64_t a = in[pr.a], b = in[pr.b];
                out[k] = (a * b + (pr.minus ? 2 * P - a - b : a + b)) % P;
            }
            break;
        case KZG_RECOVER_TREE_INV:
            CHECK((s.batch << s.log) == p.roots, "inverse tree transforms");
            ntt(in, s.log, s.batch, true, 1);
            break;
        case KZG_RECOVER_ZS:
            CHECK(s.out == z.zs0 && z.zs1 == z.zs0 + 32 * r && s.lanes == r, "zs");
            for (uint64_t k = 0; k < p.pad; k++) CHECK(in[k] == 0, "coefficient %llu below the padding is not zero", (ull)k);
            for (uint64_t k = 0; k < r; k++) out[k] = out[r + k] = k < m ? in[p.pad + k] : k == m ? 1 : 0;
            break;
        case KZG_RECOVER_ZS_FWD: ntt(in, s.log, 1, false, 1); break;
        case KZG_RECOVER_ZS_SHIFT: ntt(in, s.log, 1, false, gl); break;
        case KZG_RECOVER_MUL:
            for (uint64_t k = 0; k < n; k++) out[k] = present[k & (r - 1)] ? evals[k] * in[k & (r - 1)] % P : 0;
            break;
        case KZG_RECOVER_COPY:
            for (uint64_t k = 0; k < n; k++) out[k] = evals[k];
            ntt(out, s.log, 1, true, 1);
            break;
        case KZG_RECOVER_N_INV: ntt(in, s.log, 1, true, 1); break;
        case KZG_RECOVER_N_SHIFT: ntt(in, s.log, 1, false, G); break;
        case KZG_RECOVER_INV: {
            std::vector<int> taken(r, 0);
            for (uint64_t t = 0; t < s.lanes; t++)
                for (unsigned c = 0; c < KZG_RECOVER_INV_CHUNK; c++) {
                    const uint64_t k = kzg_recover_inv_index(s.lanes, t, c);
                    if (k >= r) continue;
                    taken[k]++;
                    CHECK(in[k] != 0, "Zs vanishes on the shifted domain");
                    in[k] = powmod(in[k], P - 2);
                }
            for (uint64_t k = 0; k < r; k++) CHECK(taken[k] == 1, "value %llu inverted %d times", (ull)k, taken[k]);
            break;
        }
        case KZG_RECOVER_DIV:
            for (uint64_t k = 0; k < n; k++) out[k] = out[k] * in[k & (r - 1)] % P;
            break;
        case KZG_RECOVER_N_UNSHIFT: ntt(in, s.log, 1, true, G); break;
        case KZG_RECOVER_TAIL:
            CHECK(s.lanes == n, "tail lanes");
            for (uint64_t k = 0; k < n; k++) {
                if (k < len) res.coeffs[k] = in[k];
                else if (in[k]) res.inconsistent = true;
                res.evals[k] = k < len ? in[k] : 0;
            }
            break;
        case KZG_RECOVER_EVALS:
            CHECK(i == p.steps - 1, "the evaluations come last");
            ntt(res.evals.data(), s.log, 1, false, 1);
            break;
        }
    }
    CHECK(level_steps == p.levels, "%u pad steps for %u levels", level_steps, p.levels);
    return res;
}

int main() {
    unsigned pipelines = 0;
    for (unsigned log_n = 1; log_n <= 10; log_n++)
        for (unsigned log_l = 0; log_l < log_n; log_l++) {
            CHECK(kzg_recover_shape_ok(log_n, log_l), "shape");
            const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n / l;
            for (unsigned leaf_log : {1u, 2u, KZG_RECOVER_LEAF_LOG}) {
                std::vector<uint64_t> ms;
                for (uint64_t m : {(uint64_t)0, (uint64_t)1, ((uint64_t)1 << leaf_log) - 1, (uint64_t)1 << leaf_log, ((uint64_t)1 << leaf_log) + 1, r / 2, r - 1})
                    if (m < r && std::find(ms.begin(), ms.end(), m) == ms.end()) ms.push_back(m);
                for (uint64_t m : ms) {
                    std::vector<uint8_t> present(r, 1);
                    for (uint64_t left = m; left;) {
                        const uint64_t k = rnd() % r;
                        if (present[k]) present[k] = 0, left--;
                    }
                    const uint64_t cap = (r - m) * l;
                    for (uint64_t len : {cap, cap > l ? cap - l : cap}) {
                        if (len != cap && r - m < 2) continue;
                        CHECK(kzg_recoverable(log_n, log_l, m, len) && !kzg_recoverable(log_n, log_l, m, cap + 1), "recoverable");
                        std::vector<uint64_t> f(n, 0), ev;
                        for (uint64_t k = 0; k < len; k++) f[k] = rnd() % P;
                        ev = f;
                        ntt(ev.data(), log_n, 1, false, 1);
                        std::vector<uint64_t> given = ev;
                        for (uint64_t k = 0; k < n; k++)
                            if (!present[k & (r - 1)]) given[k] = 0xFFFFFFFFull;  // never read
                        const Result got = run(log_n, log_l, leaf_log, given, present, len);
                        pipelines++;
                        bool same = !got.inconsistent && got.evals == ev;
                        for (uint64_t k = 0; k < len; k++) same = same && got.coeffs[k] == f[k];
                        CHECK(same, "(%u,%u) leaf %u m %llu len %llu: not the polynomial", log_n, log_l, leaf_log, (ull)m, (ull)len);
                        // one altered present value: inconsistent iff the cells were more than enough
                        uint64_t at = rnd() % n;
                        while (!present[at & (r - 1)]) at = (at + 1) % n;
                        given[at] = (given[at] + 1) % P;
                        const Result bad = run(log_n, log_l, leaf_log, given, present, len);
                        CHECK(bad.inconsistent == (len < cap), "(%u,%u) leaf %u m %llu len %llu: altered input, inconsistent %d", log_n, log_l,
                              leaf_log, (ull)m, (ull)len, (int)bad.inconsistent);
                    }
                }
            }
        }
    CHECK(!kzg_recover_shape_ok(3, 3) && !kzg_recover_shape_ok(24, 6) && kzg_recover_shape_ok(23, 0) && !kzg_recover_shape_ok(0, 0), "shape range");
    {   // the worst case the workspace is sized for, and the largest shape: the tree of r - 1 roots has R = r
        const KzgRecoverPlan p = kzg_recover_plan(23, 0, KZG_RECOVER_LEAF_LOG, ((uint64_t)1 << 23) - 1);
        CHECK(p.roots == (uint64_t)1 << 23 && p.levels == 23 - KZG_RECOVER_LEAF_LOG && p.sz.total == ((size_t)1 << 23) * (32 * 6 + 5), "largest shape");
        for (unsigned i = 0; i < p.steps; i++) {
            const KzgRecoverStep s = kzg_recover_step(p, i);
            CHECK(s.in + s.in_bytes <= p.sz.total && s.out + s.out_bytes <= p.sz.total, "largest shape, step %u", i);
        }
    }
    printf("kzg recover plan: %u pipelines, %d failures\n", pipelines, fails);
    return fails ? 1 : 0;
}
