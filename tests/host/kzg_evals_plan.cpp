// csrc/kzg_evals_plan.hpp on its own, g++ only (tests/test_kzg_evals_plan_cpu.py builds it with -fsanitize=address,undefined).
// For every log_n in 1..13, both orders, P in {1, 2, 3, 5, 65} rows, once with every z outside the domain and once with rows whose z
// is w^0, w^(n-1), w^(n/2), another root, 0 and outside points mixed, it checks that
//   - the (workgroup, lane, k) triples of the geometry cover every position of a row exactly once, a workgroup's elements lie in its
//     own slice of ONE row (short workgroups below the span: one per row, idle lanes hold nothing), and the grids of the steps are
//     those of the geometry;
//   - the MSM groups partition the rows in order, none above 64 rows (32 over an endomorphism-split handle);
//   - the pieces of the workspace are disjoint, in order, 32-byte aligned and inside its total;
//   - the whole field pipeline over F_65537 (3 generates its 2^16 roots of unity), walked lane by lane with the plan's own index
//     functions in buffers of exactly the plan's sizes -- both levels of the inversion (the written-out chunk and the tree in LDS,
//     one inversion per workgroup), the partial sums and their finishing pass, the quotient at its natural index, and the second
//     pair of passes for a z of the domain -- gives f(z) by Horner's rule and the values of the synthetic division's quotient.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kzg_evals_plan.hpp"
using namespace zkp;

static int fails = 0;
#define CHECK(cond, ...)                     \
    do {                                     \
        if (!(cond)) {                       \
            if (fails++ < 20) {              \
                printf("FAIL " __VA_ARGS__); \
                printf("\n");                \
            }                                \
        }                                    \
    } while (0)

typedef unsigned long long ull;
static const uint64_t P = 65537;
static uint64_t powmod(uint64_t b, uint64_t e) {
    uint64_t r = 1;
    for (b %= P; e; e >>= 1, b = b * b % P)
        if (e & 1) r = r * b % P;
    return r;
}
static uint64_t inv(uint64_t a) { return powmod(a, P - 2); }
static uint64_t sub(uint64_t a, uint64_t b) { return (a + P - b) % P; }
static uint64_t root(unsigned log_n) { return powmod(3, 65536 >> log_n); }

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 33;
}

// values of the polynomial c (n coefficients) at w^j, j < n, natural order: radix 2, decimation in time
static std::vector<uint64_t> ntt(const std::vector<uint64_t>& c, unsigned log_n) {
    const uint32_t n = 1u << log_n;
    std::vector<uint64_t> a(n);
    for (uint32_t i = 0; i < n; i++) a[kzg_evals_bitrev(log_n, i)] = c[i];
    for (unsigned s = 1; s <= log_n; s++) {
        const uint32_t half = 1u << (s - 1);
        const uint64_t wm = root(s);
        for (uint32_t k = 0; k < n; k += 2 * half) {
            uint64_t w = 1;
            for (uint32_t j = 0; j < half; j++, w = w * wm % P) {
                const uint64_t u = a[k + j], v = a[k + j + half] * w % P;
                a[k + j] = (u + v) % P;
                a[k + j + half] = sub(u, v);
            }
        }
    }
    return a;
}

struct Lds {  // the tree of a workgroup
    std::vector<uint64_t> node;
    Lds() : node(2 * KZG_EVALS_THREADS, 0) {}
    template <class Op>
    void up(Op op) {
        for (uint32_t s = KZG_EVALS_THREADS / 2; s >= 1; s >>= 1)
            for (uint32_t t = 0; t < s; t++) node[s + t] = op(node[2 * (s + t)], node[2 * (s + t) + 1]);
    }
};
static uint64_t mul(uint64_t a, uint64_t b) { return a * b % P; }
static uint64_t add(uint64_t a, uint64_t b) { return (a + b) % P; }

static void check_geometry(unsigned log_n) {
    const KzgEvalsGeom g = kzg_evals_geom(log_n);
    const uint32_t n = 1u << log_n;
    CHECK((uint64_t)g.wg_elems * g.blocks == n, "log_n %u: the workgroups do not tile a row", log_n);
    CHECK(g.wg_elems <= (1u << KZG_EVALS_SPAN_LOG) && g.lanes <= KZG_EVALS_THREADS && g.lanes >= 1, "log_n %u: lanes", log_n);
    CHECK(log_n >= KZG_EVALS_SPAN_LOG ? g.lanes == KZG_EVALS_THREADS : g.blocks == 1, "log_n %u: a short workgroup is the only one of its row", log_n);
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t b = 0; b < g.blocks; b++)
        for (uint32_t t = 0; t < KZG_EVALS_THREADS; t++)
            for (uint32_t k = 0; k < KZG_EVALS_CHUNK; k++) {
                const uint32_t i = kzg_evals_element(g, b, t, k);
                if (i == KZG_EVALS_NONE) continue;
                CHECK(t < g.lanes, "log_n %u: an idle lane holds an element", log_n);
                CHECK(i < n && i / g.wg_elems == b, "log_n %u: element %u outside workgroup %u", log_n, i, b);
                if (i < n) seen[i]++;
            }
    for (uint32_t i = 0; i < n; i++) CHECK(seen[i] == 1, "log_n %u: position %u covered %u times", log_n, i, seen[i]);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t e = kzg_evals_exponent(KZG_EVALS_BITREV, log_n, i);
        CHECK(e < n && kzg_evals_position(KZG_EVALS_BITREV, log_n, e) == i, "log_n %u: bitrev is no involution at %u", log_n, i);
        CHECK(kzg_evals_exponent(KZG_EVALS_NATURAL, log_n, i) == i, "natural order");
    }
}

static void check_groups(uint64_t polys) {
    for (int split = 0; split < 2; split++) {
        uint64_t next = 0;
        for (uint64_t k = 0; k < kzg_evals_groups(polys, split != 0); k++) {
            const KzgEvalsGroup g = kzg_evals_group(polys, split != 0, k);
            CHECK(g.first == next && g.count >= 1 && g.count <= (split ? 32u : 64u), "P %llu split %d: group %llu", (ull)polys, split, (ull)k);
            next = g.first + g.count;
        }
        CHECK(next == polys, "P %llu split %d: the groups do not cover the rows", (ull)polys, split);
    }
}

static void check_sizes(unsigned log_n, uint64_t polys) {
    const KzgEvalsSizes s = kzg_evals_sizes(log_n, polys);
    const size_t n = (size_t)1 << log_n, b = kzg_evals_geom(log_n).blocks;
    const size_t off[8] = {s.roots, s.dinv, s.rows, s.partial, s.partial2, s.y, s.hit, s.total};
    const size_t len[7] = {32 * n, 32 * n * polys, 32 * n * polys, 32 * b * polys, 32 * b * polys, 32 * polys, 4 * polys};
    for (int i = 0; i < 7; i++) CHECK(off[i] % 32 == 0 && off[i] + len[i] <= off[i + 1], "log_n %u P %llu: piece %d", log_n, (ull)polys, i);
    CHECK(s.total % 32 == 0, "total");
}

// One call of `polys` rows; z_kind[p]: 0 outside the domain, 1 + m: z = w^m, -1: z = 0
static void pipeline(unsigned log_n, int order, uint64_t polys, bool mixed) {
    const uint32_t n = 1u << log_n;
    const KzgEvalsGeom g = kzg_evals_geom(log_n);
    const KzgEvalsSizes sz = kzg_evals_sizes(log_n, polys);
    const uint64_t w = root(log_n);
    // the workspace, in elements / words of exactly the plan's sizes
    std::vector<uint64_t> roots((sz.dinv - sz.roots) / 32), dinv((sz.rows - sz.dinv) / 32), quotient((sz.partial - sz.rows) / 32),
        partial((sz.partial2 - sz.partial) / 32), partial2((sz.y - sz.partial2) / 32), y((sz.hit - sz.y) / 32);
    std::vector<uint32_t> hit(polys);
    roots[0] = 1;
    for (uint32_t j = 1; j < n; j++) roots[j] = roots[j - 1] * w % P;
    // rows, points and the reference
    std::vector<uint64_t> evals((size_t)polys * n), z(polys), y_ref(polys), q_ref((size_t)polys * n);
    std::vector<int64_t> m_ref(polys, -1);
    for (uint64_t p = 0; p < polys; p++) {
        std::vector<uint64_t> c(n);
        for (uint32_t i = 0; i < n; i++) c[i] = rnd() % P;
        if (p % 7 == 5) std::fill(c.begin() + 1, c.end(), 0);  // a constant row
        const std::vector<uint64_t> v = ntt(c, log_n);
        for (uint32_t i = 0; i < n; i++) evals[kzg_evals_row_index(log_n, p, i)] = v[kzg_evals_exponent(order, log_n, i)];
        uint64_t zp = 0;
        const unsigned kind = mixed ? (unsigned)(p % 6) : 5;
        if (kind <= 3) {
            const uint32_t m = kind == 0 ? 0 : kind == 1 ? n - 1 : kind == 2 ? n / 2 : (uint32_t)(rnd() % n);
            zp = roots[m];
            m_ref[p] = m;
        } else if (kind == 5) {
            do zp = rnd() % P; while (powmod(zp, n) == 1);
        }
        z[p] = zp;
        // Horner and the synthetic division by X - z
        std::vector<uint64_t> qc(n, 0);
        uint64_t acc = 0;
        for (uint32_t i = n; i-- > 0;) {
            if (i + 1 < n) qc[i] = (c[i + 1] + zp * qc[i + 1]) % P;
            acc = (acc * zp + c[i]) % P;
        }
        y_ref[p] = acc;
        const std::vector<uint64_t> qv = ntt(qc, log_n);
        for (uint32_t j = 0; j < n; j++) q_ref[kzg_evals_row_index(log_n, p, j)] = qv[j];
    }
    const uint64_t ninv = inv(n);
    uint64_t inversions = 0;
    for (unsigned i = 0; i < KZG_EVALS_STEPS; i++) {
        const KzgEvalsStep s = kzg_evals_step(log_n, polys, i);
        switch (s.kind) {
        case KZG_EVALS_PRESET:
            CHECK(i == 0 && s.grid_x == 0, "the preset is the first step");
            for (uint64_t p = 0; p < polys; p++) hit[p] = KZG_EVALS_NONE;
            break;
        case KZG_EVALS_INVERT:
            CHECK(s.grid_x == g.blocks && s.grid_y == polys, "grid of the inversion");
            for (uint32_t p = 0; p < s.grid_y; p++)
                for (uint32_t b = 0; b < s.grid_x; b++) {
                    Lds lds;
                    uint64_t v[KZG_EVALS_THREADS][4], p1[KZG_EVALS_THREADS], p2[KZG_EVALS_THREADS];
                    bool zero[KZG_EVALS_THREADS][4];
                    for (uint32_t t = 0; t < KZG_EVALS_THREADS; t++) {
                        for (uint32_t k = 0; k < 4; k++) {
                            const uint32_t at = kzg_evals_element(g, b, t, k);
                            v[t][k] = 1;
                            zero[t][k] = false;
                            if (at == KZG_EVALS_NONE) continue;
                            const uint32_t e = kzg_evals_exponent(order, log_n, at);
                            v[t][k] = sub(roots[e], z[p]);
                            if (v[t][k] == 0) {
                                CHECK(hit[p] == KZG_EVALS_NONE, "two lanes write the word of row %u", p);
                                hit[p] = e;
                                zero[t][k] = true;
                                v[t][k] = 1;
                            }
                        }
                        p1[t] = v[t][0] * v[t][1] % P;
                        p2[t] = p1[t] * v[t][2] % P;
                        lds.node[kzg_evals_leaf(t)] = p2[t] * v[t][3] % P;
                    }
                    lds.up(mul);
                    CHECK(lds.node[1] != 0, "a zero product reaches the inversion");
                    lds.node[1] = inv(lds.node[1]);
                    inversions++;
                    for (uint32_t s2 = 1; s2 < KZG_EVALS_THREADS; s2 <<= 1) {
                        std::vector<uint64_t> nv(2 * s2);
                        for (uint32_t t = 0; t < 2 * s2; t++) nv[t] = lds.node[(2 * s2 + t) >> 1] * lds.node[(2 * s2 + t) ^ 1] % P;
                        for (uint32_t t = 0; t < 2 * s2; t++) lds.node[2 * s2 + t] = nv[t];
                    }
                    uint64_t term[KZG_EVALS_THREADS];
                    for (uint32_t t = 0; t < KZG_EVALS_THREADS; t++) {
                        uint64_t in = lds.node[kzg_evals_leaf(t)], x[4];
                        x[3] = in * p2[t] % P;
                        in = in * v[t][3] % P;
                        x[2] = in * p1[t] % P;
                        in = in * v[t][2] % P;
                        x[1] = in * v[t][0] % P;
                        x[0] = in * v[t][1] % P;
                        term[t] = 0;
                        for (uint32_t k = 4; k-- > 0;) {
                            const uint32_t at = kzg_evals_element(g, b, t, k);
                            if (at == KZG_EVALS_NONE) continue;
                            dinv[kzg_evals_row_index(log_n, p, at)] = x[k];
                            if (zero[t][k]) continue;
                            CHECK(x[k] * v[t][k] % P == 1, "an inverse is wrong");
                            term[t] = (term[t] + evals[kzg_evals_row_index(log_n, p, at)] * roots[kzg_evals_exponent(order, log_n, at)] % P * x[k]) % P;
                        }
                    }
                    for (uint32_t t = 0; t < KZG_EVALS_THREADS; t++) lds.node[kzg_evals_leaf(t)] = term[t];
                    lds.up(add);
                    partial[kzg_evals_partial_index(g, p, b)] = lds.node[1];
                }
            break;
        case KZG_EVALS_Y:
            CHECK(s.grid_x == 1 && s.grid_y == polys, "grid of y");
            for (uint32_t p = 0; p < s.grid_y; p++) {
                Lds lds;
                for (uint32_t t = 0; t < KZG_EVALS_THREADS; t++) {
                    uint64_t acc = 0;
                    for (uint32_t j = t; j < g.blocks; j += KZG_EVALS_THREADS) acc = (acc + partial[kzg_evals_partial_index(g, p, j)]) % P;
                    lds.node[kzg_evals_leaf(t)] = acc;
                }
                lds.up(add);
                if (hit[p] != KZG_EVALS_NONE) y[p] = evals[kzg_evals_row_index(log_n, p, kzg_evals_position(order, log_n, hit[p]))];
                else y[p] = sub(1, powmod(z[p], n)) * ninv % P * lds.node[1] % P;
            }
            break;
        case KZG_EVALS_QUOTIENT:
            CHECK(s.grid_x == g.blocks && s.grid_y == polys, "grid of the quotient");
            for (uint32_t p = 0; p < s.grid_y; p++)
                for (uint32_t b = 0; b < s.grid_x; b++) {
                    Lds lds;
                    const uint32_t m = hit[p];
                    for (uint32_t t = 0; t < KZG_EVALS_THREADS; t++) {
                        uint64_t acc = 0;
                        for (uint32_t k = 0; k < 4; k++) {
                            const uint32_t at = kzg_evals_element(g, b, t, k);
                            if (at == KZG_EVALS_NONE) continue;
                            const uint32_t e = kzg_evals_exponent(order, log_n, at);
                            if (e == m) continue;
                            const uint64_t q = sub(evals[kzg_evals_row_index(log_n, p, at)], y[p]) * dinv[kzg_evals_row_index(log_n, p, at)] % P;
                            quotient[kzg_evals_row_index(log_n, p, e)] = q;
                            if (m != KZG_EVALS_NONE) acc = (acc + q * roots[e]) % P;
                        }
                        lds.node[kzg_evals_leaf(t)] = acc;
                    }
                    if (m == KZG_EVALS_NONE) continue;
                    lds.up(add);
                    partial2[kzg_evals_partial_index(g, p, b)] = lds.node[1];
                }
            break;
        case KZG_EVALS_QM:
            CHECK(i == KZG_EVALS_STEPS - 1 && s.grid_x == 1 && s.grid_y == polys, "grid of q_m");
            for (uint32_t p = 0; p < s.grid_y; p++) {
                const uint32_t m = hit[p];
                if (m == KZG_EVALS_NONE) continue;
                Lds lds;
                for (uint32_t t = 0; t < KZG_EVALS_THREADS; t++) {
                    uint64_t acc = 0;
                    for (uint32_t j = t; j < g.blocks; j += KZG_EVALS_THREADS) acc = (acc + partial2[kzg_evals_partial_index(g, p, j)]) % P;
                    lds.node[kzg_evals_leaf(t)] = acc;
                }
                lds.up(add);
                const uint32_t back = (uint32_t)((((uint64_t)1 << log_n) - m) & (((uint64_t)1 << log_n) - 1));
                quotient[kzg_evals_row_index(log_n, p, m)] = sub(0, roots[back] * lds.node[1] % P);
            }
            break;
        }
    }
    CHECK(inversions == (uint64_t)g.blocks * polys, "one inversion per workgroup");
    for (uint64_t p = 0; p < polys; p++) {
        CHECK((m_ref[p] < 0) == (hit[p] == KZG_EVALS_NONE) && (m_ref[p] < 0 || (uint32_t)m_ref[p] == hit[p]), "log_n %u order %d row %llu: m", log_n, order,
              (ull)p);
        CHECK(y[p] == y_ref[p], "log_n %u order %d row %llu: y %llu, expected %llu", log_n, order, (ull)p, (ull)y[p], (ull)y_ref[p]);
        for (uint32_t j = 0; j < n; j++) {
            const size_t at = kzg_evals_row_index(log_n, p, j);
            if (quotient[at] != q_ref[at]) {
                CHECK(false, "log_n %u order %d row %llu: q[%u] %llu, expected %llu (m %lld)", log_n, order, (ull)p, j, (ull)quotient[at], (ull)q_ref[at],
                      (long long)m_ref[p]);
                break;
            }
        }
    }
}

int main() {
    int pipelines = 0;
    for (unsigned log_n = KZG_EVALS_MIN_LOG; log_n <= KZG_EVALS_MAX_LOG; log_n++) {
        const KzgEvalsGeom g = kzg_evals_geom(log_n);
        CHECK((uint64_t)g.wg_elems * g.blocks == (uint64_t)1 << log_n, "log_n %u: geometry", log_n);
        CHECK(kzg_evals_shape_ok(log_n), "shape");
    }
    CHECK(!kzg_evals_shape_ok(0) && !kzg_evals_shape_ok(25), "shape bounds");
    for (uint64_t polys : {1ull, 2ull, 3ull, 5ull, 31ull, 32ull, 33ull, 64ull, 65ull, 4096ull}) check_groups(polys);
    for (unsigned log_n = 1; log_n <= 13; log_n++) {
        check_geometry(log_n);
        for (uint64_t polys : {1ull, 2ull, 3ull, 5ull, 65ull}) {
            check_sizes(log_n, polys);
            for (int order : {KZG_EVALS_NATURAL, KZG_EVALS_BITREV})
                for (int mixed = 0; mixed < 2; mixed++) {
                    pipeline(log_n, order, polys, mixed != 0);
                    pipelines++;
                }
        }
    }
    printf("kzg evals plan: %d pipelines, %d failures\n", pipelines, fails);
    return fails ? 1 : 0;
}
