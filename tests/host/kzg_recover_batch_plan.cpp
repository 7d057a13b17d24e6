// What csrc/kzg_recover_plan.hpp adds for zkp_kzg_recover_cosets_batch, on its own, g++ only (tests/test_kzg_recover_batch_plan_cpu.py
// builds it with -fsanitize=address,undefined).  Over F_65537, for shapes from (2,1) to (10,6), polys in {1, 2, 3, 5, max_polys},
// both layouts and m in {0, 1, r/2, r - 1}, it walks the batch plan launch by launch and lane by lane, with the grids the driver
// uses and the index functions the kernels use:
//   - every lane of every n-sized step reads and writes inside its own row and inside the stated buffer, every element of a row is
//     written exactly once, the LDS slots of a tile are inside the tile and distinct, and what stands at a missing cell, between len
//     and stride, or in the rows behind `polys` of the workspace is neither read nor written;
//   - the two layout index maps are inverse bijections of a buffer of rows;
//   - kzg_recover_sizes_batch(..., 1) is kzg_recover_sizes field by field, and only what lies behind vec moves with max_polys;
//   - row p of a batch run -- coefficients, evaluations in the requested layout, inconsistency word -- is the single-plan pipeline
//     (kzg_recover_plan, polys = 1, natural order) on row p, and the polynomial the row came from; one altered value makes its own
//     row inconsistent and no other.
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
static const uint64_t NEVER = 0xFFFFFFFFull;  // stands where nothing may be read; no field element
static uint64_t powmod(uint64_t b, uint64_t e) {
    uint64_t r = 1;
    for (b %= P; e; e >>= 1, b = b * b % P)
        if (e & 1) r = r * b % P;
    return r;
}
static uint64_t root(unsigned log_n) { return powmod(3, 65536 >> log_n); }
static const uint64_t G = 7;

static uint64_t rng_state = 0x243F6A8885A308D3ull;
static uint64_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 33;
}

// `batch` transforms of 2^log, contiguous rows, natural order in and out, as zkp_ntt_fr: forward multiplies element i by shift^i first;
// inverse divides by the size and then element i by shift^i.  (A direct O(n^2) sum would do; this is the usual butterfly.)
static void ntt(uint64_t* v, unsigned log, uint64_t batch, bool inverse, uint64_t shift) {
    const uint64_t n = (uint64_t)1 << log;
    uint64_t w = root(log);
    if (inverse) w = powmod(w, P - 2);
    std::vector<uint64_t> a(n);
    for (uint64_t b = 0; b < batch; b++, v += n) {
        uint64_t s = 1;
        for (uint64_t i = 0; i < n; i++, s = s * shift % P) {
            CHECK(v[i] < P, "a transform reads what is no field element");
            a[i] = inverse ? v[i] % P : v[i] % P * s % P;
        }
        for (uint64_t i = 0, j = 0; i < n; i++) {
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
    std::vector<uint64_t> coeffs, evals;  // polys x stride, polys x n
    std::vector<uint32_t> inconsistent;   // polys
};

// A buffer of rows of n with the checks of an access by a lane that works on row `row`
struct Rows {
    uint64_t* v;
    uint64_t rows;
    unsigned log_n;
    std::vector<uint8_t> written;
    const char* name;
    Rows(uint64_t* v_, uint64_t rows_, unsigned log_n_, const char* name_) : v(v_), rows(rows_), log_n(log_n_), written((size_t)rows_ << log_n_, 0), name(name_) {}
    bool ok(uint64_t off, uint64_t row) {
        const bool in = off < (rows << log_n) && (off >> log_n) == row;
        CHECK(in, "%s: offset %llu is not in row %llu of %llu", name, (ull)off, (ull)row, (ull)rows);
        return in;
    }
    uint64_t rd(uint64_t off, uint64_t row) { return ok(off, row) ? v[off] : 0; }
    void wr(uint64_t off, uint64_t row, uint64_t x) {
        if (!ok(off, row)) return;
        CHECK(!written[off], "%s: offset %llu written twice in one step", name, (ull)off);
        written[off] = 1;
        v[off] = x;
    }
    void all_written() {
        for (size_t k = 0; k < written.size(); k++) CHECK(written[k], "%s: offset %llu not written", name, (ull)k);
    }
};

static const unsigned THREADS = KZG_RECOVER_THREADS;

// The driver's walk of a plan of `polys` rows.  Field elements of the workspace are one word each at byte offset / 32.  Steps up to
// the values of Zs are the single plan's (tests/host/kzg_recover_plan.cpp checks them lane by lane); here they are computed directly.
static Result run(const KzgRecoverPlan& p, const std::vector<uint64_t>& evals, const std::vector<uint8_t>& present, uint64_t len, uint64_t stride,
                  bool want_evals) {
    const unsigned log_n = p.log_n, log_l = p.log_l, log_r = p.log_r;
    const uint64_t n = (uint64_t)1 << log_n, r = (uint64_t)1 << log_r, B = p.polys;
    const KzgRecoverSizes& z = p.sz;
    const bool cells = p.layout == KZG_RECOVER_CELLS;
    std::vector<uint64_t> ws(z.total / 32 + 1, NEVER);
    Result res;
    res.coeffs.assign(B * stride, NEVER);
    res.evals.assign(B * n, NEVER);
    res.inconsistent.assign(B, 0);
    const uint64_t groups = kzg_recover_row_groups(B), blocks = (n + THREADS - 1) / THREADS, tiles = kzg_recover_tiles(log_n, log_l);
    const KzgRecoverTile tl = kzg_recover_tile(log_n, log_l);
    CHECK(tl.tk_log <= log_r && tl.tj_log <= log_l && tl.tk_log + tl.tj_log <= KZG_RECOVER_TILE_LOG && (tiles << (tl.tk_log + tl.tj_log)) == n,
          "(%u,%u): tile %u x %u", log_n, log_l, tl.tk_log, tl.tj_log);
    CHECK(((uint64_t)1 << tl.tk_log) * (((uint64_t)1 << tl.tj_log) + 1) <= KZG_RECOVER_TILE_SLOTS, "tile slots");
    const uint64_t gl = powmod(G, (uint64_t)1 << log_l), rho = root(log_r);
    uint64_t* zs0 = ws.data() + z.zs0 / 32;
    uint64_t* zs1 = ws.data() + z.zs1 / 32;
    uint64_t* vec = ws.data() + z.vec / 32;
    // one pass through the tiles: `load(p, k, j)` cell side or natural side in, `store` on the other side
    auto tiles_pass = [&](bool cell_side_in, auto&& load, auto&& store) {
        for (uint64_t by = 0; by < groups; by++)
            for (uint64_t q = 0; q < tiles; q++)
                for (uint64_t row = by * KZG_RECOVER_ROWS; row < std::min<uint64_t>(B, (by + 1) * KZG_RECOVER_ROWS); row++) {
                    std::vector<uint64_t> lds(KZG_RECOVER_TILE_SLOTS, NEVER);
                    std::vector<uint8_t> used(KZG_RECOVER_TILE_SLOTS, 0);
                    const uint32_t active = 1u << (tl.tk_log + tl.tj_log);
                    for (uint32_t t = 0; t < active; t++) {
                        const KzgRecoverTileAt a = kzg_recover_tile_at(log_n, log_l, q, t, cell_side_in);
                        CHECK(a.k < r && (a.j >> log_l) == 0 && a.slot < KZG_RECOVER_TILE_SLOTS && !used[a.slot], "tile %llu lane %u in", (ull)q, t);
                        if (a.slot >= KZG_RECOVER_TILE_SLOTS) continue;
                        used[a.slot] = 1;
                        lds[a.slot] = load(row, a.k, a.j);
                    }
                    for (uint32_t t = 0; t < active; t++) {
                        const KzgRecoverTileAt a = kzg_recover_tile_at(log_n, log_l, q, t, !cell_side_in);
                        CHECK(a.k < r && (a.j >> log_l) == 0 && a.slot < KZG_RECOVER_TILE_SLOTS && used[a.slot], "tile %llu lane %u out", (ull)q, t);
                        if (a.slot >= KZG_RECOVER_TILE_SLOTS) continue;
                        store(row, a.k, a.j, lds[a.slot]);
                    }
                }
    };
    // one pointwise pass: lane `i` of the n indices (the lanes of the last workgroup beyond n do nothing) for the rows of its group
    auto rows_pass = [&](auto&& lane) {
        for (uint64_t by = 0; by < groups; by++)
            for (uint64_t i = 0; i < blocks * THREADS; i++) {
                if (i >> log_n) continue;
                for (uint64_t row = by * KZG_RECOVER_ROWS; row < std::min<uint64_t>(B, (by + 1) * KZG_RECOVER_ROWS); row++) lane(row, i);
            }
    };
    bool saw_cells_out = false;
    for (unsigned i = 0; i < p.steps; i++) {
        const KzgRecoverStep s = kzg_recover_step(p, i);
        CHECK(s.in + s.in_bytes <= z.total && s.out + s.out_bytes <= z.total, "step %u (kind %d) leaves the workspace", i, (int)s.kind);
        const bool n_step = s.kind == KZG_RECOVER_MUL || s.kind == KZG_RECOVER_COPY || s.kind == KZG_RECOVER_N_INV || s.kind == KZG_RECOVER_N_SHIFT ||
                            s.kind == KZG_RECOVER_DIV || s.kind == KZG_RECOVER_N_UNSHIFT || s.kind == KZG_RECOVER_TAIL || s.kind == KZG_RECOVER_EVALS ||
                            s.kind == KZG_RECOVER_CELLS_OUT;
        if (n_step) CHECK(s.batch == B, "step %u (kind %d): batch %llu of %llu rows", i, (int)s.kind, (ull)s.batch, (ull)B);
        if (s.kind == KZG_RECOVER_MUL || s.kind == KZG_RECOVER_DIV || s.kind == KZG_RECOVER_TAIL || s.kind == KZG_RECOVER_CELLS_OUT)
            CHECK(s.lanes == n * groups, "step %u (kind %d): lanes", i, (int)s.kind);
        switch (s.kind) {
        case KZG_RECOVER_LEAF: case KZG_RECOVER_PAD: case KZG_RECOVER_TREE_FWD: case KZG_RECOVER_PAIR: case KZG_RECOVER_TREE_INV:
            CHECK(s.in >= z.x && s.out >= z.x, "a tree step touches vec");
            break;
        case KZG_RECOVER_ZS: {  // (the tree's result, directly: the coefficients of prod (Y - rho^k) over the missing k)
            std::vector<uint64_t> c(r + 1, 0);
            c[0] = 1;
            uint64_t deg = 0;
            for (uint64_t k = 0; k < r; k++) {
                if (present[k]) continue;
                const uint64_t a = powmod(rho, k);
                for (uint64_t d = ++deg; d >= 1; d--) c[d] = (c[d - 1] + P - a * c[d] % P) % P;
                c[0] = (P - a * c[0] % P) % P;
            }
            CHECK(s.out == z.zs0 && z.zs1 == z.zs0 + 32 * r && deg == p.m, "zs");
            for (uint64_t k = 0; k < r; k++) zs0[k] = zs1[k] = c[k];
            break;
        }
        case KZG_RECOVER_ZS_FWD: ntt(zs0, s.log, 1, false, 1); break;
        case KZG_RECOVER_ZS_SHIFT: ntt(zs1, s.log, 1, false, gl); break;
        case KZG_RECOVER_INV:
            for (uint64_t k = 0; k < r; k++) zs1[k] = powmod(zs1[k], P - 2);
            break;
        case KZG_RECOVER_MUL: {
            CHECK(s.out == z.vec && s.out_bytes == 32 * n * B && s.in == z.zs0, "mul ranges");
            Rows in(const_cast<uint64_t*>(evals.data()), B, log_n, "evaluations"), out(vec, B, log_n, "vec (mul)");
            if (cells)
                tiles_pass(true,
                           [&](uint64_t row, uint64_t k, uint64_t j) {
                               return present[k] ? in.rd(kzg_recover_offset(KZG_RECOVER_CELLS, log_n, log_l, row, k + (j << log_r)), row) * zs0[k] % P : 0;
                           },
                           [&](uint64_t row, uint64_t k, uint64_t j, uint64_t v) {
                               out.wr(kzg_recover_offset(KZG_RECOVER_NATURAL, log_n, log_l, row, k + (j << log_r)), row, v);
                           });
            else
                rows_pass([&](uint64_t row, uint64_t e) {
                    const uint64_t k = e & (r - 1), at = kzg_recover_offset(KZG_RECOVER_NATURAL, log_n, log_l, row, e);
                    out.wr(at, row, present[k] ? in.rd(at, row) * zs0[k] % P : 0);
                });
            out.all_written();
            break;
        }
        case KZG_RECOVER_COPY: {
            CHECK(s.out == z.vec && s.out_bytes == 32 * n * B, "copy ranges");
            if (cells) {
                Rows in(const_cast<uint64_t*>(evals.data()), B, log_n, "evaluations"), out(vec, B, log_n, "vec (copy)");
                tiles_pass(true, [&](uint64_t row, uint64_t k, uint64_t j) { return in.rd(kzg_recover_offset(KZG_RECOVER_CELLS, log_n, log_l, row, k + (j << log_r)), row); },
                           [&](uint64_t row, uint64_t k, uint64_t j, uint64_t v) {
                               out.wr(kzg_recover_offset(KZG_RECOVER_NATURAL, log_n, log_l, row, k + (j << log_r)), row, v);
                           });
                out.all_written();
            } else {
                std::copy(evals.begin(), evals.begin() + B * n, vec);
            }
            ntt(vec, s.log, s.batch, true, 1);
            break;
        }
        case KZG_RECOVER_N_INV: ntt(ws.data() + s.in / 32, s.log, s.batch, true, 1); break;
        case KZG_RECOVER_N_SHIFT: ntt(ws.data() + s.in / 32, s.log, s.batch, false, G); break;
        case KZG_RECOVER_DIV: {
            CHECK(s.out == z.vec && s.out_bytes == 32 * n * B && s.in == z.zs1, "div ranges");
            Rows a(vec, B, log_n, "vec (div)");
            rows_pass([&](uint64_t row, uint64_t e) {
                const uint64_t at = (row << log_n) + e;
                a.wr(at, row, a.rd(at, row) * zs1[e & (r - 1)] % P);
            });
            a.all_written();
            break;
        }
        case KZG_RECOVER_N_UNSHIFT: ntt(ws.data() + s.in / 32, s.log, s.batch, true, G); break;
        case KZG_RECOVER_TAIL: {
            CHECK(s.in == z.vec && s.in_bytes == 32 * n * B && (cells ? s.out == z.vec && s.out_bytes == 32 * n * B : s.out_bytes == 0), "tail ranges");
            Rows a(vec, B, log_n, "vec (tail)");
            uint64_t* padded = !want_evals ? nullptr : cells ? ws.data() + s.out / 32 : res.evals.data();
            rows_pass([&](uint64_t row, uint64_t e) {
                const uint64_t at = (row << log_n) + e, v = a.rd(at, row);
                if (e < len) {
                    CHECK(row * stride + e < res.coeffs.size(), "coefficient out of its buffer");
                    res.coeffs[row * stride + e] = v;
                    if (padded && padded != vec) padded[at] = v;
                } else {
                    if (v) res.inconsistent[row] = 1;
                    if (padded) padded[at] = 0;
                }
            });
            break;
        }
        case KZG_RECOVER_EVALS:
            CHECK(i == p.steps - (cells ? 2 : 1), "the evaluations come last but for the transposition");
            if (want_evals) ntt(cells ? ws.data() + s.in / 32 : res.evals.data(), s.log, s.batch, false, 1);
            break;
        default: {  // KZG_RECOVER_CELLS_OUT
            CHECK(s.kind == KZG_RECOVER_CELLS_OUT && cells && i == p.steps - 1 && s.in == z.vec && s.in_bytes == 32 * n * B, "the transposition comes last, in cell layout only");
            saw_cells_out = true;
            if (!want_evals) break;
            Rows in(vec, B, log_n, "vec (cells out)"), out(res.evals.data(), B, log_n, "evaluations out");
            tiles_pass(false, [&](uint64_t row, uint64_t k, uint64_t j) { return in.rd(kzg_recover_offset(KZG_RECOVER_NATURAL, log_n, log_l, row, k + (j << log_r)), row); },
                       [&](uint64_t row, uint64_t k, uint64_t j, uint64_t v) {
                           out.wr(kzg_recover_offset(KZG_RECOVER_CELLS, log_n, log_l, row, k + (j << log_r)), row, v);
                       });
            out.all_written();
            break;
        }
        }
    }
    CHECK(saw_cells_out == cells, "cell layout and its last step");
    // what lies behind the rows of the call in vec (a handle made for more) was never touched
    for (uint64_t k = B * n; k < z.zs0 / 32; k++) CHECK(ws[k] == NEVER, "vec behind the last row was written");
    return res;
}

int main() {
    unsigned shapes = 0, cases = 0;
    const uint64_t MAX_POLYS = 9;  // three groups of rows, the last one partial
    const unsigned shape_list[][2] = {{2, 1}, {3, 1}, {4, 2}, {5, 0}, {6, 0}, {6, 3}, {7, 6}, {8, 4}, {9, 1}, {10, 2}, {10, 6}};
    for (const auto& sh : shape_list) {
        const unsigned log_n = sh[0], log_l = sh[1];
        shapes++;
        const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n / l;
        {   // sizes: at one polynomial the single sizes; else only vec grows
            const KzgRecoverSizes a = kzg_recover_sizes(log_n, log_l), b = kzg_recover_sizes_batch(log_n, log_l, 1), c = kzg_recover_sizes_batch(log_n, log_l, MAX_POLYS);
            CHECK(a.vec == b.vec && a.zs0 == b.zs0 && a.zs1 == b.zs1 && a.x == b.x && a.w == b.w && a.roots == b.roots && a.mask == b.mask &&
                      a.total == b.total && a.stage_roots == b.stage_roots && a.stage_mask == b.stage_mask && a.stage_total == b.stage_total,
                  "(%u,%u): sizes of a batch of one", log_n, log_l);
            const size_t grow = 32 * n * (MAX_POLYS - 1);
            CHECK(c.vec == 0 && c.zs0 == a.zs0 + grow && c.zs1 == a.zs1 + grow && c.x == a.x + grow && c.w == a.w + grow && c.roots == a.roots + grow &&
                      c.mask == a.mask + grow && c.total == a.total + grow && c.stage_total == a.stage_total && c.zs0 == 32 * n * MAX_POLYS,
                  "(%u,%u): sizes of a batch", log_n, log_l);
        }
        for (int layout : {KZG_RECOVER_NATURAL, KZG_RECOVER_CELLS}) {  // the maps, on a buffer of three rows
            std::vector<int> hit(3 * n, 0);
            for (uint64_t row = 0; row < 3; row++)
                for (uint64_t i = 0; i < n; i++) {
                    const uint64_t off = kzg_recover_offset(layout, log_n, log_l, row, i);
                    CHECK(off < 3 * n && (off >> log_n) == row, "offset leaves its row");
                    if (off >= 3 * n) continue;
                    hit[off]++;
                    const KzgRecoverRowIndex back = kzg_recover_index(layout, log_n, log_l, off);
                    CHECK(back.p == row && back.i == i, "(%u,%u) layout %d: index(offset(%llu, %llu))", log_n, log_l, layout, (ull)row, (ull)i);
                    const uint64_t k = i & (r - 1), j = i >> (log_n - log_l);
                    CHECK(off == row * n + (layout == KZG_RECOVER_CELLS ? k * l + j : k + j * r), "the layout's definition");
                }
            for (uint64_t off = 0; off < 3 * n; off++) {
                const KzgRecoverRowIndex x = kzg_recover_index(layout, log_n, log_l, off);
                CHECK(hit[off] == 1 && x.i < n && kzg_recover_offset(layout, log_n, log_l, x.p, x.i) == off, "offset(index(%llu))", (ull)off);
            }
        }
        std::vector<uint64_t> ms;
        for (uint64_t m : {(uint64_t)0, (uint64_t)1, r / 2, r - 1})
            if (std::find(ms.begin(), ms.end(), m) == ms.end()) ms.push_back(m);
        for (uint64_t m : ms) {
            std::vector<uint8_t> present(r, 1);
            for (uint64_t left = m; left;) {
                const uint64_t k = rnd() % r;
                if (present[k]) present[k] = 0, left--;
            }
            const uint64_t cap = (r - m) * l, len = cap > l ? cap - l : cap;  // one surplus cell where there is one
            CHECK(kzg_recoverable(log_n, log_l, m, len), "recoverable");
            for (uint64_t polys : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)5, MAX_POLYS})
                for (int layout : {KZG_RECOVER_NATURAL, KZG_RECOVER_CELLS}) {
                    cases++;
                    const uint64_t stride = len + (polys & 1 ? 3 : 0);
                    // rows of natural-order evaluations, the missing positions never to be read; row `bad` (where there is a surplus) altered
                    std::vector<uint64_t> f(polys * n, 0), ev, given, laid(polys * n);
                    for (uint64_t row = 0; row < polys; row++)
                        for (uint64_t k = 0; k < len; k++) f[row * n + k] = rnd() % P;
                    ev = f;
                    ntt(ev.data(), log_n, polys, false, 1);
                    given = ev;
                    const uint64_t bad = rnd() % polys;
                    if (len < cap) {
                        uint64_t at = rnd() % n;
                        while (!present[at & (r - 1)]) at = (at + 1) % n;
                        given[bad * n + at] = (given[bad * n + at] + 1) % P;
                    }
                    for (uint64_t k = 0; k < polys * n; k++)
                        if (!present[k & (r - 1)]) given[k] = NEVER;
                    for (uint64_t row = 0; row < polys; row++)
                        for (uint64_t i = 0; i < n; i++) laid[kzg_recover_offset(layout, log_n, log_l, row, i)] = given[row * n + i];
                    const KzgRecoverPlan bp = kzg_recover_plan_batch(log_n, log_l, KZG_RECOVER_LEAF_LOG, m, polys, layout, MAX_POLYS);
                    const KzgRecoverPlan sp = kzg_recover_plan(log_n, log_l, KZG_RECOVER_LEAF_LOG, m);
                    CHECK(bp.steps == sp.steps + (layout == KZG_RECOVER_CELLS ? 1 : 0) && sp.polys == 1 && sp.layout == KZG_RECOVER_NATURAL, "steps");
                    for (unsigned i = 0; i < sp.steps; i++) {  // the same steps in the same order; up to the values of Zs the same launches
                        const KzgRecoverStep a = kzg_recover_step(sp, i), b = kzg_recover_step(bp, i);
                        CHECK(a.kind == b.kind && a.log == b.log, "step %u: kind", i);
                        if (a.in >= sp.sz.zs0 && a.kind != KZG_RECOVER_MUL && a.kind != KZG_RECOVER_DIV)
                            CHECK(a.batch == b.batch && a.lanes == b.lanes && a.in_bytes == b.in_bytes && a.out_bytes == b.out_bytes &&
                                      b.in - a.in == bp.sz.zs0 - sp.sz.zs0 && b.out - a.out == bp.sz.zs0 - sp.sz.zs0,
                                  "step %u (kind %d): a step of the vanishing polynomial differs", i, (int)a.kind);
                    }
                    const bool want = (cases & 3) != 0;
                    const Result got = run(bp, laid, present, len, stride, want);
                    for (uint64_t row = 0; row < polys; row++) {
                        const std::vector<uint64_t> one(given.begin() + row * n, given.begin() + (row + 1) * n);
                        const Result ref = run(sp, one, present, len, len, true);
                        bool same = got.inconsistent[row] == ref.inconsistent[0];
                        for (uint64_t k = 0; k < len; k++) same = same && got.coeffs[row * stride + k] == ref.coeffs[k];
                        for (uint64_t k = len; k < stride; k++) same = same && got.coeffs[row * stride + k] == NEVER;
                        for (uint64_t i = 0; i < n; i++)
                            same = same && got.evals[kzg_recover_offset(layout, log_n, log_l, row, i)] == (want ? ref.evals[i] : NEVER);
                        CHECK(same, "(%u,%u) m %llu polys %llu layout %d row %llu: not the single pipeline's row", log_n, log_l, (ull)m, (ull)polys, layout,
                              (ull)row);
                        const bool altered = len < cap && row == bad;
                        CHECK(got.inconsistent[row] == (altered ? 1u : 0u), "(%u,%u) m %llu polys %llu row %llu: inconsistent %u, altered %d", log_n, log_l,
                              (ull)m, (ull)polys, (ull)row, got.inconsistent[row], (int)altered);
                        if (!altered) {
                            bool truth = true;
                            for (uint64_t k = 0; k < len; k++) truth = truth && got.coeffs[row * stride + k] == f[row * n + k];
                            for (uint64_t i = 0; want && i < n; i++) truth = truth && ref.evals[i] == ev[row * n + i];
                            CHECK(truth, "(%u,%u) m %llu polys %llu row %llu: not the polynomial", log_n, log_l, (ull)m, (ull)polys, (ull)row);
                        }
                    }
                }
        }
    }
    {   // the largest handle: 4096 rows of 2^23 stay inside size_t arithmetic, and the steps inside the workspace
        const KzgRecoverPlan p = kzg_recover_plan_batch(23, 6, KZG_RECOVER_LEAF_LOG, 5, KZG_RECOVER_MAX_POLYS, KZG_RECOVER_CELLS, KZG_RECOVER_MAX_POLYS);
        CHECK(p.sz.zs0 == ((size_t)32 << 23) * KZG_RECOVER_MAX_POLYS, "largest handle");
        for (unsigned i = 0; i < p.steps; i++) {
            const KzgRecoverStep s = kzg_recover_step(p, i);
            CHECK(s.in + s.in_bytes <= p.sz.total && s.out + s.out_bytes <= p.sz.total, "largest handle, step %u", i);
        }
    }
    printf("kzg recover batch plan: %u shapes, %u cases, %d failures\n", shapes, cases, fails);
    return fails ? 1 : 0;
}
