// csrc/kzg_cells_plan.hpp on its own, g++ only (tests/test_kzg_cells_plan_cpu.py builds it with -fsanitize=address,undefined).
// For every log_n <= 7, every log_l < log_n, chunk logs 0, 1 and the default, and a list of random and adversarial batches (all
// cells in one coset, one cell, every coset once, N = max_cells, no cell at all, one commitment, duplicates) it builds the tables
// the driver builds, in buffers of exactly the sizes the plan reports (the sanitizer sees every index), and checks that
//   - each sort holds every cell exactly once, segments are contiguous, in key order, and keep the batch order inside a key;
//   - no chunk is empty, exceeds 2^chunk_log cells or crosses a segment; the chunk counts respect the bounds the sizes are made from;
//   - the table of the call fits the verifier's, and the pieces of the workspace are disjoint and inside its total;
//   - the whole field pipeline over F_65537 (3 generates its 2^16 roots of unity), walked lane by lane with exactly these tables and
//     index functions -- aggregate, combine, inverse transform, tail, scalars, commitment weights --, gives the sum of the weighted
//     interpolants computed cell by cell, the sums of the weights and rho_i c_i.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "kzg_cells_plan.hpp"
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 33;
}

// the inverse transform of 2^log values, natural order in and out, by the definition (the sizes here are small)
static std::vector<uint64_t> intt(const std::vector<uint64_t>& v, unsigned log) {
    const uint64_t n = (uint64_t)1 << log, winv = powmod(root(log), P - 2), ninv = powmod(n, P - 2);
    std::vector<uint64_t> out(n), pw(n, 1);
    for (uint64_t k = 1; k < n; k++) pw[k] = pw[k - 1] * winv % P;
    for (uint64_t i = 0; i < n; i++) {
        uint64_t acc = 0;
        for (uint64_t j = 0; j < n; j++) acc = (acc + v[j] * pw[i * j % n]) % P;
        out[i] = acc * ninv % P;
    }
    return out;
}

struct Batch {
    std::vector<uint32_t> commit, coset;
};

static void run(unsigned log_n, unsigned log_l, unsigned chunk_log, uint64_t max_cells, uint64_t max_commits, const Batch& b, uint64_t commits) {
    const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l, N = b.coset.size(), per = (uint64_t)1 << chunk_log;
    const unsigned log_r = log_n - log_l;
    const KzgCellsSizes sz = kzg_cells_sizes(log_n, log_l, chunk_log, max_cells, max_commits);
    {   // the pieces of the workspace, in order, disjoint, inside total
        const size_t piece[9] = {sz.a, sz.partial, sz.cpartial, sz.interp, sz.sc_right, sz.sc_left, sz.report, sz.table, sz.total};
        const size_t bytes[8] = {32 * n, 32 * l * sz.max_chunks, 32 * sz.max_cchunks, 32 * l, 32 * (max_commits + max_cells),
                                 32 * (max_commits + max_cells), 64, 4 * sz.table_words};
        for (int i = 0; i < 8; i++) CHECK(piece[i] + bytes[i] <= piece[i + 1] && piece[i] % 32 == 0, "piece %d of the workspace", i);
        CHECK(sz.stage_total == 4 * sz.table_words && sz.scratch_words >= r + 1 && sz.scratch_words >= max_commits + 1, "staging and scratch");
    }
    std::vector<uint32_t> scratch(sz.scratch_words), table(sz.table_words, 0xDEADBEEFu);
    const KzgCellsTables t = kzg_cells_tables(log_n, log_l, chunk_log, b.commit.data(), b.coset.data(), N, commits, scratch.data(), table.data());
    CHECK(t.words <= sz.table_words, "(%u,%u) N %llu: a table of %llu words in %llu", log_n, log_l, (ull)N, (ull)t.words, (ull)sz.table_words);
    CHECK(t.chunks <= sz.max_chunks && t.cchunks <= sz.max_cchunks && t.used <= sz.max_used, "chunk bounds");
    CHECK(t.chunks <= kzg_cells_max_chunks(N, r, chunk_log) && t.cchunks <= kzg_cells_max_chunks(N, commits, chunk_log), "chunk bounds of the call");
    {   // the pieces of the table, in order, disjoint
        const size_t piece[9] = {t.by_coset, t.chunk_start, t.used_coset, t.seg_chunk, t.cell_coset, t.by_commit, t.cchunk_start, t.cseg_chunk, t.words};
        const size_t words[8] = {N, t.chunks + 1, t.used, t.used + 1, N, N, t.cchunks + 1, commits + 1};
        for (int i = 0; i < 8; i++) CHECK(piece[i] + words[i] == piece[i + 1], "piece %d of the table", i);
    }
    // the two sorts
    for (int which = 0; which < 2; which++) {
        const uint32_t* key = which ? b.commit.data() : b.coset.data();
        const uint32_t* order = &table[which ? t.by_commit : t.by_coset];
        const uint32_t* cstart = &table[which ? t.cchunk_start : t.chunk_start];
        const uint32_t* seg = &table[which ? t.cseg_chunk : t.seg_chunk];
        const uint64_t chunks = which ? t.cchunks : t.chunks, segs = which ? commits : t.used;
        std::vector<int> seen(N, 0);
        for (uint64_t i = 0; i < N; i++) {
            CHECK(order[i] < N, "cell id");
            if (order[i] < N) seen[order[i]]++;
            if (i) CHECK(key[order[i - 1]] < key[order[i]] || (key[order[i - 1]] == key[order[i]] && order[i - 1] < order[i]), "sort %d: order at %llu", which, (ull)i);
        }
        for (uint64_t i = 0; i < N; i++) CHECK(seen[i] == 1, "sort %d: cell %llu appears %d times", which, (ull)i, seen[i]);
        CHECK(cstart[0] == 0 || (chunks == 0 && cstart[0] == N), "first chunk");
        CHECK(cstart[chunks] == N && seg[0] == 0 && seg[segs] == chunks, "ends");
        for (uint64_t u = 0; u < segs; u++) {
            const uint32_t k = which ? (uint32_t)u : table[t.used_coset + u];
            if (!which) CHECK(k < r && (!u || table[t.used_coset + u - 1] < k), "used cosets ascend");
            CHECK(seg[u] <= seg[u + 1] && (which || seg[u] < seg[u + 1]), "segment %llu", (ull)u);
            uint64_t members = 0;
            for (uint32_t q = seg[u]; q < seg[u + 1]; q++) {
                const uint64_t len = cstart[q + 1] - cstart[q];
                CHECK(len >= 1 && len <= per, "sort %d: chunk %u of %llu cells", which, q, (ull)len);
                CHECK(q + 1 == seg[u + 1] || len == per, "only the last chunk of a segment is short");
                for (uint32_t at = cstart[q]; at < cstart[q + 1]; at++, members++) CHECK(key[order[at]] == k, "sort %d: chunk %u crosses a segment", which, q);
            }
            uint64_t want = 0;
            for (uint64_t i = 0; i < N; i++) want += key[i] == k;
            CHECK(members == want, "sort %d: key %u has %llu of %llu cells", which, k, (ull)members, (ull)want);
        }
    }
    for (uint64_t i = 0; i < N; i++) CHECK(table[t.cell_coset + i] == b.coset[i], "coset of cell %llu", (ull)i);

    // the field pipeline, lane by lane, in buffers of the sizes the plan reports
    std::vector<uint64_t> evals(N * l), weights(N), a(n, 0xDEAD), partial(sz.max_chunks * l, 0xDEAD), cpartial(sz.max_cchunks, 0xDEAD), interp(l, 0xDEAD),
        cw(commits, 0xDEAD), ps(N, 0xDEAD);
    for (uint64_t& v : evals) v = rnd() % P;
    for (uint64_t& v : weights) v = rnd() % P;
    if (N > 2) weights[1] = 0;
    const uint64_t rho = root(log_r);
    for (unsigned i = 0; i < KZG_CELLS_STEPS; i++) {
        const KzgCellsStep s = kzg_cells_step(log_l, t, i);
        switch (s.kind) {
        case KZG_CELLS_ZERO: std::fill(a.begin(), a.end(), 0); break;
        case KZG_CELLS_AGGREGATE:
            CHECK(s.lanes == t.chunks * l, "aggregate lanes");
            for (uint64_t lane = 0; lane < s.lanes; lane++) {
                const uint64_t q = lane >> log_l, j = lane & (l - 1);
                uint64_t acc = 0;
                for (uint32_t at = table[t.chunk_start + q]; at < table[t.chunk_start + q + 1]; at++) {
                    const uint32_t cell = table[t.by_coset + at];
                    acc = (acc + weights.at(cell) * evals.at(kzg_cells_eval_index(log_l, cell, j))) % P;
                }
                partial.at(kzg_cells_partial_index(log_l, q, j)) = acc;
            }
            break;
        case KZG_CELLS_COMBINE:
            CHECK(s.lanes == t.used * l, "combine lanes");
            for (uint64_t lane = 0; lane < s.lanes; lane++) {
                const uint64_t u = lane >> log_l, j = lane & (l - 1);
                uint64_t acc = 0;
                for (uint32_t q = table[t.seg_chunk + u]; q < table[t.seg_chunk + u + 1]; q++) acc = (acc + partial.at(kzg_cells_partial_index(log_l, q, j))) % P;
                a.at(kzg_cells_a_index(log_r, table[t.used_coset + u], j)) = acc;
            }
            break;
        case KZG_CELLS_NTT: a = intt(a, log_n); break;
        case KZG_CELLS_TAIL:
            CHECK(s.lanes == l, "tail lanes");
            for (uint64_t j = 0; j < s.lanes; j++) interp[j] = a[j] * (r % P) % P;
            break;
        case KZG_CELLS_SCALARS:
            CHECK(s.lanes == N + t.cchunks, "scalar lanes");
            for (uint64_t lane = 0; lane < s.lanes; lane++) {
                if (lane < N) {
                    ps[lane] = weights[lane] * powmod(rho, table[t.cell_coset + lane]) % P;
                } else {
                    const uint64_t q = lane - N;
                    uint64_t acc = 0;
                    for (uint32_t at = table[t.cchunk_start + q]; at < table[t.cchunk_start + q + 1]; at++) acc = (acc + weights.at(table[t.by_commit + at])) % P;
                    cpartial.at(q) = acc;
                }
            }
            break;
        case KZG_CELLS_COMMITS:
            CHECK(s.lanes == commits, "commit lanes");
            for (uint64_t m = 0; m < s.lanes; m++) {
                uint64_t acc = 0;
                for (uint32_t q = table[t.cseg_chunk + m]; q < table[t.cseg_chunk + m + 1]; q++) acc = (acc + cpartial.at(q)) % P;
                cw[m] = acc;
            }
            break;
        }
    }
    // the definition: every cell's interpolant, coefficient i = x_k^-i times coefficient i of the inverse transform of l of its values
    std::vector<uint64_t> want(l, 0), want_cw(commits, 0);
    const uint64_t w = root(log_n);
    for (uint64_t i = 0; i < N; i++) {
        const std::vector<uint64_t> c = intt(std::vector<uint64_t>(evals.begin() + i * l, evals.begin() + (i + 1) * l), log_l);
        const uint64_t xinv = powmod(powmod(w, b.coset[i]), P - 2);
        for (uint64_t j = 0; j < l; j++) want[j] = (want[j] + weights[i] * (c[j] * powmod(xinv, j) % P)) % P;
        want_cw[b.commit[i]] = (want_cw[b.commit[i]] + weights[i]) % P;
        CHECK(ps[i] == weights[i] * powmod(w, (uint64_t)b.coset[i] * l) % P, "proof scalar %llu", (ull)i);
    }
    CHECK(interp == want, "(%u,%u) chunk %u N %llu: not the sum of the interpolants", log_n, log_l, chunk_log, (ull)N);
    CHECK(cw == want_cw, "(%u,%u) chunk %u N %llu: commitment weights", log_n, log_l, chunk_log, (ull)N);
}

int main() {
    unsigned pipelines = 0;
    for (unsigned log_n = 1; log_n <= 7; log_n++)
        for (unsigned log_l = 0; log_l < log_n; log_l++) {
            CHECK(kzg_cells_shape_ok(log_n, log_l), "shape");
            const uint64_t r = (uint64_t)1 << (log_n - log_l);
            for (unsigned chunk_log : {0u, 1u, KZG_CELLS_CHUNK_LOG}) {
                const uint64_t max_cells = 40, max_commits = 5;
                std::vector<std::pair<Batch, uint64_t>> batches;
                auto add = [&](uint64_t cells, uint64_t commits, int mode) {
                    Batch b;
                    for (uint64_t i = 0; i < cells; i++) {
                        b.commit.push_back((uint32_t)(mode == 3 ? commits - 1 : rnd() % commits));
                        b.coset.push_back((uint32_t)(mode == 1 ? r - 1 : mode == 2 ? i % r : rnd() % r));
                    }
                    if (mode == 4 && cells > 4) b.commit[4] = b.commit[0], b.coset[4] = b.coset[0];  // the same cell twice
                    batches.push_back({b, commits});
                };
                add(1, 1, 0);                                   // one cell
                add(1, max_commits, 3);
                add(max_cells, 3, 1);                           // all cells in one coset, N = max_cells
                add(std::min<uint64_t>(r, max_cells), 2, 2);    // every coset once
                add(max_cells, max_commits, 0);                 // N = max_cells, M = max_commits
                add(max_cells, 1, 0);                           // one commitment
                add(0, 2, 0);                                   // no cell
                for (int k = 0; k < 20; k++) add(1 + rnd() % max_cells, 1 + rnd() % max_commits, k % 2 ? 4 : 0);
                for (const auto& bc : batches) {
                    run(log_n, log_l, chunk_log, max_cells, max_commits, bc.first, bc.second);
                    pipelines++;
                }
            }
        }
    CHECK(!kzg_cells_shape_ok(3, 3) && !kzg_cells_shape_ok(24, 6) && kzg_cells_shape_ok(23, 0) && !kzg_cells_shape_ok(0, 0), "shape range");
    {   // the practical shape at its largest batch, and the largest counts: sizes without overflow
        const KzgCellsSizes s = kzg_cells_sizes(13, 6, KZG_CELLS_CHUNK_LOG, 8192, 64);
        CHECK(s.max_used == 128 && s.max_chunks == 128 + 512 && s.max_cchunks == 64 + 512 && s.total < ((size_t)1 << 23), "n = 2^13, l = 64");
        const KzgCellsSizes big = kzg_cells_sizes(23, 22, KZG_CELLS_MAX_CHUNK_LOG, KZG_CELLS_MAX_COUNT, KZG_CELLS_MAX_COUNT);
        CHECK(big.max_chunks == 2 + ((uint64_t)1 << 14) && big.max_cchunks == KZG_CELLS_MAX_COUNT && big.total > ((size_t)1 << 36), "largest counts");
    }
    printf("kzg cells plan: %u pipelines, %d failures\n", pipelines, fails);
    return fails ? 1 : 0;
}
