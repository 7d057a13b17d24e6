// csrc/kzg_points_plan.hpp on its own, g++ only (tests/test_kzg_points_plan_cpu.py builds it with -fsanitize=address,undefined).
// For N in {1, 2, 15, 16, 17, 255, 256, 257, 1025}, the groupings identity (no index), one commitment, one opening per commitment
// plus a commitment nothing names, and a skewed split (most openings on one commitment, some commitments empty), and chunk logs 0, 1
// and the default, it builds the table the driver builds, in buffers of exactly the sizes the plan reports (the sanitizer sees every
// index), and checks that
//   - the sort holds every opening exactly once, segments are in commitment order and keep the batch order inside a commitment;
//   - no chunk is empty, exceeds 2^chunk_log openings or crosses a segment; the chunk count respects the bound the sizes are made from;
//   - the table of the call fits the verifier's, and the pieces of the workspace are disjoint, aligned and inside its total;
//   - the whole field pipeline over F_65537, walked launch by launch and lane by lane with exactly these tables, step descriptions and
//     index functions -- scalars with the tree of every workgroup, the finishing workgroup, chunk sums, commitment sums -- gives the
//     plain sums; a second, smaller call in the same buffers sees nothing of the first;
//   - the bisection halves a slice into pieces that reach one opening within ceil(log2 N) steps.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kzg_points_plan.hpp"
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

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return rng_state >> 33;
}

// tree[1] <- the sum of the leaves, as points_tree_sum walks it: level by level, lane t < s of a level writes node s + t
static void tree_sum(std::vector<uint64_t>& tree) {
    for (uint32_t s = KZG_CELLS_THREADS / 2; s >= 1; s >>= 1)
        for (uint32_t t = 0; t < s; t++) tree.at(s + t) = (tree.at(2 * (s + t)) + tree.at(2 * (s + t) + 1)) % P;
}

struct Work {  // a verifier's buffers, of exactly the sizes the plan reports
    KzgPointsSizes sz;
    std::vector<uint32_t> scratch, table;
    std::vector<uint64_t> cpartial, ypartial;
};

// one call: commit == nullptr is the identity index
static void run(Work& w, unsigned chunk_log, uint64_t max_openings, uint64_t max_commits, const std::vector<uint32_t>* commit, uint64_t N, uint64_t M) {
    const uint64_t per = (uint64_t)1 << chunk_log;
    CHECK(N <= max_openings && M <= max_commits, "the case fits the verifier");
    std::fill(w.table.begin(), w.table.end(), 0xDEADBEEFu);
    const KzgPointsTables t = kzg_points_tables(chunk_log, commit ? commit->data() : nullptr, N, M, commit ? w.scratch.data() : nullptr,
                                                commit ? w.table.data() : nullptr);
    CHECK(t.openings == N && t.commits == M && t.identity == !commit, "the call's counts");
    CHECK(t.words <= w.sz.table_words && t.cchunks <= w.sz.max_cchunks, "N %llu M %llu: a table of %llu words in %llu", (ull)N, (ull)M, (ull)t.words,
          (ull)w.sz.table_words);
    if (commit) {
        CHECK(t.cchunks <= kzg_cells_max_chunks(N, M, chunk_log), "chunk bound of the call");
        const size_t piece[4] = {t.by_commit, t.cchunk_start, t.cseg_chunk, t.words};
        const size_t words[3] = {N, t.cchunks + 1, M + 1};
        for (int i = 0; i < 3; i++) CHECK(piece[i] + words[i] == piece[i + 1], "piece %d of the table", i);
        const uint32_t* order = &w.table[t.by_commit];
        const uint32_t* cstart = &w.table[t.cchunk_start];
        const uint32_t* seg = &w.table[t.cseg_chunk];
        std::vector<int> seen(N, 0);
        for (uint64_t i = 0; i < N; i++) {
            CHECK(order[i] < N, "opening id");
            if (order[i] < N) seen[order[i]]++;
            if (i)
                CHECK((*commit)[order[i - 1]] < (*commit)[order[i]] || ((*commit)[order[i - 1]] == (*commit)[order[i]] && order[i - 1] < order[i]),
                      "order at %llu", (ull)i);
        }
        for (uint64_t i = 0; i < N; i++) CHECK(seen[i] == 1, "opening %llu appears %d times", (ull)i, seen[i]);
        CHECK(cstart[0] == 0 && cstart[t.cchunks] == N && seg[0] == 0 && seg[M] == t.cchunks, "ends");
        for (uint64_t m = 0; m < M; m++) {
            CHECK(seg[m] <= seg[m + 1], "segment %llu", (ull)m);
            uint64_t members = 0, want = 0;
            for (uint32_t q = seg[m]; q < seg[m + 1]; q++) {
                const uint64_t len = cstart[q + 1] - cstart[q];
                CHECK(len >= 1 && len <= per, "chunk %u of %llu openings", q, (ull)len);
                CHECK(q + 1 == seg[m + 1] || len == per, "only the last chunk of a segment is short");
                for (uint32_t at = cstart[q]; at < cstart[q + 1]; at++, members++) CHECK((*commit)[order[at]] == m, "chunk %u crosses a segment", q);
            }
            for (uint64_t i = 0; i < N; i++) want += (*commit)[i] == m;
            CHECK(members == want, "commitment %llu has %llu of %llu openings", (ull)m, (ull)members, (ull)want);
        }
    } else {
        CHECK(t.words == 0 && t.cchunks == 0 && M == N, "the identity index needs no table");
    }

    // the field pipeline, launch by launch and lane by lane
    std::vector<uint64_t> weights(N), z(N), y(N), cw(M, 0xDEAD), rz(N, 0xDEAD), r(N, 0xDEAD);
    for (uint64_t i = 0; i < N; i++) weights[i] = rnd() % P, z[i] = rnd() % P, y[i] = rnd() % P;
    if (N > 2) weights[1] = 0, z[2] = 0, y[0] = 0, weights[N - 1] = P - 1;
    uint64_t neg = 0xDEAD;
    unsigned launches = 0;
    for (unsigned i = 0; i < KZG_POINTS_STEPS; i++) {
        const KzgPointsStep s = kzg_points_step(t, i);
        CHECK(s.blocks * KZG_CELLS_THREADS >= s.lanes || s.kind == KZG_POINTS_FINISH, "step %u: workgroups for every lane", i);
        if (!s.blocks) continue;
        launches++;
        switch (s.kind) {
        case KZG_POINTS_SCALARS:
            CHECK(s.lanes == N && s.blocks == kzg_points_blocks(N) && s.blocks <= w.sz.max_blocks, "scalar lanes");
            for (uint64_t b = 0; b < s.blocks; b++) {
                std::vector<uint64_t> tree(2 * KZG_CELLS_THREADS, 0xDEAD);
                for (uint32_t lane = 0; lane < KZG_CELLS_THREADS; lane++) {
                    const uint64_t o = b * KZG_CELLS_THREADS + lane;
                    uint64_t leaf = 0;
                    if (o < t.openings) {
                        r.at(o) = weights.at(o);
                        rz.at(o) = weights.at(o) * z.at(o) % P;
                        if (t.identity) cw.at(o) = weights.at(o);
                        leaf = weights.at(o) * y.at(o) % P;
                    }
                    tree.at(kzg_points_leaf(lane)) = leaf;
                }
                tree_sum(tree);
                w.ypartial.at(b) = tree[1];
            }
            break;
        case KZG_POINTS_FINISH: {
            CHECK(s.blocks == 1 && s.lanes == KZG_CELLS_THREADS, "one finishing workgroup");
            std::vector<uint64_t> tree(2 * KZG_CELLS_THREADS, 0xDEAD);
            const uint64_t blocks = kzg_points_blocks(t.openings);
            for (uint32_t lane = 0; lane < KZG_CELLS_THREADS; lane++) {
                uint64_t acc = 0;
                for (uint64_t b = lane; b < blocks; b += KZG_CELLS_THREADS) acc = (acc + w.ypartial.at(b)) % P;
                tree.at(kzg_points_leaf(lane)) = acc;
            }
            tree_sum(tree);
            neg = (P - tree[1]) % P;
            break;
        }
        case KZG_POINTS_CHUNKS:
            CHECK(s.lanes == t.cchunks && !t.identity, "chunk lanes");
            for (uint64_t q = 0; q < s.lanes; q++) {
                uint64_t acc = 0;
                for (uint32_t at = w.table.at(t.cchunk_start + q); at < w.table.at(t.cchunk_start + q + 1); at++)
                    acc = (acc + weights.at(w.table.at(t.by_commit + at))) % P;
                w.cpartial.at(q) = acc;
            }
            break;
        case KZG_POINTS_COMMITS:
            CHECK(s.lanes == M && !t.identity, "commit lanes");
            for (uint64_t m = 0; m < s.lanes; m++) {
                uint64_t acc = 0;
                for (uint32_t q = w.table.at(t.cseg_chunk + m); q < w.table.at(t.cseg_chunk + m + 1); q++) acc = (acc + w.cpartial.at(q)) % P;
                cw.at(m) = acc;
            }
            break;
        }
    }
    CHECK(launches == (N ? (t.identity ? 2u : 4u) : (t.identity || !M ? 1u : 2u)), "N %llu M %llu: %u launches", (ull)N, (ull)M, launches);
    // the definition
    std::vector<uint64_t> want_cw(M, 0);
    uint64_t sum = 0;
    for (uint64_t i = 0; i < N; i++) {
        const uint64_t m = commit ? (*commit)[i] : i;
        want_cw[m] = (want_cw[m] + weights[i]) % P;
        sum = (sum + weights[i] * y[i]) % P;
        CHECK(r[i] == weights[i] && rz[i] == weights[i] * z[i] % P, "scalars of opening %llu", (ull)i);
    }
    CHECK(cw == want_cw, "chunk %u N %llu M %llu: commitment weights", chunk_log, (ull)N, (ull)M);
    CHECK((neg + sum) % P == 0 && neg < P, "chunk %u N %llu: -sum r y", chunk_log, (ull)N);
}

int main() {
    unsigned pipelines = 0;
    const uint64_t sizes[9] = {1, 2, 15, 16, 17, 255, 256, 257, 1025};
    for (unsigned chunk_log : {0u, 1u, KZG_CELLS_CHUNK_LOG}) {
        const uint64_t max_openings = 1025, max_commits = 1026;
        Work w;
        w.sz = kzg_points_sizes(chunk_log, max_openings, max_commits);
        const KzgPointsSizes& sz = w.sz;
        {   // the pieces of the workspace, in order, disjoint, aligned, inside total
            const size_t piece[9] = {sz.cpartial, sz.ypartial, sz.sc_right, sz.sc_left, sz.y, sz.gen, sz.report, sz.table, sz.total};
            const size_t bytes[8] = {32 * sz.max_cchunks, 32 * sz.max_blocks, 32 * (max_commits + max_openings + 1), 32 * (max_commits + max_openings + 1),
                                     32 * max_openings, 96, 64, 4 * sz.table_words};
            for (int i = 0; i < 8; i++) CHECK(piece[i] + bytes[i] <= piece[i + 1] && piece[i] % 32 == 0, "piece %d of the workspace", i);
            CHECK(sz.stage_total == 4 * sz.table_words && sz.scratch_words >= max_commits + 1 && sz.max_blocks == 5, "staging, scratch, workgroups");
        }
        w.scratch.resize(sz.scratch_words);
        w.table.resize(sz.table_words);
        w.cpartial.assign(sz.max_cchunks, 0xDEAD);
        w.ypartial.assign(sz.max_blocks, 0xDEAD);
        for (int pass = 0; pass < 2; pass++)  // descending the second time: a smaller call after a larger one in the same buffers
            for (int k = 0; k < 9; k++) {
                const uint64_t N = sizes[pass ? 8 - k : k];
                std::vector<uint32_t> one(N, 0), each(N), skew(N);
                for (uint64_t i = 0; i < N; i++) {
                    each[i] = (uint32_t)((i * 7 + 3) % N);          // one opening per commitment (N and 7 coprime here), commitment N unused
                    skew[i] = rnd() % 8 ? 2u : (uint32_t)(rnd() % 2 ? 0 : 5);  // commitments 1, 3 and 4 of 6 stay empty
                }
                run(w, chunk_log, max_openings, max_commits, nullptr, N, N);
                run(w, chunk_log, max_openings, max_commits, &one, N, 1);
                run(w, chunk_log, max_openings, max_commits, &each, N, N + 1);
                run(w, chunk_log, max_openings, max_commits, &skew, N, 6);
                pipelines += 4;
            }
        const std::vector<uint32_t> none(1, 0);  // (an index array of no opening: not null, which would mean the identity)
        run(w, chunk_log, max_openings, max_commits, &none, 0, 3);  // no opening at all: zeros
        run(w, chunk_log, max_openings, max_commits, nullptr, 0, 0);
        pipelines += 2;
    }
    for (uint64_t N : {1ull, 2ull, 3ull, 37ull, 256ull, 257ull, 4096ull, 1ull << 30}) {  // the bisection, down the larger piece each time
        uint64_t lo = 0, hi = N;
        unsigned steps = 0;
        while (hi - lo > 1) {
            const uint64_t mid = kzg_points_bisect_mid(lo, hi);
            CHECK(lo < mid && mid < hi && mid - lo >= hi - mid, "a slice is cut into two pieces, the lower no smaller");
            hi = mid;
            steps++;
        }
        CHECK(steps == kzg_points_bisect_checks(N), "N %llu: %u steps", (ull)N, steps);
    }
    CHECK(kzg_points_bisect_checks(37) == 6 && kzg_points_bisect_checks(1) == 0 && kzg_points_bisect_checks(4096) == 12, "ceil(log2 N)");
    {   // the largest counts: sizes without overflow
        const KzgPointsSizes big = kzg_points_sizes(0, KZG_CELLS_MAX_COUNT, KZG_CELLS_MAX_COUNT);
        CHECK(big.max_cchunks == KZG_CELLS_MAX_COUNT && big.max_blocks == KZG_CELLS_MAX_COUNT / KZG_CELLS_THREADS && big.total > ((size_t)1 << 37),
              "largest counts");
    }
    printf("kzg points plan: %u pipelines, %d failures\n", pipelines, fails);
    return fails ? 1 : 0;
}
