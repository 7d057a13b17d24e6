// The MSM plan (csrc/msm_plan.hpp) on the host, g++ only: tests/test_msm_plan_cpu.py.
//   msm_plan_table plans <table>      plan_msm against the plans recorded from the MSM driver before the plan became its own
//                                     function (tests/golden/msm_plans.txt)
//   msm_plan_table launches <table>   range_geom, acc_launch, the fold steps, plan_reduce and the partscatter tile against the launch
//                                     shapes recorded from the driver before they moved into the plan (tests/golden/msm_launches.txt)
//   msm_plan_table replay             the bucket reduction as plan_reduce schedules it and pyr_item / pyr_result address it, over
//                                     wrap-around integers in place of points
// Both tables: one line per case, "<inputs> -> <expected>"; the cases that differ are printed, and every plan must keep the
// invariants the driver relies on (broken, launches_broken).
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "msm_plan.hpp"
using namespace zkp;

static std::string runs(const std::vector<uint64_t>& v) {  // 5,7*3 = 5,7,7,7
    std::string s;
    for (size_t i = 0, j; i < v.size(); i = j) {
        for (j = i; j < v.size() && v[j] == v[i]; j++) {}
        s += (i ? "," : "") + std::to_string(v[i]) + (j - i > 1 ? "*" + std::to_string(j - i) : "");
    }
    return s;
}

static std::string show(const MsmPlan& p) {
    const MsmGeom& g = p.g;
    const MsmSizes& b = p.bytes;
    char buf[1024];
    snprintf(buf, sizeof buf,
             "rc=0 lens=%s range=%llu nwin1=%u overlap=%d nbuf=%zu g=%u,%u,%u,%u,%llu,%llu,%llu,%llu,%u,%u,%u,%u,%u,%u,%u,%u sg=%u,%u "
             "caps=%u,%u,%zu sizes=%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu,%zu",
             runs(p.lens).c_str(), (unsigned long long)p.range, p.nwin1, (int)p.overlap, p.nbuf, g.c, g.nwin, g.nb, g.nchunk,
             (unsigned long long)g.n, (unsigned long long)g.chunk, (unsigned long long)g.ns, (unsigned long long)g.plane_stride, g.nslice,
             g.shared, g.run_limit, g.piece, g.resume, g.interleave, g.split_log, g.more, p.sg.lo_bits, p.sg.nhi, p.over_cap, p.desc_cap,
             p.over_bytes, b.digits, b.sorted, b.counts, b.entries, b.start, b.perm, b.over, b.pieces, b.buckets, b.parts, b.pyr1, b.odd0,
             b.odd1, b.result, b.host_result);
    return buf;
}

// "<ranges> fold=<steps> pyr=<levels> tail=<level0,blocks,threads | collect> poll=<0|1> ps=<tile>,<LDS bytes>"
//   range: off,len,set,resume,more,n,chunk, then its accumulate: q|l (quad / lane kernel),per_block,bucket_blocks,extra_blocks,grid,combine grid.x
//   fold step: pairs:q|l:grid.x        level: level:half:q|l:grid.x
static std::string show_launches(const MsmPlan& p) {
    auto S = [](unsigned long long v) { return std::to_string(v); };
    std::string out = "rc=0 ranges=", fold, pyr;
    for (size_t ridx = 0; ridx < p.lens.size(); ridx++) {
        const MsmRange r = range_geom(p, ridx);
        const AccLaunch a = acc_launch(p, r.g);
        out += (ridx ? ";" : "") + S(r.off) + "," + S(r.len) + "," + S(r.set) + "," + S(r.g.resume) + "," + S(r.g.more) + "," + S(r.g.n) + "," +
               S(r.g.chunk) + "," + (a.quad ? "q" : "l") + "," + S(a.per_block) + "," + S(a.bucket_blocks) + "," + S(a.extra_blocks) + "," +
               S(a.grid) + "," + S(a.combine_x);
    }
    for (uint32_t t = 0; t < p.g.split_log; t++)
        fold += (t ? "," : "") + S(p.fold[t].pairs) + ":" + (p.fold[t].lane ? "l" : "q") + ":" + S(p.fold[t].grid_x);
    for (uint32_t k = 0; k < p.red.nlevel; k++) {
        const PyrLaunch& v = p.red.level[k];
        pyr += (k ? "," : "") + S(v.level) + ":" + S(v.half) + ":" + (v.quad ? "q" : "l") + ":" + S(v.grid_x);
    }
    out += " fold=" + (fold.empty() ? "-" : fold) + " pyr=" + (pyr.empty() ? "-" : pyr);
    out += " tail=" + (p.red.tail_blocks ? S(p.red.nlevel) + "," + S(p.red.tail_blocks) + "," + S(p.red.tail_threads) : "collect");
    return out + " poll=" + S(p.poll_result) + " ps=" + S(p.ps_tile) + "," + S(p.ps_lds);
}

// what msm_partial_batch relies on, whatever the knobs
static const char* broken(const MsmPlan& p, const uint16_t* pre_off, uint64_t n, uint64_t count, bool feed) {
    const MsmGeom& g = p.g;
    const size_t W = g.nwin, nb = g.nb;
    const uint32_t sets = g.glv ? 2 : 1;
    uint64_t sum = 0, longest = 0, cap = g.shared ? (sets * p.nwin1 <= 12 ? 1ull << 24 : 1ull << 23) : n;
    if (const long long v = knob_int(KNOB_MSM_RANGE_LOG)) cap = 1ull << v;
    else if (feed) cap = std::min<uint64_t>(cap, 1ull << msm_feed_ranges(n).range_log);
    for (uint64_t l : p.lens) {
        if (l == 0 || l > cap) return "a range is empty or longer than the cap";
        sum += l;
        longest = std::max(longest, l);
    }
    if (sum != n) return "the ranges do not add up to n";
    if (longest != p.range || g.ns != p.range) return "range is not the longest range";
    if (p.overlap != (p.lens.size() > 1 && g.shared && !knob_flag(KNOB_MSM_NO_OVERLAP)) || p.nbuf != (p.overlap ? 2u : 1u)) return "overlap";
    if (g.nwin != (g.shared ? sets * count : count * p.nwin1) || g.n != (g.shared ? p.nwin1 * p.range : n)) return "windows / entries";
    for (uint32_t s = 0; s <= p.nwin1; s++)
        if (g.off[s] != (g.shared ? pre_off[s] : s * g.c)) return "slice offsets";
    if (g.nb != 1u << (g.c - 1) || p.sg.nhi << p.sg.lo_bits != g.nb || g.chunk * g.nchunk < g.n) return "bucket / sort geometry";
    if (p.lens.size() > 1 && g.split_log) return "split runs over several ranges";
    // the carving of msm_workspace(): counts = W x (nchunk x nhi) counts | W x nhi totals | W x (nhi + 1) starts | W x 256 | W x 256
    const size_t count_words = W * ((size_t)g.nchunk * p.sg.nhi + p.sg.nhi + (p.sg.nhi + 1) + 256 + 256);
    if (4 * count_words > p.bytes.counts) return "counts carving";
    // one buffer set of `over`: W x desc_cap 16-byte descriptors | W x 2 | W x over_cap | W x (over_cap + 1) words
    if (16 * W * p.desc_cap + 4 * W * (2 + (size_t)p.over_cap + p.over_cap + 1) > p.over_bytes || p.over_bytes % 256) return "over carving";
    if (p.bytes.over < p.nbuf * p.over_bytes || p.bytes.sorted < p.nbuf * 4 * W * g.n || p.bytes.start < p.nbuf * 4 * W * (nb + 2) ||
        p.bytes.perm < p.nbuf * 4 * W * nb || p.bytes.digits < 4 * W * g.n || p.bytes.entries < 8 * W * g.n)
        return "double-buffered sets";
    if (p.bytes.parts < 256 * W * nb * ((1u << g.split_log) - 1) || p.bytes.pieces < 256 * W * (size_t)p.desc_cap) return "parts / pieces";
    if (p.bytes.host_result < 256 * W * g.c + 4 * W || p.bytes.result < 4 * PYR_BAR_STRIDE * W) return "results";
    return nullptr;
}

// what the launches of the walk and of the reduction must keep, whatever the knobs; `waves`: the device argument of the plan
static bool grid_ok(uint64_t x, uint64_t y = 1, uint64_t z = 1) { return x >= 1 && x <= 0x7fffffffull && y >= 1 && y <= 65535 && z >= 1 && z <= 65535; }
static const char* launches_broken(const MsmPlan& p, uint64_t n, uint64_t count, uint32_t waves) {
    const MsmGeom& g = p.g;
    uint64_t next = 0;
    for (size_t ridx = 0; ridx < p.lens.size(); ridx++) {
        const MsmRange r = range_geom(p, ridx);
        if (r.off != next || r.len != p.lens[ridx] || r.ridx != ridx || r.set != (p.overlap ? ridx & 1 : 0)) return "ranges are not contiguous";
        next += r.len;
        if (r.g.resume != (ridx ? 1u : 0u) || r.g.more != (ridx + 1 < p.lens.size() ? 1u : 0u)) return "resume / more";
        if (r.g.ns != r.len || r.g.n > g.n || r.g.n != (g.shared ? (uint64_t)p.nwin1 * r.len : n)) return "a range's entries";
        if (r.g.chunk * r.g.nchunk < r.g.n || r.g.chunk > g.chunk) return "a range's chunks";
        const SortLaunch sl = sort_launch(p.sg, r.g);
        if (!grid_ok(sl.digits_x, count) || (uint64_t)sl.digits_x * MSM_THREADS < r.g.ns || !grid_ok(r.g.nchunk, g.nwin) || !grid_ok(sl.prefix_x, g.nwin) ||
            sl.prefix_x * 64 < p.sg.nhi || !grid_ok(p.sg.nhi, g.nwin) || !grid_ok(sl.rank_x, g.nwin) || (uint64_t)sl.rank_x * 1024 < g.nb)
            return "sort grids";
        const AccLaunch a = acc_launch(p, r.g);
        if (a.quad && p.lens.size() != 1) return "quad accumulate over several ranges";
        if (a.quad != (acc_quad(r.g) ? 1u : 0u) || a.per_block != (a.quad ? ACC_THREADS / 4u : ACC_THREADS)) return "accumulate variant";
        const uint64_t units = (uint64_t)g.nb << g.split_log;  // bucket lanes (quads)
        if ((uint64_t)a.bucket_blocks * a.per_block < units || (uint64_t)(a.bucket_blocks - 1) * a.per_block >= units) return "accumulate blocks do not cover the buckets";
        if (a.extra_blocks < 1 || a.extra_blocks > 64 || (uint64_t)a.grid != ((uint64_t)a.bucket_blocks + a.extra_blocks) * g.nwin || !grid_ok(a.grid))
            return "accumulate grid";
        if (a.combine_x < 1 || a.combine_x > 64 || !grid_ok(a.combine_x, g.nwin)) return "combine grid";
    }
    if (next != n) return "the ranges do not add up to n";
    if (p.poll_result != (range_geom(p, p.lens.size() - 1).g.n <= (1ull << 24))) return "poll_result";
    // the split sizing went by the kernel the accumulate launch then takes
    if (p.lens.size() == 1 && !getenv("ZKP_MSM_SPLIT_LOG")) {
        const uint64_t want = acc_launch(p, range_geom(p, 0).g).quad ? SPLIT_FILL_QUADS : SPLIT_FILL_LANES;
        uint32_t s = 0;
        while (s < MSM_MAX_SPLIT_LOG && (((uint64_t)g.nb * g.nwin) << s) < want) s++;
        if (s != g.split_log) return "split sizing and accumulate launch disagree";
    }
    uint64_t pairs = 0;
    const uint64_t cap = (uint64_t)g.nwin * g.nb;
    for (uint32_t t = 0; t < g.split_log; t++) {
        const FoldStep& f = p.fold[t];
        pairs += f.pairs;
        if (f.pairs != 1u << (g.split_log - 1 - t) || (uint64_t)f.grid_x * (f.lane ? MSM_THREADS : MSM_THREADS / 4) < cap || !grid_ok(f.grid_x, f.pairs)) return "fold step";
    }
    if (g.split_log > MSM_MAX_SPLIT_LOG || pairs != (1u << g.split_log) - 1 || p.bytes.parts != 256 * cap * pairs) return "fold pairs against bytes.parts";
    // every level 0 .. c - 2 exactly once, in order: own launches, then the last-levels launch
    const ReducePlan& red = p.red;
    for (uint32_t k = 0; k < red.nlevel; k++) {
        const PyrLaunch& v = red.level[k];
        if (v.level != k || v.half != g.nb >> (k + 1) || (uint64_t)v.grid_x * (v.quad ? MSM_THREADS / 4 : MSM_THREADS) < v.half || !grid_ok(v.grid_x, k + 1, g.nwin))
            return "a reduction level";
    }
    if (red.tail_blocks) {
        if (red.nlevel + 1 >= g.c) return "a last-levels launch without a level";
        if (red.tail_threads < 64 || red.tail_threads > 512 || red.tail_threads % 64 || !grid_ok(red.tail_blocks, g.nwin)) return "last-levels launch shape";
        if ((uint64_t)red.tail_blocks * g.nwin * (red.tail_threads / 64) > waves) return "the last-levels launch is not co-resident";
    } else if (red.nlevel != g.c - 1 || g.c > 64 || !grid_ok(g.nwin)) {
        return "collect only, but the levels do not reach c - 2";
    }
    if (p.ps_tile != partscatter_tile(p.sg.nhi) || p.ps_lds != partscatter_lds_bytes(p.sg.nhi, p.ps_tile)) return "partscatter tile";
    return nullptr;
}

struct Case {
    unsigned long long n = 0, bn = 0, count = 0;
    unsigned w = 0, waves = 2048;
    int glv = 0, feed = 0;
    char env[512] = {0};
    MsmSlices sl{};
    MsmPlan p;
    int rc = 0;
};
// the plan of a case, under its knobs
static void plan_case(Case& c) {
    for (int k = 0; k < KNOB_MSM_PLAN_END; k++) unsetenv(kKnobs[k].name);  // the knobs the plan reads (knobs.hpp)
    if (strcmp(c.env, "-") != 0) {
        std::stringstream ss(c.env);
        for (std::string kv; std::getline(ss, kv, ';');) setenv(kv.substr(0, kv.find('=')).c_str(), kv.substr(kv.find('=') + 1).c_str(), 1);
    }
    // slice offsets of bases expanded for window_bits w (zkp_g1_bases_precompute*): the rule of the library itself
    MsmBases b{c.bn, 0, 0, c.sl.off, 0};
    if (c.w) {
        c.sl = msm_slice_offsets(c.glv ? 129 : 256, c.w, 1);
        b.pre_c = c.sl.widest;
        b.pre_planes = c.sl.planes;
        b.glv = c.glv ? 1 : 0;
    }
    MsmFeedRanges fr;
    if (c.feed) fr = msm_feed_ranges(c.n);
    c.rc = plan_msm(b, c.count, c.n, c.feed ? &fr : nullptr, c.waves, &c.p);
}

static int table(const char* path, bool launches) {
    std::ifstream in(path);
    int cases = 0, bad = 0;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        const size_t arrow = line.find(" -> ");
        Case c;
        const bool read = launches ? sscanf(line.c_str(), "n=%llu bn=%llu count=%llu w=%u glv=%d feed=%d waves=%u env=%511s", &c.n, &c.bn, &c.count, &c.w,
                                            &c.glv, &c.feed, &c.waves, c.env) == 8
                                   : sscanf(line.c_str(), "n=%llu bn=%llu count=%llu w=%u feed=%d env=%511s", &c.n, &c.bn, &c.count, &c.w, &c.feed, c.env) == 6;
        if (arrow == std::string::npos || !read) {
            printf("unreadable line: %s\n", line.c_str());
            return 2;
        }
        plan_case(c);
        const MsmPlan& p = c.p;
        const std::string got = c.rc ? "rc=" + std::to_string(c.rc) + " msg=" + p.error : p.lens.empty() ? "rc=0 empty" : launches ? show_launches(p) : show(p);
        const std::string want = line.substr(arrow + 4);
        const char* why = c.rc || p.lens.empty() ? nullptr : broken(p, c.sl.off, c.n, c.count, c.feed != 0);
        if (!why && !c.rc && !p.lens.empty()) why = launches_broken(p, c.n, c.count, c.waves);
        cases++;
        if (got != want || why) {
            bad++;
            printf("%s\n  got  %s\n  want %s\n  %s\n", line.substr(0, arrow).c_str(), got.c_str(), want.c_str(), why ? why : "");
        }
    }
    printf("msm %s: %d cases, %d failures\n", launches ? "launches" : "plans", cases, bad);
    return bad || cases == 0 ? 1 : 0;
}

// The partscatter staging next to 12 bytes per partition must fit the 160 KiB of LDS for every partition count the sort takes
static int partscatter_fits() {
    for (uint32_t nhi = 1; nhi <= SORT_MAX_PART; nhi++)
        if (partscatter_lds_bytes(nhi, partscatter_tile(nhi)) > 160 * 1024) {
            printf("partscatter: %u partitions need %zu bytes of LDS\n", nhi, partscatter_lds_bytes(nhi, partscatter_tile(nhi)));
            return 1;
        }
    return 0;
}

// The bucket reduction of nwin sets of 2^(c-1) buckets over uint64_t (wrap-around) in place of points: level 0 seeded at
// pyr_pos(b - 1, nb), every own-launch level with its grid, the last-levels launch with its item loop, the gathering by pyr_result;
// then V = R_0 + sum_l 2^l R_{1+l} against sum_b b B_b.  Within a level no item may touch an entry that another item writes, and
// no item may read an entry that nothing has written.
struct Replay {
    uint32_t c, nb, nwin;
    uint64_t cap;
    std::vector<uint64_t> buf[4];   // pyr0, pyr1, odd0, odd1
    std::vector<char> written[4];
    struct Item { int src, dst; PyrItem it; };
    std::vector<Item> items;
    ReducePlan red{};
    const char* error = nullptr;

    void item(uint32_t l, uint32_t kind, uint32_t s, uint32_t w) {
        const uint32_t half = nb >> (l + 1);
        const PyrItem it = pyr_item(nb, l, half, kind, s, (uint64_t)w * nb);
        const int pyr_in = l & 1, pyr_out = (l + 1) & 1, odd_in = 2 + (l & 1), odd_out = 2 + ((l + 1) & 1);  // as the kernels pick them
        items.push_back({kind == 0 ? pyr_in : it.src_is_pyr_out ? pyr_out : odd_in, kind ? odd_out : pyr_out, it});
    }
    void run_level() {  // the items of one level (between two launches, or two barriers of the last-levels launch) run in any order
        std::vector<int> writer[4];
        for (auto& v : writer) v.assign(cap, -1);
        for (size_t k = 0; k < items.size(); k++) {
            const Item& i = items[k];
            if (i.it.a >= cap || i.it.b >= cap || i.it.d >= cap) { error = "an item outside the arrays"; return; }
            if (writer[i.dst][i.it.d] >= 0) { error = "two items write one entry"; return; }
            writer[i.dst][i.it.d] = (int)k;
        }
        std::vector<uint64_t> sums(items.size());
        for (size_t k = 0; k < items.size(); k++) {
            const Item& i = items[k];
            for (uint64_t e : {i.it.a, i.it.b}) {
                if (writer[i.src][e] >= 0) { error = "an item reads an entry that an item of the same level writes"; return; }
                if (!written[i.src][e]) { error = "an item reads an entry nothing has written"; return; }
            }
            sums[k] = buf[i.src][i.it.a] + buf[i.src][i.it.b];
        }
        for (size_t k = 0; k < items.size(); k++) {
            buf[items[k].dst][items[k].it.d] = sums[k];
            written[items[k].dst][items[k].it.d] = 1;
        }
        items.clear();
    }
    const char* run(uint32_t c_, uint32_t nwin_, uint32_t waves) {
        c = c_, nb = 1u << (c - 1), nwin = nwin_, cap = (uint64_t)nwin * nb;
        if (plan_reduce(c, nwin, waves, &red, &error)) return error;
        uint64_t rng = 0x9E3779B97F4A7C15ull * (c * 131 + nwin * 7 + waves);
        auto next = [&rng] { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return rng; };
        for (int k = 0; k < 4; k++) {
            buf[k].resize(cap);
            for (auto& v : buf[k]) v = next();  // (what an earlier MSM left behind)
            written[k].assign(cap, 0);
        }
        std::vector<uint64_t> want(nwin, 0);
        for (uint32_t w = 0; w < nwin; w++)
            for (uint32_t b = 1; b <= nb; b++) {
                const uint64_t e = (uint64_t)w * nb + pyr_pos(b - 1, nb), v = next();
                buf[0][e] = v;
                written[0][e] = 1;
                want[w] += b * v;
            }
        uint32_t levels = 0;
        for (uint32_t k = 0; k < red.nlevel; k++, levels++) {  // msm_pyramid_kernel / msm_pyramid_quad_kernel over (grid_x, level + 1, nwin)
            const PyrLaunch& v = red.level[k];
            if (v.level != levels) return "own-launch levels out of order";
            const uint32_t per = v.quad ? MSM_THREADS / 4 : MSM_THREADS;
            for (uint32_t w = 0; w < nwin; w++)
                for (uint32_t kind = 0; kind <= v.level; kind++)
                    for (uint32_t s = 0; s < v.grid_x * per; s++)
                        if (s < v.half) item(v.level, kind, s, w);
            run_level();
            if (error) return error;
        }
        if (red.tail_blocks) {  // msm_pyramid_tail_kernel over (tail_blocks, nwin) x tail_threads: a quad per add
            const uint32_t nquad = red.tail_blocks * (red.tail_threads >> 2);
            for (uint32_t l = red.nlevel; l + 1 < c; l++, levels++) {
                const uint32_t half = nb >> (l + 1);
                for (uint32_t w = 0; w < nwin; w++)
                    for (uint32_t quad = 0; quad < nquad; quad++)
                        for (uint32_t it = quad; it < (l + 1) * half; it += nquad) item(l, it / half, it % half, w);
                run_level();
                if (error) return error;
            }
        }
        if (levels != c - 1) return "the levels 0 .. c - 2 did not each run once";
        const int fin = (c - 1) & 1;  // what the driver hands msm_collect_kernel, and what the last-levels launch derives from c
        for (uint32_t w = 0; w < nwin; w++) {
            uint64_t v = 0;
            for (uint32_t e = 0; e < c; e++) {
                const uint64_t wbase = (uint64_t)w * nb;
                const uint64_t* src = pyr_result(buf[fin].data(), buf[fin ^ 1].data(), buf[2 + fin].data(), wbase, nb, c, e);
                if (!*pyr_result(written[fin].data(), written[fin ^ 1].data(), written[2 + fin].data(), wbase, nb, c, e))
                    return "the gathering reads an entry nothing has written";
                v += e == 0 ? *src : *src << (e - 1);
            }
            if (v != want[w]) return "the reduction does not give sum_b b B_b";
        }
        return nullptr;
    }
};

static int replay() {
    int cases = 0, bad = 0, tails = 0, collects = 0;
    for (const char* half : {(const char*)nullptr, "1", "4"}) {  // (default: the last-levels launch takes over at 64 pairs)
        for (int k = 0; k < KNOB_MSM_PLAN_END; k++) unsetenv(kKnobs[k].name);
        if (half) setenv("ZKP_PYR_TAIL_HALF", half, 1);
        for (uint32_t c = 2; c <= 9; c++)
            for (uint32_t nwin : {1u, 3u})
                for (uint32_t waves : {4u, 2048u}) {
                    Replay r;
                    const char* why = r.run(c, nwin, waves);
                    (r.red.tail_blocks ? tails : collects)++;
                    cases++;
                    if (why) bad++, printf("replay c=%u nwin=%u waves=%u tail_half=%s: %s\n", c, nwin, waves, half ? half : "default", why);
                }
    }
    printf("msm replay: %d cases (%d with a last-levels launch, %d collect only), %d failures\n", cases, tails, collects, bad);
    return bad || !tails || !collects ? 1 : 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "plans" && argc > 2) return table(argv[2], false);
    if (mode == "launches" && argc > 2) return table(argv[2], true) | partscatter_fits();
    if (mode == "replay") return replay();
    printf("usage: msm_plan_table plans|launches <table> | replay\n");
    return 2;
}
