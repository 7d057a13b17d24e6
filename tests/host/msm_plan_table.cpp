// plan_msm (csrc/msm_plan.hpp) against a table of plans recorded from the MSM driver before the plan became its own function
// (tests/golden/msm_plans.txt), plus the invariants every plan keeps.  g++ only: tests/test_msm_plan_cpu.py.
//   msm_plan_table <table>   one line per case: "<inputs> -> <expected plan>"; prints the cases that differ
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>

#include "msm_plan.hpp"
using namespace zkp;

// slice offsets of bases expanded for window_bits w (zkp_g1_bases_precompute): equal slices of w bits when they tile 256
// exactly, otherwise floor / ceil(256 / planes) bits
static void expand(uint32_t w, uint32_t* planes, uint32_t* cmax, uint16_t* off) {
    *planes = 256 / w + (256 % w ? 1 : 0);
    *cmax = w;
    if (*planes * w == 256) {
        for (uint32_t s = 0; s <= *planes; s++) off[s] = (uint16_t)(s * w);
        return;
    }
    const uint32_t base = 256 / *planes, rem = 256 % *planes;
    *cmax = base + (rem ? 1 : 0);
    for (uint32_t s = 0; s < *planes; s++) off[s + 1] = (uint16_t)(off[s] + base + (s < rem ? 1 : 0));
}

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

// what msm_partial_batch relies on, whatever the knobs
static const char* broken(const MsmPlan& p, const uint16_t* pre_off, uint64_t n, uint64_t count, bool feed) {
    const MsmGeom& g = p.g;
    const size_t W = g.nwin, nb = g.nb;
    uint64_t sum = 0, longest = 0, cap = g.shared ? (p.nwin1 <= 12 ? 1ull << 24 : 1ull << 23) : n;
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
    if (g.nwin != (g.shared ? count : count * p.nwin1) || g.n != (g.shared ? p.nwin1 * p.range : n)) return "windows / entries";
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

int main(int argc, char** argv) {
    std::ifstream in(argc > 1 ? argv[1] : "tests/golden/msm_plans.txt");
    int cases = 0, bad = 0;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        const size_t arrow = line.find(" -> ");
        unsigned long long n = 0, bn = 0, count = 0;
        unsigned w = 0;
        int feed = 0;
        char env[512] = {0};
        if (arrow == std::string::npos ||
            sscanf(line.c_str(), "n=%llu bn=%llu count=%llu w=%u feed=%d env=%511s", &n, &bn, &count, &w, &feed, env) != 6) {
            printf("unreadable line: %s\n", line.c_str());
            return 2;
        }
        for (int k = 0; k < KNOB_MSM_PLAN_END; k++) unsetenv(kKnobs[k].name);  // the knobs plan_msm and msm_feed_ranges read (knobs.hpp)
        if (strcmp(env, "-") != 0) {
            std::stringstream ss(env);
            for (std::string kv; std::getline(ss, kv, ';');) setenv(kv.substr(0, kv.find('=')).c_str(), kv.substr(kv.find('=') + 1).c_str(), 1);
        }
        uint16_t off[36] = {0};
        MsmBases b{bn, 0, 0, off};
        if (w) expand(w, &b.pre_planes, &b.pre_c, off);
        MsmFeedRanges fr;
        if (feed) fr = msm_feed_ranges(n);
        MsmPlan p;
        const int rc = plan_msm(b, count, n, feed ? &fr : nullptr, &p);
        const std::string got = rc ? "rc=" + std::to_string(rc) + " msg=" + p.error : p.lens.empty() ? "rc=0 empty" : show(p);
        const std::string want = line.substr(arrow + 4);
        const char* why = rc || p.lens.empty() ? nullptr : broken(p, off, n, count, feed != 0);
        cases++;
        if (got != want || why) {
            bad++;
            printf("%s\n  got  %s\n  want %s\n  %s\n", line.substr(0, arrow).c_str(), got.c_str(), want.c_str(), why ? why : "");
        }
    }
    printf("msm plans: %d cases, %d failures\n", cases, bad);
    return bad || cases == 0 ? 1 : 0;
}
