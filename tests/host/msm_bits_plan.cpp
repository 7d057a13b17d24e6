// The plan of an MSM over bounded scalars (csrc/msm_plan.hpp: msm_bound_slices, plan_msm's scalar_bits) on the host, g++ only:
// tests/test_msm_bits_plan_cpu.py.
//   rule    for every offset table the library makes and every bound, t = msm_bound_slices is the brute-force minimum: at 2^bits - 1
//           (and at the values that stress a carry) the first t digits say the value exactly and nothing leaves slice t - 1; with
//           t - 1 slices 2^bits - 1 carries out
//   plans   plan_msm(bases, ..., bits) equals plan_msm over bases that hold only the first t planes, in every field; the default and
//           bits >= 255 equal the plan of whole scalars; split planes run as one plain bucket set up to 127 bits
#include <cstdio>
#include <cstring>
#include <string>

#include "msm_plan.hpp"
using namespace zkp;

// ---- the recoding of msm_recode (msm.hpp) over the first m slices of a table, on a 256-bit value in 32-bit words
struct Recoded {
    int64_t d[36];
    uint32_t carry;
};
static Recoded recode(const uint32_t (&k)[8], const uint16_t* off, uint32_t m) {
    Recoded r{};
    uint32_t carry = 0;
    for (uint32_t w = 0; w < m; w++) {
        const uint32_t lo = off[w], width = (uint32_t)off[w + 1] - lo, limb = lo >> 5, sh = lo & 31;
        uint64_t v = limb < 8 ? k[limb] : 0;
        if (limb + 1 < 8) v |= (uint64_t)k[limb + 1] << 32;
        const uint32_t u = ((uint32_t)(v >> sh) & ((1u << width) - 1)) + carry;
        if (u > (1u << (width - 1))) {
            r.d[w] = (int64_t)u - ((int64_t)1 << width);
            carry = 1;
        } else {
            r.d[w] = u;
            carry = 0;
        }
    }
    r.carry = carry;
    return r;
}
// sum_s d[s] 2^off[s] == k, in two's complement over 320 bits
static bool exact(const uint32_t (&k)[8], const Recoded& r, const uint16_t* off, uint32_t m) {
    uint32_t acc[10] = {0};
    for (uint32_t s = 0; s < m; s++) {
        const bool neg = r.d[s] < 0;
        const uint64_t mag = (uint64_t)(neg ? -r.d[s] : r.d[s]);
        uint32_t term[10] = {0};
        const uint32_t limb = off[s] >> 5, sh = off[s] & 31;
        // mag < 2^25 shifted by sh < 32: three words at most
        const unsigned __int128 wide = (unsigned __int128)mag << sh;
        for (uint32_t q = 0; q < 3 && limb + q < 10; q++) term[limb + q] = (uint32_t)(wide >> (32 * q));
        uint64_t c = neg ? 1 : 0;  // acc += term, or acc += ~term + 1
        for (int q = 0; q < 10; q++) {
            c += (uint64_t)acc[q] + (neg ? ~term[q] : term[q]);
            acc[q] = (uint32_t)c;
            c >>= 32;
        }
    }
    for (int q = 0; q < 10; q++)
        if (acc[q] != (q < 8 ? k[q] : 0u)) return false;
    return true;
}
static void low_bits(uint32_t (&k)[8], const uint32_t (&src)[8], unsigned bits) {  // src mod 2^bits
    for (unsigned q = 0; q < 8; q++) k[q] = bits >= 32 * q + 32 ? src[q] : bits > 32 * q ? src[q] & ((1u << (bits - 32 * q)) - 1) : 0u;
}

static int bad = 0;
#define EXPECT(cond, ...)                        \
    do {                                         \
        if (!(cond)) {                           \
            if (bad++ < 40) { printf(__VA_ARGS__); printf("  [%s]\n", #cond); } \
        }                                        \
    } while (0)

struct Table {
    std::string name;
    uint16_t off[36];
    uint32_t nslice, cover;
};
static std::vector<Table> tables() {
    std::vector<Table> t;
    for (uint32_t c : {8u, 16u}) {  // per-window mode: off[s] = s c
        Table x{"per-window " + std::to_string(c), {0}, 256 / c, 256};
        for (uint32_t s = 0; s <= x.nslice; s++) x.off[s] = (uint16_t)(s * c);
        t.push_back(x);
    }
    for (uint32_t cover : {256u, 129u})
        for (uint32_t w = 9; w <= 24; w++) {
            const MsmSlices sl = msm_slice_offsets(cover, w, 1);
            Table x{"expansion " + std::to_string(cover) + "/" + std::to_string(w), {0}, sl.planes, cover};
            std::memcpy(x.off, sl.off, sizeof x.off);
            t.push_back(x);
        }
    return t;
}

static int rule() {
    int cases = 0;
    uint64_t rng = 0x243F6A8885A308D3ull;
    auto next = [&rng] { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (uint32_t)(rng >> 16); };
    for (const Table& tb : tables()) {
        // a bound the table cannot hold (split planes above 127 bits) is not the rule's business: plan_msm keeps both bucket sets there
        const unsigned top = tb.cover == 129 ? MSM_BITS_GLV_ONE_SET : MSM_BITS_MAX;
        for (unsigned bits = 1; bits <= top; bits++) {
            const uint32_t t = msm_bound_slices(tb.off, tb.nslice, bits);
            cases++;
            EXPECT(t >= 1 && t <= tb.nslice, "%s bits %u: t = %u", tb.name.c_str(), bits, t);
            EXPECT(tb.off[t] >= bits + 1 || t == tb.nslice, "%s bits %u: off[t] below bits + 1", tb.name.c_str(), bits);
            EXPECT(t == 1 || tb.off[t - 1] < bits + 1, "%s bits %u: t is not the smallest index", tb.name.c_str(), bits);
            if (bits >= MSM_BITS_WHOLE) {  // r < 2^255: the whole table
                EXPECT(t == tb.nslice, "%s bits %u: whole scalars need every slice", tb.name.c_str(), bits);
                continue;
            }
            uint32_t ones[8], k[8];
            std::memset(ones, 0xFF, sizeof ones);
            // brute force at 2^bits - 1: the smallest m whose digits say it with no carry out is t
            low_bits(k, ones, bits);
            uint32_t m = 1;
            for (; m <= tb.nslice; m++) {
                const Recoded r = recode(k, tb.off, m);
                if (!r.carry && exact(k, r, tb.off, m)) break;
            }
            EXPECT(m == t, "%s bits %u: brute force %u, rule %u", tb.name.c_str(), bits, m, t);
            if (t > 1) EXPECT(recode(k, tb.off, t - 1).carry == 1, "%s bits %u: no carry out of %u slices", tb.name.c_str(), bits, t - 1);
            // other values below 2^bits: 0, 1, 2^(bits-1), every slice exactly half (the largest digit that does not carry), half + 1
            // in every slice (every slice carries), random ones
            for (int pat = 0; pat < 25; pat++) {
                uint32_t v[8] = {0};
                if (pat == 1) v[0] = 1;
                if (pat == 2) v[(bits - 1) >> 5] = 1u << ((bits - 1) & 31);
                if (pat == 3 || pat == 4)
                    for (uint32_t s = 0; s < tb.nslice; s++) {
                        const uint32_t hb = tb.off[s + 1] - 1;  // top bit of slice s
                        if (hb < 256) v[hb >> 5] |= 1u << (hb & 31);
                        if (pat == 4 && tb.off[s] < 256) v[tb.off[s] >> 5] |= 1u << (tb.off[s] & 31);
                    }
                if (pat >= 5)
                    for (auto& q : v) q = next();
                low_bits(k, v, bits);
                const Recoded r = recode(k, tb.off, t);
                EXPECT(!r.carry && exact(k, r, tb.off, t), "%s bits %u pattern %d: %u slices do not say the value", tb.name.c_str(), bits, pat, t);
            }
        }
    }
    printf("msm bits rule: %d cases, %d failures\n", cases, bad);
    return bad ? 1 : 0;
}

// ---- every field of a plan, the ranges and the launches it implies
static std::string dump(const MsmPlan& p) {
    auto S = [](unsigned long long v) { return std::to_string(v) + ","; };
    const MsmGeom& g = p.g;
    const MsmSizes& b = p.bytes;
    std::string s = "g=";
    for (unsigned long long v : {(unsigned long long)g.c, (unsigned long long)g.nwin, (unsigned long long)g.nb, (unsigned long long)g.nchunk, (unsigned long long)g.n,
                                 (unsigned long long)g.chunk, (unsigned long long)g.ns, (unsigned long long)g.plane_stride, (unsigned long long)g.nslice,
                                 (unsigned long long)g.shared, (unsigned long long)g.run_limit, (unsigned long long)g.piece, (unsigned long long)g.resume,
                                 (unsigned long long)g.interleave, (unsigned long long)g.split_log, (unsigned long long)g.more, (unsigned long long)g.glv})
        s += S(v);
    s += " off=";
    for (uint16_t o : g.off) s += S(o);
    s += " sg=" + S(p.sg.lo_bits) + S(p.sg.nhi) + " lens=";
    for (uint64_t l : p.lens) s += S(l);
    s += " plan=" + S(p.range) + S(p.overlap) + S(p.nwin1) + S(p.over_cap) + S(p.desc_cap) + S(p.nbuf) + S(p.over_bytes) + S(p.poll_result) +
         S((unsigned)p.ps_tile) + S(p.ps_lds) + " bytes=";
    for (size_t v : {b.digits, b.sorted, b.counts, b.entries, b.start, b.perm, b.over, b.pieces, b.buckets, b.parts, b.pyr1, b.odd0, b.odd1, b.result, b.host_result})
        s += S(v);
    s += " fold=";
    for (uint32_t t = 0; t < g.split_log; t++) s += S(p.fold[t].pairs) + S(p.fold[t].lane) + S(p.fold[t].grid_x);
    s += " red=" + S(p.red.nlevel) + S(p.red.tail_blocks) + S(p.red.tail_threads);
    for (uint32_t k = 0; k < p.red.nlevel; k++) s += S(p.red.level[k].level) + S(p.red.level[k].half) + S(p.red.level[k].quad) + S(p.red.level[k].grid_x);
    s += " ranges=";
    for (size_t r = 0; r < p.lens.size(); r++) {
        const MsmRange x = range_geom(p, r);
        const AccLaunch a = acc_launch(p, x.g);
        const SortLaunch sl = sort_launch(p.sg, x.g);
        s += S(x.off) + S(x.len) + S(x.set) + S(x.g.n) + S(x.g.chunk) + S(x.g.resume) + S(x.g.more) + S(a.quad) + S(a.grid) + S(a.combine_x) + S(sl.digits_x) +
             S(sl.prefix_x) + S(sl.rank_x) + ";";
    }
    return s;
}
static std::string plan_of(const MsmBases& b, size_t count, size_t n, bool feed, int bits /* < 0: the default argument */, int* rc) {
    MsmPlan p;
    MsmFeedRanges fr;
    if (feed) fr = msm_feed_ranges(n);
    *rc = bits < 0 ? plan_msm(b, count, n, feed ? &fr : nullptr, 2048, &p) : plan_msm(b, count, n, feed ? &fr : nullptr, 2048, &p, (unsigned)bits);
    if (*rc) return "rc=" + std::to_string(*rc) + " " + p.error;
    return p.lens.empty() ? "empty" : dump(p);
}

static int plans() {
    int cases = 0;
    for (const char* range_log : {(const char*)nullptr, "10"}) {
        for (int k = 0; k < KNOB_MSM_PLAN_END; k++) unsetenv(kKnobs[k].name);
        if (range_log) setenv("ZKP_MSM_RANGE_LOG", range_log, 1);
        for (int glv : {0, 1})
            for (uint32_t w : {0u, 12u, 16u, 20u, 22u}) {
                if (glv && !w) continue;
                MsmSlices sl{};
                if (w) sl = msm_slice_offsets(glv ? 129 : 256, w, 1);
                for (size_t n : {(size_t)1, (size_t)65, (size_t)2047, (size_t)2048, (size_t)4096, (size_t)1 << 16, (size_t)1 << 20, ((size_t)1 << 24) + 5}) {
                    if (range_log && n > 4096) continue;
                    const MsmBases full{n + 3, w ? sl.widest : 0u, w ? sl.planes : 0u, sl.off, (uint32_t)glv};
                    for (size_t count : {(size_t)1, (size_t)3, (size_t)33, (size_t)64}) {
                        if (count > 3 && n > 4096) continue;  // (workspaces of batches of large MSMs: nothing the bound changes)
                        for (int feed = 0; feed <= (w && count == 1 && n >= (1u << 19) ? 1 : 0); feed++) {
                            int rc0, rc;
                            const std::string today = plan_of(full, count, n, feed, -1, &rc0);
                            for (int bits = 1; bits <= 256; bits++) {
                                cases++;
                                const std::string got = plan_of(full, count, n, feed, bits, &rc);
                                const std::string where = "w=" + std::to_string(w) + " glv=" + std::to_string(glv) + " n=" + std::to_string(n) + " count=" +
                                                          std::to_string(count) + " feed=" + std::to_string(feed) + " bits=" + std::to_string(bits);
                                if (bits >= (int)MSM_BITS_WHOLE || (glv && bits > (int)MSM_BITS_GLV_ONE_SET)) {
                                    // whole scalars, and split planes above 127 bits: today's plan, refusals included (33 split MSMs)
                                    EXPECT(got == today && rc == rc0, "%s\n  got  %s\n  want %s", where.c_str(), got.c_str(), today.c_str());
                                    if (glv && count == 33) EXPECT(rc == ZKP_E_ARG, "%s: 33 split MSMs accepted", where.c_str());
                                    continue;
                                }
                                if (w) {  // the plan over the first t planes, as plain planes
                                    const uint32_t t = msm_bound_slices(sl.off, sl.planes, (unsigned)bits);
                                    const MsmBases first{n + 3, sl.widest, t, sl.off, 0};
                                    int rc1;
                                    const std::string want = plan_of(first, count, n, feed, -1, &rc1);
                                    EXPECT(got == want && rc == rc1, "%s\n  got  %s\n  want %s", where.c_str(), got.c_str(), want.c_str());
                                    EXPECT(rc == ZKP_OK, "%s: refused", where.c_str());  // (a batch of 64 over split planes too)
                                    MsmPlan p;
                                    if (plan_msm(full, count, n, nullptr, 2048, &p, (unsigned)bits) == ZKP_OK)
                                        EXPECT(p.g.glv == 0 && p.g.nwin == count && p.nwin1 == t && p.g.nslice == t && p.g.n == (uint64_t)t * p.range,
                                               "%s: one plain bucket set per MSM over t planes", where.c_str());
                                } else {  // per-window mode has no planes to drop: the same formulas over t windows per scalar
                                    MsmPlan p, f;
                                    EXPECT(plan_msm(full, count, n, nullptr, 2048, &p, (unsigned)bits) == ZKP_OK && plan_msm(full, count, n, nullptr, 2048, &f) == ZKP_OK,
                                           "%s: refused", where.c_str());
                                    uint16_t off[36];
                                    for (uint32_t s = 0; s <= f.nwin1; s++) off[s] = (uint16_t)(s * f.g.c);
                                    const uint32_t t = msm_bound_slices(off, f.nwin1, (unsigned)bits);
                                    EXPECT(p.nwin1 == t && p.g.nslice == t && p.g.nwin == t * count && p.g.n == n && p.g.c == f.g.c && p.g.nb == f.g.nb &&
                                               p.g.shared == 0 && p.g.glv == 0 && p.lens == f.lens,
                                           "%s: per-window geometry", where.c_str());
                                    bool offs = true;
                                    for (uint32_t s = 0; s < 36; s++) offs = offs && p.g.off[s] == (s <= t ? s * p.g.c : 0u);
                                    EXPECT(offs, "%s: offsets", where.c_str());
                                    const size_t W = p.g.nwin;
                                    EXPECT(p.g.nchunk == std::min<uint64_t>(std::max<uint32_t>(1, (512 + p.g.nwin - 1) / p.g.nwin), (n + 4095) / 4096) &&
                                               p.bytes.digits == 4 * W * n && p.bytes.buckets == 256 * W * p.g.nb && p.bytes.host_result == 256 * W * p.g.c + 4 * W,
                                           "%s: sizes follow the windows", where.c_str());
                                    ReducePlan red{};
                                    const char* err = nullptr;
                                    bool same = plan_reduce(p.g.c, p.g.nwin, 2048, &red, &err) == ZKP_OK && red.nlevel == p.red.nlevel &&
                                                red.tail_blocks == p.red.tail_blocks && red.tail_threads == p.red.tail_threads;
                                    for (uint32_t k = 0; same && k < red.nlevel; k++) same = std::memcmp(&red.level[k], &p.red.level[k], sizeof(PyrLaunch)) == 0;
                                    EXPECT(same, "%s: reduce plan", where.c_str());
                                    if (t == f.nwin1) EXPECT(dump(p) == dump(f), "%s: every window kept, yet another plan", where.c_str());
                                }
                            }
                        }
                    }
                }
            }
    }
    {  // bounds outside 1..256
        MsmPlan p;
        const MsmBases b{64, 0, 0, nullptr, 0};
        EXPECT(plan_msm(b, 1, 64, nullptr, 2048, &p, 0) == ZKP_E_ARG && plan_msm(b, 1, 64, nullptr, 2048, &p, 257) == ZKP_E_ARG, "bits 0 / 257 accepted");
    }
    printf("msm bits plans: %d cases, %d failures\n", cases, bad);
    return bad || !cases ? 1 : 0;
}

int main(int argc, char** argv) {
    const std::string mode = argc > 1 ? argv[1] : "";
    if (mode == "rule") return rule();
    if (mode == "plans") return plans();
    printf("usage: msm_bits_plan rule|plans\n");
    return 2;
}
