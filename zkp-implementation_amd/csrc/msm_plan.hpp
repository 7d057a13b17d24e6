// msm_plan.hpp -- the host-side plan of one MSM pass (msm_partial_batch, msm_host.inc): window choice, scalar ranges, the
// geometry the kernels of msm.hpp receive, the byte size of every workspace, and the shape of every launch: the geometry of each
// range (range_geom), the accumulate and its fold steps (acc_launch, MsmPlan::fold), the bucket reduction (plan_reduce) and the
// addressing of its pyramid (pyr_item, pyr_result), which the kernels call too.  Plain C++17 without HIP, so that
// tests/host/msm_plan_table.cpp can check it with g++ alone; msm.hpp includes it (after ff.hpp: ZKP_HD).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "../../include/zkp_hip.h"
#include "knobs.hpp"

namespace zkp {

#ifdef ZKP_HD  // (hipcc: the kernels of msm.hpp call the addressing functions below)
#define ZKP_MSMPLAN_FN ZKP_HD
#else
#define ZKP_MSMPLAN_FN inline
#endif

// Two modes.  Per-window buckets (default): every c-bit window of every MSM of a batch is its own "sort window" with
// n = ns entries and 2^(c-1) buckets.  Shared buckets (bases expanded with zkp_g1_bases_precompute): the W windows of a
// scalar address W pre-multiplied copies of the base (planes 2^(c s) P_i), so ALL of them fall into ONE bucket set:
// the sort window has n = W * ns entries, entry e = s * ns + i selects plane s, point i.
struct MsmGeom {
    uint32_t c;        // window bits
    uint32_t nwin;     // sort windows (bucket sets) in this pass
    uint32_t nb;       // buckets per window = 2^(c-1)   (bucket ids 1..nb)
    uint32_t nchunk;   // chunks per window in the counting sort
    uint64_t n;        // entries per sort window
    uint64_t chunk;    // entries per chunk
    uint64_t ns;       // scalars per MSM
    uint64_t plane_stride;  // points per plane of the expanded bases (shared mode)
    uint32_t nslice;   // c-bit windows per scalar
    uint32_t shared;   // 1: shared bucket set
    uint32_t run_limit;  // buckets with more entries are cut into pieces (msm_order)
    uint32_t piece;      // entries per piece
    uint32_t resume;     // 1: the buckets already hold the sums of earlier passes over other scalar ranges (shared mode)
    uint16_t off[36];    // bit offset of every slice of a scalar (off[nslice] >= 256); widths <= c
    uint32_t interleave; // 1: msm_accumulate walks the bucket sets interleaved (see there)
    uint32_t split_log;  // 2^split_log lanes (quads) share a bucket's run, one contiguous part each (small problems, see msm_accumulate)
    uint32_t more;       // 1: another scalar range follows: the bucket sums go to the hand-over array (msm_accumulate_body), not to `buckets`
    uint32_t glv;        // 1: endomorphism-split planes: MSM m owns bucket sets 2m (k mod lambda) and 2m + 1 (k div lambda), see glv.hpp
};

// Counting sort geometry (msm.hpp): bucket ids are 1..nb; (b - 1) = hi * 2^lo_bits + lo.
struct SortGeom {
    uint32_t lo_bits;  // 8 or 9 (at most c - 1): bins of the second pass
    uint32_t nhi;      // partitions per window = nb >> lo_bits
};

constexpr int MSM_MAX_BATCH = 64;
constexpr uint32_t SORT_MAX_PART = 8192;  // partitions per window: 2^(c-1) buckets = partitions x (256 .. 1024 bins)
constexpr uint32_t MSM_MAX_WINDOW_BITS = 24;  // widest window of zkp_g1_bases_precompute (bounded by the sort geometry above)
constexpr uint32_t PYR_BAR_STRIDE = 32;  // words between the barrier counters of two windows (msm_pyramid_tail): a 128-byte line each
// bucket lanes / bucket quads below which a bucket's run is split: enough for TWO generations of workgroups, so that the dispatcher
// evens out the longest runs (PLONK 2^16: 3.83 -> 3.75 ms per proof, round 5)
constexpr uint64_t SPLIT_FILL_LANES = 6 * 1024 * 64, SPLIT_FILL_QUADS = 2 * 1024 * 64 / 4 * 2;
constexpr uint32_t MSM_MAX_SPLIT_LOG = 2;  // eight parts measured no better than four (2^16 single 0.535 against 0.529 ms, batches worse)
static_assert(kKnobs[KNOB_MSM_SPLIT_LOG].hi == MSM_MAX_SPLIT_LOG, "ZKP_MSM_SPLIT_LOG's range");
constexpr int MSM_THREADS = 256;
constexpr int ACC_THREADS = 256;  // workgroup size of msm_accumulate (64 and 128 measure the same)
constexpr uint32_t PYR_TAIL_THREADS = 256;    // four waves = 64 cooperative adds per workgroup and round
constexpr uint32_t PYR_TAIL_BLOCKS = 16;      // workgroups per window at most (1024 adds per round)
static_assert(kKnobs[KNOB_PYR_TAIL_THREADS].dflt == PYR_TAIL_THREADS && kKnobs[KNOB_PYR_TAIL_BLOCKS].dflt == PYR_TAIL_BLOCKS, "knobs.hpp");

#ifndef ZKP_PS_TILE
#define ZKP_PS_TILE 12288
#endif
// entries per tile of the first pass, as large as the 160 KB of LDS allow next to the 12 bytes per partition: 12288 entries over up to
// 2048 partitions leave as 48..96-byte runs (147 KB; 8192: 32..64-byte runs; round 4, profiles/r04_m: together with the 16384-entry
// second pass the sort goes 0.192 -> 0.176 ms at 2^20, 0.63 -> 0.57 at 2^22, 2.49 -> 2.3 ms at 2^24), 8192 up to 4096 partitions
// (131 KB), 4096 up to 8192 partitions -- 24-bit windows -- (139 KB).  One workgroup per CU, no loss on small problems.
constexpr int PS_TILE_BIG = ZKP_PS_TILE, PS_TILE_MID = 8192, PS_TILE_SMALL = 4096;
ZKP_MSMPLAN_FN size_t partscatter_lds_bytes(uint32_t nhi, int tile) { return 8 * (size_t)tile + 2 * (size_t)tile + 4 * (size_t)(3 * nhi + 1); }
ZKP_MSMPLAN_FN int partscatter_tile(uint32_t nhi) { return nhi <= 2048 ? PS_TILE_BIG : nhi <= 4096 ? PS_TILE_MID : PS_TILE_SMALL; }

// Physical position of logical entry i of an n-entry level of the reduction pyramid (msm_pyramid_kernel): even entries in the first
// half, odd entries in the second.  The bucket array is level 0 (n = nb, i = bucket - 1).
ZKP_MSMPLAN_FN uint64_t pyr_pos(uint32_t i, uint32_t n) { return (uint64_t)(i >> 1) + (uint64_t)(i & 1u) * (n >> 1); }

// Plane of a shared-mode entry (msm_accumulate_run): pt / ns for pt, ns < 2^31 with ONE multiply-high by m = floor((2^32 - 1) / ns),
// made once per run, and a one-step correction: 7 instructions per insertion where the 32-bit division took 15 (two correction steps and
// a remainder, its reciprocal already hoisted by the compiler; profiles/acc_insertion_overhead.md).
// m ns >= 2^32 - ns, so pt m / 2^32 >= pt / ns - pt / 2^32 > pt / ns - 1/2: the estimate is floor(pt / ns) or one below it, never
// above (m <= 2^32 / ns), and r = pt - q ns < 2 ns < 2^32 does not wrap.  tests/host/locate_div.cpp checks it against `/`.
struct PlaneDiv {
    uint32_t ns, m;
};
ZKP_MSMPLAN_FN PlaneDiv plane_div_make(uint32_t ns) { return PlaneDiv{ns, ns ? 0xffffffffu / ns : 0u}; }
ZKP_MSMPLAN_FN uint32_t plane_div(const PlaneDiv& d, uint32_t pt) {
    const uint32_t q = (uint32_t)(((uint64_t)pt * d.m) >> 32);
    return q + (pt - q * d.ns >= d.ns ? 1u : 0u);
}

// One launch of the bucket reduction (the schedule: msm.hpp, above msm_pyramid_kernel)
struct PyrLevel {
    uint32_t level;  // l
    uint32_t half;   // nb >> (l+1)
    uint32_t nb;
    uint32_t nwin;
};
ZKP_MSMPLAN_FN uint64_t odd_off(uint32_t nb, uint32_t j) { return (uint64_t)nb - (nb >> j); }
// operands and destination of item (kind, s) of launch `level`: entry offsets inside the buffers named by the flags
struct PyrItem {
    uint64_t a, b, d;
    bool src_is_pyr_out;  // kind j + 1 == level: the operands are level j's odd half, in the pyramid buffer this launch also writes
};
ZKP_MSMPLAN_FN PyrItem pyr_item(uint32_t nb, uint32_t level, uint32_t half, uint32_t kind, uint32_t s, uint64_t wbase) {
    PyrItem it;
    if (kind == 0) {
        it.a = wbase + s;
        it.b = wbase + half + s;
        it.d = wbase + pyr_pos(s, half);
        it.src_is_pyr_out = false;
    } else {
        const uint64_t o = wbase + odd_off(nb, kind - 1);
        it.src_is_pyr_out = kind == level;
        const uint64_t src = it.src_is_pyr_out ? wbase + 2 * (uint64_t)half : o;  // level j = level - 1 has 4 half entries: odd half at [2 half, 4 half)
        it.a = src + s;
        it.b = src + half + s;
        it.d = o + s;
    }
    return it;
}
// Where result e of a bucket set (0: sum(B) = A_{c-1}[0]; 1 + j: U_j, j < c - 1) sits after launch c - 2: what the last-levels launch
// and msm_collect_kernel gather.  U_{c-2} is the odd entry of the two-entry level c - 2, still in the other pyramid buffer.
// pyr_final / odd_final: the pyramid and odd buffers of parity (c - 1) & 1, pyr_prev: the other pyramid buffer; wbase: the set's first entry
template <class T>
ZKP_MSMPLAN_FN T* pyr_result(T* pyr_final, T* pyr_prev, T* odd_final, uint64_t wbase, uint32_t nb, uint32_t c, uint32_t e) {
    return e == 0 ? pyr_final + wbase : e == c - 1 ? pyr_prev + (wbase + 1) : odd_final + (wbase + odd_off(nb, e - 1));
}

// Window width: only widths dividing 256 leave no sparse top window (others 4-9x slower, profiles/r01_window_sweep.txt); below 8 bits
// a scalar has more than 32 windows (MsmGeom::off holds 36 offsets).
inline unsigned pick_window_bits(size_t n) { return (unsigned)knob_int(KNOB_MSM_C, n >= 2048 ? 16 : 8); }

// The shape of the bases an MSM runs over (zkp_bases): pre_c != 0 means pre_planes expanded planes, plane s = 2^pre_off[s] * P;
// glv != 0: the planes cover the 129 bits of a scalar half only (zkp_g1_bases_precompute_glv)
struct MsmBases { uint64_t n; uint32_t pre_c, pre_planes; const uint16_t* pre_off; uint32_t glv = 0; };

// Slices of an expansion (zkp_g1_bases_precompute*): ceil(cover / window_bits) planes over `cover` bits -- 256 for whole scalars, 129
// for the halves of the endomorphism split (both at most lambda + 1 < 0.674 * 2^128: with 128 bits the top signed digit would carry
// out and msm_digits drops that carry; with 129 the top slice stays below half its range, as r < 2^255 keeps it for 256).  When that
// many windows of window_bits overshoot the cover, the top window is short by that many bits and its 2^-k of the buckets collect 2^k
// times the points of the others; from `balance_from` bits of overshoot on (ZKP_MSM_BALANCE_FROM, default: any) the cover is split
// into slices of floor/ceil(cover / planes) bits instead (256 bits: 18 -> 15 slices of 17/18 bits, 19 -> 14 of 18/19, 20 -> 13 of
// 19/20; 129 bits: 22 -> 6 of 21/22, 20 -> 7 of 18/19).  Round 3: from ANY overshoot on (rounds 1-2: from 8 bits) -- at 20 bits the
// 4-bit overshoot left 2^14 buckets with ~90 entries against 26 on average at 2^20 points, and those 256 waves, dispatched first,
// were still walking their runs alone when the rest of the machine had finished (profiles/r03_j_balanced_slices.md).
struct MsmSlices {
    uint32_t planes, widest;  // widest slice in bits: 2^(widest - 1) buckets
    uint16_t off[36];         // plane s holds 2^off[s] * P; off[planes] >= cover
};
inline MsmSlices msm_slice_offsets(uint32_t cover, uint32_t window_bits, uint32_t balance_from) {
    MsmSlices s{};
    s.planes = cover / window_bits + (cover % window_bits ? 1 : 0);
    s.widest = window_bits;
    if (s.planes > 35) return s;  // (window_bits below 8: refused by the callers)
    if (s.planes * window_bits - cover < balance_from) {
        for (uint32_t k = 0; k <= s.planes; k++) s.off[k] = (uint16_t)(k * window_bits);
    } else {
        const uint32_t base = cover / s.planes, rem = cover % s.planes;
        s.widest = base + (rem ? 1 : 0);
        for (uint32_t k = 0; k < s.planes; k++) s.off[k + 1] = (uint16_t)(s.off[k] + base + (k < rem ? 1 : 0));
    }
    return s;
}

// A bound on the scalars (zkp_msm_g1_bits*): canonical values below 2^bits need only the first t slices of an offset table off[0..nslice],
// t the smallest index with off[t] >= bits + 1, at most nslice.  Slice s takes the bits [off[s], off[s + 1]) plus the carry of the slice
// below and hands a carry up when that exceeds half its range (msm_recode).  The bit at position `bits` is zero, so the slice that holds it
// stays below half its range whatever arrives from below, and nothing leaves slice t - 1: the t digits say the scalar exactly.  With
// t - 1 slices off[t - 1] <= bits, every bit of 2^bits - 1 below off[t - 1] is set, and the top slice kept carries out: t is minimal.
// From 255 bits on the bound says nothing (r < 2^255): MSM_BITS_WHOLE and above plan the whole scalar.
// tests/host/msm_bits_plan.cpp checks the rule against brute force for every table the library makes.
constexpr unsigned MSM_BITS_WHOLE = 255, MSM_BITS_MAX = 256;
constexpr unsigned MSM_BITS_GLV_ONE_SET = 127;  // lambda = z^2 - 1 > 2^127: a scalar below 2^127 is its own low half, the high half is 0
inline uint32_t msm_bound_slices(const uint16_t* off, uint32_t nslice, unsigned bits) {
    uint32_t t = 1;
    while (t < nslice && off[t] < bits + 1) t++;
    return t;
}

// Host-fed scalars (zkp_msm_g1, shared-bucket mode): ranges of at most 2^range_log scalars; first_len != 0: a short first range (its
// upload is the exposed one), second_len != 0: then a second short one, then the rest
struct MsmFeedRanges { uint64_t range_log = 0, first_len = 0, second_len = 0; };

// The ranges a host feed of n scalars asks for.  The first range's upload is exposed and every range pays a pass over the buckets,
// so the first is just long enough for its kernels to cover the next upload: 25 % + 75 % up to 2^21 terms, from there
// 10 % + 30 % + 60 % (2^24: 36.0 -> 34.0 ms; profiles/r04_i, profiles/r05_o).
inline MsmFeedRanges msm_feed_ranges(uint64_t n) {
    MsmFeedRanges f;
    uint64_t parts = 2;
    unsigned first_pct = n >= (1u << 21) ? 10 : 25;
    const int ranges = (int)knob_int(KNOB_MSM_FEED_RANGES);  // equal ranges, as rounds 2-3 (tuning aid)
    if (ranges) { parts = (uint64_t)ranges; first_pct = 0; }
    first_pct = (unsigned)knob_int(KNOB_MSM_FEED_FIRST_PCT, first_pct);  // share of the first range (0 = equal ranges)
    const unsigned second_pct = (unsigned)knob_int(KNOB_MSM_FEED_SECOND_PCT, n >= (1u << 21) ? 30 : 0);  // a second short range
    if (first_pct) {
        f.first_len = std::max<uint64_t>(1024, (n * first_pct / 100) & ~(uint64_t)1023);
        if (second_pct) f.second_len = std::max<uint64_t>(1024, (n * second_pct / 100) & ~(uint64_t)1023);
        parts = 1;  // the rest in one piece (or as many as the range limit asks for)
    }
    while ((parts << f.range_log) < n) f.range_log++;
    return f;
}

// Byte sizes of the workspaces of one pass (Ctx's DevBufs of the same names; host_result is pinned)
struct MsmSizes {
    size_t digits, sorted, counts, entries, start, perm, over, pieces, buckets, parts, pyr1, odd0, odd1, result, host_result;
};

// The launches of the bucket reduction: levels 0 .. nlevel - 1 each as their own launch of grid (grid_x, level + 1, nwin), then ONE
// launch of grid (tail_blocks, nwin) x tail_threads for the levels nlevel .. c - 2 and the gathering -- or, tail_blocks == 0, only
// the gathering (msm_collect_kernel): every level ran as its own launch.
struct PyrLaunch { uint32_t level, half, quad, grid_x; };  // quad: four lanes per add
struct ReducePlan {
    uint32_t nlevel, tail_blocks, tail_threads;
    PyrLaunch level[MSM_MAX_WINDOW_BITS];
};

// The reduction of nwin bucket sets of 2^(c-1) buckets on a device that keeps tail_max_waves waves of the last-levels launch
// resident.  Tuning aids (A/B runs): ZKP_PYR_TAIL_THREADS / _BLOCKS, workgroup size and count of that launch, and ZKP_PYR_TAIL_HALF,
// the per-array pair count from which it takes over; out of range: ZKP_E_ARG and *error.
inline int plan_reduce(uint32_t c, uint32_t nwin, uint32_t tail_max_waves, ReducePlan* r, const char** error) {
    const uint32_t tail_threads = (uint32_t)knob_int(KNOB_PYR_TAIL_THREADS), tail_blocks = (uint32_t)knob_int(KNOB_PYR_TAIL_BLOCKS);
    const uint32_t tail_half = (uint32_t)knob_int(KNOB_PYR_TAIL_HALF);
    if (tail_threads < 64 || tail_threads > 512 || (tail_threads & 63) || !tail_blocks || tail_blocks > 256 || !tail_half) {
        *error = "ZKP_PYR_TAIL_THREADS must be a multiple of 64 up to 512, ZKP_PYR_TAIL_BLOCKS 1..256, ZKP_PYR_TAIL_HALF >= 1";
        return ZKP_E_ARG;
    }
    if (c < 1 || c > MSM_MAX_WINDOW_BITS) {  // (ReducePlan::level; plan_msm's sort geometry has refused such a width before)
        *error = "bucket reduction: window width outside 1..24 bits";
        return ZKP_E_ARG;
    }
    const uint32_t nb = 1u << (c - 1);
    uint32_t level_tail = 0;  // first level whose per-array work is <= 64 pairs: the rest runs in one launch
    while (level_tail + 1 < c && (nb >> (level_tail + 1)) > tail_half) level_tail++;
    // ... unless even one workgroup per bucket set is more than the device keeps resident (many bucket sets, a partition with few
    // CUs): the barrier of that launch would spin for its whole time-out, so every level runs as its own launch instead
    if ((uint64_t)nwin * (tail_threads / 64) > tail_max_waves) level_tail = c - 1;
    for (uint32_t l = 0; l < level_tail; l++) {
        const uint32_t half = nb >> (l + 1);
        // levels with few adds are latency-bound: four lanes per add there (threshold swept 2^14..2^20: 2^16 is the minimum)
        const bool quad = (uint64_t)half * (l + 1) * nwin <= (1u << 16);
        const uint32_t per = quad ? MSM_THREADS / 4 : MSM_THREADS;  // adds per workgroup
        r->level[l] = {l, half, quad ? 1u : 0u, (half + per - 1) / per};
    }
    r->nlevel = level_tail;
    r->tail_threads = tail_threads;
    r->tail_blocks = 0;
    if (level_tail + 1 < c) {
        uint32_t tb = tail_blocks;
        while (tb > 1 && (uint64_t)tb * nwin * (tail_threads / 64) > tail_max_waves) tb >>= 1;
        r->tail_blocks = tb;
    }
    return ZKP_OK;
}

struct FoldStep { uint32_t pairs, lane, grid_x; };  // grid (grid_x, pairs); lane: one lane per add, else four

// buckets += parts, pairwise, over nwin bucket sets of nb buckets: split_log steps; a step with many adds runs one lane per add, a
// small one four (latency): msm.hpp.  Tuning aid: ZKP_FOLD_LANE_MIN, the adds in one launch from which the lane form is used.
inline void plan_fold(uint32_t nwin, uint32_t nb, uint32_t split_log, FoldStep* fold) {
    const uint64_t cap = (uint64_t)nwin * nb, lane_from = (uint64_t)knob_int(KNOB_FOLD_LANE_MIN);
    for (uint32_t t = 0; t < split_log; t++) {
        const uint32_t pairs = 1u << (split_log - 1 - t), lane = cap * pairs >= lane_from ? 1u : 0u;
        const uint32_t per = lane ? MSM_THREADS : MSM_THREADS / 4;  // adds per workgroup
        fold[t] = {pairs, lane, (uint32_t)((cap + per - 1) / per)};
    }
}

struct MsmPlan {
    MsmGeom g;                  // geometry of the longest range (range_geom narrows it for shorter ones)
    SortGeom sg;
    std::vector<uint64_t> lens; // the scalar ranges in order; empty: nothing to compute (count == 0 or n == 0)
    uint64_t range;             // the longest range: what the workspaces and the sort geometry are sized for
    bool overlap;               // several ranges: digits + sort of range r+1 on a second stream under the accumulate of range r
    uint32_t nwin1, over_cap, desc_cap;  // windows (slices) per scalar; oversized buckets and piece descriptors per window (msm_order)
    size_t nbuf, over_bytes;    // buffer sets of sorted / start / perm / over (2 with overlap); bytes of one set of `over`
    MsmSizes bytes;
    FoldStep fold[MSM_MAX_SPLIT_LOG];  // g.split_log steps of buckets += parts behind every accumulate
    ReducePlan red;
    bool poll_result;           // the host polls the result flags instead of waiting for the stream: up to 2^24 entries per bucket set in the last range
    int ps_tile;                // msm_partscatter_kernel<ps_tile> with ps_lds bytes of LDS: the largest tile whose staging fits next to 12 bytes per partition
    size_t ps_lds;
    const char* error;          // the message of a refusal (plan_msm's return value != ZKP_OK)
};

// THE choice between the two accumulate kernels: up to 2^20 entries four lanes per bucket -- one lane would be latency-bound by its
// longest run (tools/small_msm_bench.py) -- and only where the buckets neither resume nor hand over (a single range)
ZKP_MSMPLAN_FN bool acc_quad(const MsmGeom& g) { return !g.resume && !g.more && (uint64_t)g.n * g.nwin <= (1ull << 20); }

// Range ridx of the walk: where its scalars start, its buffer set (the sort of range r + 1 fills the other one under overlap) and
// the geometry its kernels receive
struct MsmRange {
    uint64_t off, len;
    uint32_t ridx, set;
    MsmGeom g;
};
inline MsmRange range_geom(const MsmPlan& p, size_t ridx) {
    MsmRange r{0, p.lens[ridx], (uint32_t)ridx, p.overlap ? (uint32_t)(ridx & 1) : 0u, p.g};
    for (size_t k = 0; k < ridx; k++) r.off += p.lens[k];
    if (r.len != p.g.ns) {  // a range shorter than the longest (the last one, or the first of a host-fed walk): smaller geometry
        r.g.ns = r.len;
        r.g.n = (uint64_t)p.nwin1 * r.len;
        r.g.chunk = (r.g.n + r.g.nchunk - 1) / r.g.nchunk;
    }
    r.g.resume = r.off ? 1u : 0u;
    r.g.more = ridx + 1 < p.lens.size() ? 1u : 0u;
    return r;
}

// grid.x of the digits, partprefix and rank launches of a range with geometry g (the sort's other grids are g.nchunk, sg.nhi and g.nwin)
struct SortLaunch { uint32_t digits_x, prefix_x, rank_x; };
inline SortLaunch sort_launch(const SortGeom& sg, const MsmGeom& g) {
    return {(uint32_t)((g.ns + MSM_THREADS - 1) / MSM_THREADS), (sg.nhi + 63) / 64, (g.nb + 1023) / 1024};
}

// The accumulate of a range with geometry g: msm_accumulate_quad_kernel or msm_accumulate_kernel over a 1-D grid of
// (bucket_blocks + extra_blocks) x nwin workgroups of ACC_THREADS, then msm_combine_kernel over (combine_x, nwin)
struct AccLaunch { uint32_t quad, per_block, bucket_blocks, extra_blocks, grid, combine_x; };
inline AccLaunch acc_launch(const MsmPlan& p, const MsmGeom& g) {
    AccLaunch a;
    a.quad = acc_quad(g) ? 1u : 0u;
    a.per_block = a.quad ? ACC_THREADS / 4 : ACC_THREADS;
    a.bucket_blocks = (uint32_t)((((uint64_t)g.nb << g.split_log) + a.per_block - 1) / a.per_block);
    a.extra_blocks = std::min<uint32_t>((p.desc_cap + a.per_block - 1) / a.per_block, 64);
    a.grid = (a.bucket_blocks + a.extra_blocks) * g.nwin;
    a.combine_x = std::min<uint32_t>(p.over_cap, 64);
    return a;
}

// Everything msm_partial_batch decides before it touches the device, for a device that keeps tail_max_waves waves of the
// reduction's last-levels launch resident (plan_reduce).  Reads the knobs of knobs.hpp before KNOB_MSM_PLAN_END.
// scalar_bits: every canonical scalar is below 2^scalar_bits (the caller's promise; the digits kernel of the bounded path checks it).
// From MSM_BITS_WHOLE on that is the plan of whole scalars.  Below it the plan is the one of bases that hold only the first
// t = msm_bound_slices planes -- per-window mode: of scalars with t windows -- and split planes run as plain ones up to
// MSM_BITS_GLV_ONE_SET bits (the high half is zero); with a wider bound they keep both bucket sets and every slice of a half.
inline int plan_msm(const MsmBases& bases_in, size_t count, size_t n, const MsmFeedRanges* feed, uint32_t tail_max_waves, MsmPlan* p,
                    unsigned scalar_bits = MSM_BITS_MAX) {
    auto refuse = [p](int code, const char* msg) { p->error = msg; return code; };
    p->lens.clear();
    if (scalar_bits < 1 || scalar_bits > MSM_BITS_MAX) return refuse(ZKP_E_ARG, "scalar bound outside 1..256 bits");
    MsmBases bases = bases_in;
    const bool bounded = scalar_bits < MSM_BITS_WHOLE;
    if (bounded && bases.pre_c && !(bases.glv && scalar_bits > MSM_BITS_GLV_ONE_SET)) {
        bases.pre_planes = msm_bound_slices(bases.pre_off, bases.pre_planes, scalar_bits);
        bases.glv = 0;
    }
    if (n > bases.n) return refuse(ZKP_E_SIZE, "more scalars than bases (kzg/src/scheme.rs:86)");
    if (count == 0 || n == 0) return ZKP_OK;
    if (n >= (1ull << 31)) return refuse(ZKP_E_ARG, "n >= 2^31");
    if (count > (size_t)MSM_MAX_BATCH) return refuse(ZKP_E_ARG, "batch of more than 64 MSMs");
    // expanded bases: always the shared bucket set (even 2^10 terms: 0.35 vs 0.85 ms on the per-window path)
    const bool shared = bases.pre_c != 0;
    // endomorphism-split planes: every MSM is a batch of two over the same planes (k mod lambda, k div lambda), one bucket set each
    const bool glv = shared && bases.glv != 0;
    const uint32_t sets = glv ? 2 : 1;
    if (sets * count > (size_t)MSM_MAX_BATCH)
        return refuse(ZKP_E_ARG, "batch of more than 32 MSMs over endomorphism-split bases (two bucket sets per MSM, 64 per pass)");
    MsmGeom& g = p->g = MsmGeom{};
    g.c = shared ? bases.pre_c : pick_window_bits(n);
    uint32_t nwin1 = shared ? bases.pre_planes : 256 / g.c + (256 % g.c ? 1 : 0);
    static_assert(sizeof(MsmGeom::off) / sizeof(uint16_t) == 36, "MsmGeom::off");
    if (nwin1 + 1 > 36) return refuse(ZKP_E_ARG, "more than 35 windows per scalar");
    if (bounded && !shared) {  // the windows a bounded scalar fills (off[s] = s c, as below)
        uint16_t off[36];
        for (uint32_t s = 0; s <= nwin1; s++) off[s] = (uint16_t)(s * g.c);
        nwin1 = msm_bound_slices(off, nwin1, scalar_bits);
    }
    p->nwin1 = g.nslice = nwin1;
    for (uint32_t s = 0; s <= nwin1; s++) g.off[s] = shared ? bases.pre_off[s] : (uint16_t)(s * g.c);
    g.shared = shared ? 1u : 0u;
    g.glv = glv ? 1u : 0u;
    // Shared mode walks the scalars in ranges: random 128-byte reads over more than ~26 GB of planes fall off a translation cliff
    // (profiles/r01_f_shared_buckets.md, profiles/r02_j_sort_under_accumulate.md).  Later ranges add into the same buckets.
    std::vector<uint64_t>& lens = p->lens;
    if (shared) {
        // The cap goes by insertions per scalar (split planes: two per plane), not by planes: 12 x 2^24 entries is what the
        // workspaces and the sort were measured with, and a split pass of 2 x 6 x 2^24 has exactly that many.  Its planes are half
        // as large (13 GB at 2^24), so the translation cliff is no nearer than in plain mode; longer split ranges are unmeasured.
        const uint64_t max_range = sets * bases.pre_planes <= 12 ? 1ull << 24 : 1ull << 23;
        uint64_t cap = feed ? std::min<uint64_t>(max_range, 1ull << feed->range_log) : max_range;
        if (const long long v = knob_int(KNOB_MSM_RANGE_LOG)) cap = 1ull << v;
        uint64_t want_first = feed ? feed->first_len : 0;
        if (!feed && count == 1) {  // tuning aid (resident scalars): a short first range whose sort is the exposed one
            const long long v = knob_int(KNOB_MSM_FIRST_PCT);
            if (v) want_first = std::max<uint64_t>(1024, ((uint64_t)n * v / 100) & ~(uint64_t)1023);
        }
        uint64_t done = 0;  // short ranges first (they obey the range limit like the others), then the rest in equal ranges of at most `cap`
        for (uint64_t want : {want_first, feed && want_first ? feed->second_len : (uint64_t)0})
            if (want && done + want < n) {
                lens.push_back(std::min<uint64_t>(want, cap));
                done += lens.back();
            }
        const uint64_t rest = n - done, rpass = (rest + cap - 1) / cap, rr = (rest + rpass - 1) / rpass;
        for (; done < n; done += lens.back()) lens.push_back(std::min<uint64_t>(rr, n - done));
    } else {
        lens.push_back(n);
    }
    const uint64_t range = p->range = *std::max_element(lens.begin(), lens.end());
    g.ns = range;
    g.plane_stride = bases.n;
    g.nwin = shared ? sets * (uint32_t)count : nwin1 * (uint32_t)count;  // sort windows = bucket sets
    g.n = shared ? (uint64_t)nwin1 * range : n;                   // entries per sort window
    if (g.n >= (1ull << 31)) return refuse(ZKP_E_ARG, "windows x scalars >= 2^31 with expanded bases");
    g.nb = 1u << (g.c - 1);
    g.interleave = (g.nwin > 1 && g.n <= (1ull << 22)) ? 1u : 0u;  // measured: +5 % at 2^22, 0 at 2^23, -5 % at 2^24
    const uint64_t entries = g.n;
    g.nchunk = (uint32_t)std::min<uint64_t>(std::max<uint32_t>(1, (512 + g.nwin - 1) / g.nwin), (entries + 4095) / 4096);
    if (const long long v = knob_int(KNOB_MSM_NCHUNK)) g.nchunk = (uint32_t)std::min<uint64_t>((uint64_t)v, entries);
    g.chunk = (entries + g.nchunk - 1) / g.nchunk;
    // a bucket is oversized above 4x the average run; its pieces are no longer than an average run (they execute next to
    // the ordinary lanes, so a longer piece would become the critical path)
    g.run_limit = (uint32_t)std::max<uint64_t>(128, 4 * (entries / g.nb));
    g.piece = (uint32_t)std::max<uint64_t>(32, entries / g.nb);
    SortGeom& sg = p->sg;
    // 2^19 buckets: 1024 partitions x 512 bins; 21..24-bit windows: 1024 bins per partition (measured, round 2)
    sg.lo_bits = std::min<uint32_t>(g.c >= 21 ? 10 : g.c >= 20 ? 9 : 8, g.c - 1);
    if (const long long lo = knob_int(KNOB_SORT_LO_BITS); lo && (uint32_t)lo < g.c) sg.lo_bits = (uint32_t)lo;  // tuning aid
    sg.nhi = g.nb >> sg.lo_bits;
    if (sg.nhi > SORT_MAX_PART) return refuse(ZKP_E_ARG, "window width above 24 bits is not supported by the sort");
    const size_t W = g.nwin, nb = g.nb, c = g.c;
    // Several scalar ranges: the (memory-bound) sort of range r+1 runs under the (issue-bound) accumulate of range r, on its own buffers
    p->overlap = shared && range < n && !knob_flag(KNOB_MSM_NO_OVERLAP);
    const size_t nbuf = p->nbuf = p->overlap ? 2 : 1;
    // oversized-bucket bookkeeping (msm_order): at most n / LIMIT oversized buckets and n / PIECE + that many pieces
    p->over_cap = (uint32_t)std::min<uint64_t>(entries / 128 + 1, (uint64_t)nb);  // also bounds the saturated bin
    p->desc_cap = (uint32_t)(entries / g.piece + entries / g.run_limit + 2);
    p->over_bytes = ((4 * W * (2 + (size_t)p->over_cap + p->over_cap + 1) + 16 * W * (size_t)p->desc_cap) + 255) & ~(size_t)255;
    // Few buckets for the machine (a small MSM over narrow windows, single pass): 2 or 4 lanes / quads share a bucket's run
    // (msm.hpp, split_run) so that narrow windows -- a short bucket reduction -- still fill the SIMDs.
    if (range >= n) {  // (g is that single range's geometry: neither resume nor more)
        const uint64_t units = (uint64_t)nb * W, want_units = acc_quad(g) ? SPLIT_FILL_QUADS : SPLIT_FILL_LANES;
        while (g.split_log < MSM_MAX_SPLIT_LOG && (units << g.split_log) < want_units) g.split_log++;
        g.split_log = (uint32_t)knob_int(KNOB_MSM_SPLIT_LOG, g.split_log);  // tuning aid
    }
    plan_fold(g.nwin, g.nb, g.split_log, p->fold);
    p->poll_result = range_geom(*p, lens.size() - 1).g.n <= (1ull << 24);
    p->ps_tile = partscatter_tile(sg.nhi);
    p->ps_lds = partscatter_lds_bytes(sg.nhi, p->ps_tile);
    if (const int rc = plan_reduce(g.c, g.nwin, tail_max_waves, &p->red, &p->error)) return rc;
    p->bytes = MsmSizes{4 * W * entries, nbuf * 4 * W * entries, 4 * W * ((size_t)g.nchunk * sg.nhi + 2 * sg.nhi + 1 + 512),
                        8 * W * entries, nbuf * 4 * W * (nb + 2), nbuf * 4 * W * nb, nbuf * p->over_bytes,
                        256 * W * (size_t)p->desc_cap, 256 * W * nb, 256 * W * nb * ((1u << g.split_log) - 1),
                        256 * W * nb, 256 * W * nb, 256 * W * nb, 4 * PYR_BAR_STRIDE * W, 256 * W * c + 4 * W};
    return ZKP_OK;
}

}  // namespace zkp
