// ntt_shard_plan.hpp -- what one call of the sharded Fr transform (ntt_sharded.inc, whose header comment defines the layouts and the
// two flows F and M) enqueues for one device slot: the split of N over the slots, the numbering of the events, and a flat list of
// operations cut into phases -- a phase is what a slot's host thread enqueues between two meetings at the barrier.  An operation is
// plain data: which stream, which element ranges of which slot's buffers, which event, which index map.  ntt_sharded.inc walks the
// list; tests/host/ntt_shard_plan.cpp checks it with g++ alone: against the operations recorded before the list existed, against
// the two ordering rules of the protocol over all slots' lists of a call, and by interpreting it over a small field.
// Plain C++17 without HIP and without the environment.
#pragma once
#include <algorithm>
#include <cstdint>
#include <string>
#include <vector>

#include "ntt_plan.hpp"  // NttRemap, PermuteSpec

namespace zkp {

struct ShardGeom {
    unsigned l1 = 0, l2 = 0, lw = 0;
    uint64_t G = 1, n1 = 0, n2 = 0, r1 = 0, r2 = 0, C = 1, cw = 0, slab = 0;
};

inline unsigned log2_exact(uint64_t v) {
    unsigned b = 0;
    while ((1ull << b) < v) b++;
    return b;
}

// the split is a function of (log_n, slots) only -- zkp_hip/dist.py: four_step_split is the same function, so that a vector left in
// the K1SLAB or COLUMNS layout by one transport can be read by the other.  Returns the message of a refusal, else an empty string.
inline std::string shard_geometry(unsigned log_n, uint64_t G, unsigned chunks, ShardGeom* o) {
    if (G == 0 || (G & (G - 1)) || G > 64) return "the sharded transform needs a power-of-two number of device slots (at most 64)";
    if (log_n > 32) return "log_n > 32 (two-adicity of the field)";
    ShardGeom g;
    g.G = G;
    g.lw = log2_exact(G);
    g.l1 = std::max<unsigned>(std::min<unsigned>(8, (log_n + 1) / 2), g.lw);
    if (log_n < g.l1 + g.lw + 2)
        return "transform too small for " + std::to_string(G) + " slots: N2 / slots = 2^" + std::to_string((int)log_n - (int)g.l1 - (int)g.lw) +
               " columns per slot, at least four are needed (128-byte runs of the tile kernels)";
    g.l2 = log_n - g.l1;
    g.n1 = 1ull << g.l1;
    g.n2 = 1ull << g.l2;
    g.r1 = g.n1 / G;
    g.r2 = g.n2 / G;
    if (chunks == 0) {
        g.C = 4;
        while (g.C > 1 && g.r2 / g.C < 4) g.C >>= 1;
    } else {
        if ((chunks & (chunks - 1)) || chunks > 64 || g.r2 / chunks < 4)
            return "chunks must be a power of two (at most 64) that leaves at least four columns per chunk: r2 = " + std::to_string(g.r2) +
                   ", chunks = " + std::to_string(chunks) + " (it is part of the COLUMNS layout and is never adjusted silently)";
        g.C = chunks;
    }
    g.cw = g.r2 / g.C;
    g.slab = (1ull << log_n) / G;
    *o = g;
    return std::string();
}

// The events of one slot: SEND1(q), RECV1(q), SEND2(q) per chunk q, then RECV2, SEND3, RECV3
enum { SH_EV_PER_CHUNK = 3, SH_EV_EXTRA = 3 };
inline uint32_t shard_event_count(const ShardGeom& G) { return (uint32_t)(SH_EV_PER_CHUNK * G.C + SH_EV_EXTRA); }

enum ShardLayout { SH_NATURAL = 0, SH_K1SLAB = 1, SH_COLUMNS = 2 };  // the values of ZKP_NTT_* (include/zkp_hip.h)
enum ShardStream : uint8_t { SH_LAUNCH = 0, SH_COPY = 1 };  // the slot's launch stream and the stream of its peer copies
enum ShardBuf : uint8_t { SH_SLAB = 0, SH_A = 1, SH_B = 2 };  // the slab (or its staging copy in the host form) and the two exchange buffers
enum ShardOpKind : uint8_t {
    SH_PERMUTE,  // fr_permute_kernel src -> dst by `perm`
    SH_PEER,     // copy of dst.count contiguous elements from another slot's buffer (or this slot's own)
    SH_AXIS0,    // run_ntt_axis0: matrix [2^len_log][batch] at src -> dst, twiddle omega_N^(+-(tw_first + column) k) when tw_log_n != 0
    SH_ROWS,     // run_ntt: `batch` transforms of 2^len_log through in_remap / out_remap, twiddle omega_N^(+-(tw_first + row) k)
    SH_COSET,    // dst[i] *= coset^(+-(tw_first + i))
    SH_RECORD,   // event (this slot, ev) on `stream`
    SH_WAIT      // `stream` waits for event (ev_slot, ev)
};
struct ShardRef {
    uint32_t slot;
    uint8_t buf;
    uint64_t off, count;  // the elements [off, off + count) the operation may touch: exact for contiguous operands, the bounding range for a
                          // strided view, the whole buffer behind an NttRemap
};
struct ShardOp {
    uint8_t kind, stream;
    const char* label;  // the profile scope it runs under, or null
    ShardRef src, dst;
    uint32_t ev_slot, ev;
    PermuteSpec perm;
    NttRemap in_remap, out_remap;
    unsigned len_log;
    uint64_t batch;
    unsigned tw_log_n;
    uint64_t tw_first;
};
struct ShardPlan {
    std::vector<ShardOp> ops;
    std::vector<size_t> phase_end;  // phase p is ops [phase_end[p - 1], phase_end[p]); phase 0 is the setup
};

// Appends the operations of slot g to its list, each under the profile label and in the phase that are current
struct ShardPlanner {
    const ShardGeom& G;
    const uint32_t g;
    const uint64_t blk, chunk;  // one peer's block of one chunk; one chunk = the matrix [N1][cw]
    const char* label = nullptr;
    ShardPlan plan;
    ShardPlanner(const ShardGeom& geom, size_t slot) : G(geom), g((uint32_t)slot), blk(geom.r1 * geom.cw), chunk(geom.G * geom.r1 * geom.cw) {
        plan.ops.reserve(G.C * (5 * G.G + 6) + 4 * G.G + 9);  // the longest list (NATURAL -> NATURAL): built once per call and slot, no regrowth
    }
    uint32_t SEND1(uint64_t q) const { return (uint32_t)q; }
    uint32_t RECV1(uint64_t q) const { return (uint32_t)(G.C + q); }
    uint32_t SEND2(uint64_t q) const { return (uint32_t)(2 * G.C + q); }
    uint32_t RECV2() const { return (uint32_t)(3 * G.C); }
    uint32_t SEND3() const { return RECV2() + 1; }
    uint32_t RECV3() const { return RECV2() + 2; }
    uint32_t peer(uint64_t i) const { return (uint32_t)((g + i) % G.G); }  // every slot starts with another partner
    ShardRef mine(uint8_t buf, uint64_t off, uint64_t count) const { return ShardRef{g, buf, off, count}; }
    ShardRef whole(uint8_t buf) const { return ShardRef{g, buf, 0, G.slab}; }

    ShardOp& add(uint8_t kind, uint8_t stream, ShardRef src = ShardRef(), ShardRef dst = ShardRef()) {
        ShardOp& op = plan.ops.emplace_back();  // (zeroed)
        op.kind = kind;
        op.stream = stream;
        op.label = label;
        op.src = src;
        op.dst = dst;
        return op;
    }
    void end_phase() {
        plan.phase_end.push_back(plan.ops.size());
        label = nullptr;
    }
    void event(uint8_t kind, uint8_t stream, uint32_t slot, uint32_t ev) {
        ShardOp& op = add(kind, stream);
        op.ev_slot = slot;
        op.ev = ev;
    }
    void wait(uint8_t stream, uint32_t slot, uint32_t ev) { event(SH_WAIT, stream, slot, ev); }
    void wait_all(uint8_t stream, uint32_t ev) {
        for (uint64_t i = 0; i < G.G; i++) wait(stream, peer(i), ev);
    }
    void record(uint32_t ev, uint8_t stream) { event(SH_RECORD, stream, g, ev); }
    void permute(uint8_t sbuf, uint64_t soff, uint8_t dbuf, uint64_t doff, const PermuteSpec& sp) {
        uint64_t in = 1, out = 1;  // the bounding ranges of the two strided views
        for (int d = 0; d < 4; d++) in += ((1ull << sp.bits[d]) - 1) * sp.in_stride[d], out += ((1ull << sp.bits[d]) - 1) * sp.out_stride[d];
        add(SH_PERMUTE, SH_LAUNCH, mine(sbuf, soff, in), mine(dbuf, doff, out)).perm = sp;
    }
    // B_g[q][p] <- A_p[q][g] (or the other way round: the same block arithmetic serves both exchanges), each block after the
    // event `send` of its owner
    void pull_chunk(uint64_t q, bool into_b, uint32_t send) {
        for (uint64_t i = 0; i < G.G; i++) {
            const uint32_t p = peer(i);
            wait(SH_COPY, p, send);
            add(SH_PEER, SH_COPY, ShardRef{p, (uint8_t)(into_b ? SH_A : SH_B), q * chunk + g * blk, blk}, mine(into_b ? SH_B : SH_A, q * chunk + p * blk, blk));
        }
    }
    void axis0(ShardRef src, ShardRef dst, unsigned tw_log_n, uint64_t col0) {
        ShardOp& op = add(SH_AXIS0, SH_LAUNCH, src, dst);
        op.len_log = G.l1;
        op.batch = G.cw;
        op.tw_log_n = tw_log_n;
        op.tw_first = col0;
    }
    ShardOp& rows(ShardRef src, ShardRef dst) {
        ShardOp& op = add(SH_ROWS, SH_LAUNCH, src, dst);
        op.len_log = G.l2;
        op.batch = G.r1;
        return op;
    }
    void coset_scale() { add(SH_COSET, SH_LAUNCH, ShardRef(), whole(SH_SLAB)).tw_first = G.slab * g; }
};

// The operations of slot g.  `host`: the host-pointer form (NATURAL in and out), `coset`: ... with a coset.  Every slot's list has the
// same phases, and every path of the walk passes the same barriers.
inline ShardPlan plan_shard(const ShardGeom& G, unsigned log_n, int inverse, int lin, int lout, bool host, bool coset, size_t g) {
    ShardPlanner P(G, g);
    const uint64_t C = G.C, cw = G.cw, r1 = G.r1, r2 = G.r2, n1 = G.n1, n2 = G.n2, blk = P.blk, chunk = P.chunk;
    const unsigned lcw = log2_exact(cw), lC = log2_exact(C), lr1 = log2_exact(r1), lr2 = log2_exact(r2), lW = G.lw;
    NttRemap gathered{};  // logical n2 = (p, q, c) of row j at [q][p][j][c]
    gathered.on = 1;
    gathered.lo_bits = lcw;
    gathered.mid_bits = lC;
    gathered.mid_stride = chunk;
    gathered.hi_stride = blk;
    gathered.batch_stride = cw;

    if (host && coset && !inverse) P.coset_scale();
    P.end_phase();  // setup: buffers, streams and events are published to the other slots
    if (lin != SH_K1SLAB) {
        const bool nat_in = lin == SH_NATURAL, nat_out = lout == SH_NATURAL;
        if (nat_in) {
            P.label = "ntt_sharded_pack";
            for (uint64_t q = 0; q < C; q++) {
                PermuteSpec sp{};
                sp.bits[1] = lW; sp.in_stride[1] = r2; sp.out_stride[1] = blk;   // h
                sp.bits[2] = lr1; sp.in_stride[2] = n2; sp.out_stride[2] = cw;   // j
                sp.bits[3] = lcw; sp.in_stride[3] = 1; sp.out_stride[3] = 1;     // c
                P.permute(SH_SLAB, q * cw, SH_A, q * chunk, sp);
                P.record(P.SEND1(q), SH_LAUNCH);
            }
            P.end_phase();
            for (uint64_t q = 0; q < C; q++) {
                P.pull_chunk(q, true, P.SEND1(q));
                P.record(P.RECV1(q), SH_COPY);
            }
            P.end_phase();
        }
        P.label = "ntt_sharded_columns";
        for (uint64_t q = 0; q < C; q++) {
            if (nat_in) P.wait(SH_LAUNCH, (uint32_t)g, P.RECV1(q));
            P.axis0(P.mine(nat_in ? SH_B : SH_SLAB, q * chunk, chunk), P.mine(SH_B, q * chunk, chunk), log_n, g * r2 + q * cw);
            P.record(P.SEND2(q), SH_LAUNCH);
        }
        P.end_phase();
        for (uint64_t q = 0; q < C; q++) {
            if (nat_in) P.wait_all(SH_COPY, P.RECV1(q));  // A[q] is the source of everybody's first pull of this chunk
            P.pull_chunk(q, false, P.SEND2(q));
        }
        P.record(P.RECV2(), SH_COPY);
        P.label = "ntt_sharded_exchange_wait";
        P.wait(SH_LAUNCH, (uint32_t)g, P.RECV2());
        P.end_phase();
        if (nat_out) P.wait_all(SH_LAUNCH, P.RECV2());  // the row transforms write B: not before everyone's second pull is through with it
        P.label = "ntt_sharded_rows";
        ShardOp& rows = P.rows(P.whole(SH_A), P.whole(nat_out ? SH_B : SH_SLAB));
        rows.in_remap = gathered;
        if (nat_out) {  // output k2 = (h, c) of row j goes to B[h][j][c], the send block of slot h
            rows.out_remap.on = 1;
            rows.out_remap.lo_bits = lr2;
            rows.out_remap.hi_stride = r1 * r2;
            rows.out_remap.batch_stride = r2;
        }
        P.label = nullptr;
        if (nat_out) P.record(P.SEND3(), SH_LAUNCH);
        else P.wait_all(SH_LAUNCH, P.RECV2());  // B stays a source until then
        P.end_phase();
        if (nat_out) {
            for (uint64_t i = 0; i < G.G; i++) {
                const uint32_t p = P.peer(i);
                P.wait(SH_COPY, p, P.SEND3());
                P.add(SH_PEER, SH_COPY, ShardRef{p, SH_B, (uint64_t)g * r1 * r2, r1 * r2}, P.mine(SH_A, p * r1 * r2, r1 * r2));
            }
            P.record(P.RECV3(), SH_COPY);
            P.label = "ntt_sharded_exchange_wait";
            P.wait(SH_LAUNCH, (uint32_t)g, P.RECV3());
            P.label = "ntt_sharded_unpack";
            PermuteSpec sp{};  // A[p][j][c] -> x[c][p r1 + j]: slot g's natural slab is k2 in [g r2, (g+1) r2), k = k1 + N1 k2
            sp.bits[1] = lr2; sp.in_stride[1] = 1; sp.out_stride[1] = n1;        // c
            sp.bits[2] = lW; sp.in_stride[2] = r1 * r2; sp.out_stride[2] = r1;   // p
            sp.bits[3] = lr1; sp.in_stride[3] = r2; sp.out_stride[3] = 1;        // j
            P.permute(SH_A, 0, SH_SLAB, 0, sp);
            if (host && coset && inverse) P.coset_scale();
            P.end_phase();
            P.wait_all(SH_LAUNCH, P.RECV3());
            P.end_phase();
        }
    } else {
        const bool cols_out = lout == SH_COLUMNS;
        P.label = "ntt_sharded_rows";
        ShardOp& rows = P.rows(P.whole(SH_SLAB), P.whole(SH_A));
        rows.out_remap = gathered;  // output n2 = (h, q, c) of row j goes to A[q][h][j][c]
        rows.tw_log_n = log_n;
        rows.tw_first = g * r1;
        P.label = nullptr;
        P.record(P.SEND1(0), SH_LAUNCH);
        P.end_phase();
        for (uint64_t q = 0; q < C; q++) {
            P.pull_chunk(q, true, P.SEND1(0));
            P.record(P.RECV1(q), SH_COPY);
        }
        P.label = "ntt_sharded_columns";
        for (uint64_t q = 0; q < C; q++) {
            P.wait(SH_LAUNCH, (uint32_t)g, P.RECV1(q));
            P.axis0(P.mine(SH_B, q * chunk, chunk), P.mine(cols_out ? SH_SLAB : SH_B, q * chunk, chunk), 0, 0);
            if (!cols_out) P.record(P.SEND2(q), SH_LAUNCH);
        }
        P.end_phase();
        if (cols_out) {  // A stays the source of the others' pulls until their events
            for (uint64_t q = 0; q < C; q++) P.wait_all(SH_LAUNCH, P.RECV1(q));
            P.end_phase();
        } else {
            for (uint64_t q = 0; q < C; q++) {
                P.wait_all(SH_COPY, P.RECV1(q));
                P.pull_chunk(q, false, P.SEND2(q));
            }
            P.record(P.RECV2(), SH_COPY);
            P.label = "ntt_sharded_exchange_wait";
            P.wait(SH_LAUNCH, (uint32_t)g, P.RECV2());
            P.label = "ntt_sharded_unpack";
            PermuteSpec sp{};  // x[j][p][q][c] = A[q][p][j][c]
            sp.bits[0] = lC; sp.in_stride[0] = chunk; sp.out_stride[0] = cw;     // q
            sp.bits[1] = lW; sp.in_stride[1] = blk; sp.out_stride[1] = r2;       // p
            sp.bits[2] = lr1; sp.in_stride[2] = cw; sp.out_stride[2] = n2;       // j
            sp.bits[3] = lcw; sp.in_stride[3] = 1; sp.out_stride[3] = 1;         // c
            P.permute(SH_A, 0, SH_SLAB, 0, sp);
            P.end_phase();
            P.wait_all(SH_LAUNCH, P.RECV2());
            P.end_phase();
        }
    }
    return std::move(P.plan);
}

}  // namespace zkp
