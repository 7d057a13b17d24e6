// ntt_sharded.inc -- included by api.hip.  The four-step Fr transform spread over the device slots of this process
// (include/zkp_hip.h: zkp_ntt_fr_sharded_dev, zkp_ntt_fr_sharded): BASELINE configs[4]'s NTT behind the C ABI, serving the
// GeneralEvaluationDomain call sites of the reference (plonk/src/prover.rs:70,374-375,396-443; plonk/src/circuit.rs:170-176).
//
// N = N1 x N2, index n = n1 N2 + n2 in, k = k1 + N1 k2 out.  Slot g owns rows [g r1, (g+1) r1) of the input matrix (NATURAL), or its
// columns [g r2, (g+1) r2) (COLUMNS), or rows k1 in [g r1, (g+1) r1) of the output matrix [k1][k2] (K1SLAB).
//
//   F  NATURAL / COLUMNS -> K1SLAB (-> NATURAL)
//      pack        A[q][h][j][c] = x[j][h r2 + q cw + c]                  (NATURAL in only: an exchange moves contiguous blocks)
//      exchange 1  B_g[q][p] <- A_p[q][g]: what arrives IS the matrix [N1][cw] of chunk q (all n1, my n2): no transpose
//      columns     axis-0 transforms of B[q] in place (COLUMNS in: x[q] -> B[q]), twiddle omega_N^(n2 k1) fused into the store
//      exchange 2  A_g[q][p] <- rows [g r1, (g+1) r1) of B_p[q] (contiguous: no pack)
//      rows        transforms of length N2 READ the gathered [q][p][j][c] layout, write x[j][k2]                      -> K1SLAB
//      (NATURAL out: the row transforms write B[h][j][c] instead, exchange 3 A_g[p] <- B_p[g], transpose A -> x[k2 - g r2][k1])
//   M  K1SLAB -> NATURAL / COLUMNS: the mirror image
//      rows        transforms of x[j][.] write the twiddled, scattered send blocks A[q][h][j][c] directly
//      exchange 1  B_g[q][p] <- A_p[q][g]    (the matrix [N1][cw] again)
//      columns     axis-0 transforms B[q] in place (COLUMNS out: B[q] -> x[q], done)
//      exchange 2  A_g[q][p] <- rows of my n1 slab of B_p[q];  unpack x[j][p][q][c] = A[q][p][j][c]
//
// Who copies: the RECEIVER pulls its G blocks per chunk on its own copy stream (`xstream`), after waiting -- on the device, with
// hipStreamWaitEvent across devices -- for the event the owner of the source recorded behind the kernel that produced it; the launch
// stream waits for the copy stream's event before it touches a chunk, so the copies of chunk q + 1 run under the column transforms
// of chunk q.  A buffer is rewritten only after the events of everyone who read it.  The host threads (one per slot,
// DeviceWorkers) meet at a barrier between "record" and "wait" -- an event must have been recorded before another thread may
// enqueue a wait on it -- and nowhere else; they never wait for the device unless the caller asked for a synchronous call.
//
// WHAT a slot enqueues -- every index, offset, event number and wait -- is data: plan_shard (ntt_shard_plan.hpp) lists the operations of
// one slot, cut into the phases between two barriers, and tests/host/ntt_shard_plan.cpp checks the lists of all slots against both
// rules above without a device.  This file is the mechanics: set a slot up, walk its list, finish.
#include "ntt_shard_plan.hpp"

namespace {

static_assert(SH_NATURAL == ZKP_NTT_NATURAL && SH_K1SLAB == ZKP_NTT_K1SLAB && SH_COLUMNS == ZKP_NTT_COLUMNS, "ntt_shard_plan.hpp layouts");

int shard_geom(unsigned log_n, uint64_t G, unsigned chunks, ShardGeom* o) {
    const std::string refusal = shard_geometry(log_n, G, chunks, o);
    return refusal.empty() ? ZKP_OK : fail(ZKP_E_ARG, refusal);
}

struct ShardSlot {
    Fr* x = nullptr;  // the slab (caller's memory, or the staging buffer of the host form)
    Fr* a = nullptr;
    Fr* b = nullptr;
    hipStream_t main = nullptr, xs = nullptr;
    int device = -1;
    const Event* ev = nullptr;
};
struct ShardCall {
    ShardGeom g;
    unsigned log_n = 0;
    int inverse = 0, lin = 0, lout = 0;
    void* const* d_slabs = nullptr;
    void* const* streams = nullptr;
    uint64_t* host = nullptr;       // host form: natural order in and out
    const uint64_t* coset = nullptr;
    bool sync = true;               // wait for the devices before returning
    std::vector<int> devices;       // HIP device of every slot (snapshot taken before the workers start)
    std::vector<ShardSlot> s;
    PhaseBarrier bar;
};

int peer_copy(void* dst, int dst_dev, const void* src, int src_dev, size_t bytes, hipStream_t st) {
    if (dst_dev == src_dev) HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, st));
    else HIPCHK(hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, bytes, st));
    return ZKP_OK;
}

int launch_permute(const Fr* in, Fr* out, const PermuteSpec& sp, hipStream_t st) {
    uint64_t total = 1;
    for (int d = 0; d < 4; d++) total <<= sp.bits[d];
    hipLaunchKernelGGL(fr_permute_kernel, dim3((unsigned)((2 * total + 255) / 256)), dim3(256), 0, st, reinterpret_cast<const uint4*>(in),
                       reinterpret_cast<uint4*>(out), sp, total);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

// c * coset^(+-(idx0 + i)) on a slab (the coset of coset_fft / coset_ifft in the host form)
int launch_coset_scale(Fr* data, uint64_t count, uint64_t idx0, unsigned log_n, int inverse, const uint64_t* coset, hipStream_t st) {
    PowTab<Fr> tab;
    ZCHK(get_coset_tables<Fr>(log_n, inverse, coset, HFr::one(), &tab, st));
    hipLaunchKernelGGL(scale_pow_kernel<Fr>, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, data, count, idx0, tab);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

// setup of slot g: buffers, streams, events, peer access, the upload of the host form; the barrier behind it publishes them to the others
int shard_setup(ShardCall& c, size_t g, std::unique_ptr<WsOrder>* order) {
    const ShardGeom& G = c.g;
    ShardSlot& me = c.s[g];
    Ctx& cx = ctx();
    me.device = cx.device;
    me.main = c.streams ? reinterpret_cast<hipStream_t>(c.streams[g]) : (g_rt.multi ? cx.stream : nullptr);
    if (!c.streams && !c.host) HIPCHK(hipDeviceSynchronize());  // the slab's producer may be any stream of this device
    order->reset(new WsOrder(me.main));
    const size_t bytes = sizeof(Fr) * G.slab;
    ZCHK(cx.xchg_a.ensure(bytes));
    ZCHK(cx.xchg_b.ensure(bytes));
    ZCHK(cx.xstream.ensure(hipStreamNonBlocking));
    while (cx.xev.size() < shard_event_count(G)) {
        Event e;
        ZCHK(e.ensure(hipEventDisableTiming));
        cx.xev.push_back(std::move(e));
    }
    if (!cx.peers_enabled) {  // direct reads of the other slots' devices; without it a peer copy is staged through the host
        for (int od : c.devices) {
            if (od == cx.device) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, cx.device, od) == hipSuccess && can) (void)hipDeviceEnablePeerAccess(od, 0);
            (void)hipGetLastError();  // already enabled (another slot on this device) is fine
        }
        cx.peers_enabled = true;
    }
    me.a = reinterpret_cast<Fr*>(cx.xchg_a.p);
    me.b = reinterpret_cast<Fr*>(cx.xchg_b.p);
    me.xs = cx.xstream;
    me.ev = cx.xev.data();
    if (c.host) {
        ZCHK(cx.tmp.ensure(bytes));
        me.x = reinterpret_cast<Fr*>(cx.tmp.p);
        HIPCHK(hipMemcpyAsync(me.x, c.host + 4 * G.slab * g, bytes, hipMemcpyHostToDevice, me.main));
    } else {
        me.x = reinterpret_cast<Fr*>(c.d_slabs[g]);
    }
    return ZKP_OK;
}

int shard_exec(const ShardCall& c, size_t g, const ShardOp& op) {
    const ShardSlot& me = c.s[g];
    const hipStream_t st = op.stream == SH_COPY ? me.xs : me.main;
    auto at = [&](const ShardRef& r) {
        const ShardSlot& s = c.s[r.slot];
        return (r.buf == SH_SLAB ? s.x : r.buf == SH_A ? s.a : s.b) + r.off;
    };
    switch (op.kind) {
    case SH_WAIT: HIPCHK(hipStreamWaitEvent(st, c.s[op.ev_slot].ev[op.ev], 0)); return ZKP_OK;
    case SH_RECORD: HIPCHK(hipEventRecord(me.ev[op.ev], st)); return ZKP_OK;
    case SH_PEER: return peer_copy(at(op.dst), me.device, at(op.src), c.s[op.src.slot].device, sizeof(Fr) * op.dst.count, st);
    case SH_PERMUTE: return launch_permute(at(op.src), at(op.dst), op.perm, st);
    case SH_AXIS0: return run_ntt_axis0<Fr>(at(op.src), at(op.dst), op.len_log, (size_t)op.batch, c.inverse, op.tw_log_n, op.tw_first, st);
    case SH_ROWS: {
        NttIo io;
        io.in_remap = op.in_remap.on ? &op.in_remap : nullptr;
        io.out_remap = op.out_remap.on ? &op.out_remap : nullptr;
        io.tw_log_n = op.tw_log_n;
        io.tw_row0 = op.tw_first;
        return run_ntt<Fr>(at(op.src), at(op.dst), op.len_log, (size_t)op.batch, c.inverse, nullptr, st, &io);
    }
    case SH_COSET: return launch_coset_scale(at(op.dst), op.dst.count, op.tw_first, c.log_n, c.inverse, c.coset, st);
    }
    return fail(ZKP_E_DEVICE, "internal error: unknown operation in a shard plan");
}

// the operations [first, end) of one phase, one profile scope per run of operations under the same label
int shard_phase(const ShardCall& c, size_t g, const ShardPlan& plan, size_t first, size_t end) {
    for (size_t i = first; i < end;) {
        const char* label = plan.ops[i].label;
        ProfScope ps(label, c.s[g].main);  // (no label: nothing is recorded)
        do ZCHK(shard_exec(c, g, plan.ops[i]));
        while (++i < end && plan.ops[i].label == label);
    }
    return ZKP_OK;
}

// the work of slot g; every path through it passes the same barriers.  A failure's message is the worker's g_err when this returns
// (run_on_slots reads it there): nothing between a failed step and the return -- barriers, drain, ~WsOrder, ~CtxScope -- calls fail().
int shard_job(ShardCall& c, size_t g) {
    CtxScope scope((int)g);
    int rc = scope.rc;
    std::unique_ptr<WsOrder> order;  // (behind `scope`: it goes before the context is left)
    ShardSlot& me = c.s[g];
    ShardPlan plan;
    auto step = [&](auto&& f) {
        if (rc != ZKP_OK) return;
        try {
            rc = f();
        } catch (...) {
            rc = on_exception();
        }
    };
    step([&] {
        plan = plan_shard(c.g, c.log_n, c.inverse, c.lin, c.lout, c.host != nullptr, c.coset != nullptr, g);
        return shard_setup(c, g, &order);
    });
    if (plan.phase_end.empty()) {  // no context or no plan: meet the others at the first barrier, where this verdict takes everyone out
        (void)c.bar.arrive(false);
        return rc;
    }
    bool alive = true;
    for (size_t p = 0, first = 0; alive && p < plan.phase_end.size(); first = plan.phase_end[p++]) {
        step([&] { return shard_phase(c, g, plan, first, plan.phase_end[p]); });
        alive = c.bar.arrive(rc == ZKP_OK);
    }
    if (!alive) {
        if (scope.rc == ZKP_OK) {  // drain
            if (me.xs) (void)hipStreamSynchronize(me.xs);
            (void)hipStreamSynchronize(me.main);
        }
        return rc != ZKP_OK ? rc : fail(ZKP_E_DEVICE, "another device slot failed");
    }
    if (c.host) {
        hipError_t e = hipMemcpyAsync(c.host + 4 * c.g.slab * g, me.x, sizeof(Fr) * c.g.slab, hipMemcpyDeviceToHost, me.main);
        if (e == hipSuccess) e = hipStreamSynchronize(me.main);
        if (e != hipSuccess) return fail(ZKP_E_DEVICE, hipGetErrorString(e));
    } else if (c.sync) {
        HIPCHK(hipStreamSynchronize(me.main));
    }
    return ZKP_OK;
}

int ntt_sharded_run(ShardCall& c) {
    const size_t W = (size_t)c.g.G;
    c.s.assign(W, ShardSlot());
    c.bar.n = W;
    {
        std::lock_guard<std::mutex> g(g_rt.mu);
        if (g_rt.slots.size() != W) return fail(ZKP_E_ARG, "the device slots changed during the call");
        for (const auto& o : g_rt.slots) c.devices.push_back(o->device);
    }
    const SlotResults r = run_on_slots(W, [&](size_t i) { return shard_job(c, i); });  // (a job never leaves the barriers: shard_job catches inside its steps)
    const std::vector<int>& rc = r.rc;
    const std::vector<std::string>& msg = r.msg;
    int first = -1;  // the slot that failed by itself, not the ones it took down
    for (size_t i = 0; i < W; i++)
        if (rc[i] != ZKP_OK && (first < 0 || msg[(size_t)first] == "another device slot failed")) first = (int)i;
    if (first >= 0) return fail(rc[(size_t)first], "device slot " + std::to_string(first) + ": " + msg[(size_t)first]);
    return ZKP_OK;
}

size_t runtime_slots() {
    std::lock_guard<std::mutex> g(g_rt.mu);
    return g_rt.slots.size();
}

}  // namespace

bool ntt_should_shard(unsigned log_n) {
    const unsigned min_log = (unsigned)knob_int(KNOB_NTT_SHARD_MIN_LOG);
    const size_t W = runtime_slots();
    ShardGeom g;
    return W > 1 && !(W & (W - 1)) && log_n >= min_log && shard_geometry(log_n, W, 0, &g).empty();
}

int ntt_fr_sharded_host(uint64_t* data, unsigned log_n, int inverse, const uint64_t* coset) {
    if (!data) return fail(ZKP_E_ARG, "data is null");
    size_t W = runtime_slots();
    if (W == 0) {
        ZCHK(zkp_init(-1));
        W = 1;
    }
    ShardCall c;
    ZCHK(shard_geom(log_n, W, 0, &c.g));
    c.log_n = log_n;
    c.inverse = inverse ? 1 : 0;
    c.lin = c.lout = ZKP_NTT_NATURAL;
    c.host = data;
    c.coset = coset;
    return ntt_sharded_run(c);
}

extern "C" {

int zkp_ntt_fr_sharded_geometry(unsigned log_n, unsigned slots, unsigned chunks, zkp_ntt_shard_geometry* out) try {
    if (!out) return fail(ZKP_E_ARG, "null argument");
    size_t W = slots ? slots : runtime_slots();
    if (W == 0) W = 1;
    ShardGeom g;
    ZCHK(shard_geom(log_n, W, chunks, &g));
    out->slots = (unsigned)g.G;
    out->log_n1 = g.l1;
    out->log_n2 = g.l2;
    out->chunks = (unsigned)g.C;
    out->r1 = (size_t)g.r1;
    out->r2 = (size_t)g.r2;
    out->cw = (size_t)g.cw;
    out->slab = (size_t)g.slab;
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_ntt_fr_sharded_dev(void* const* d_slabs, unsigned log_n, int inverse, int layout_in, int layout_out, unsigned chunks,
                           void* const* streams) try {
    if (!d_slabs) return fail(ZKP_E_ARG, "null argument");
    size_t W = runtime_slots();
    if (W == 0) {
        ZCHK(zkp_init(-1));
        W = 1;
    }
    const bool ok = (layout_in == ZKP_NTT_NATURAL && (layout_out == ZKP_NTT_K1SLAB || layout_out == ZKP_NTT_NATURAL)) ||
                    (layout_in == ZKP_NTT_COLUMNS && layout_out == ZKP_NTT_K1SLAB) ||
                    (layout_in == ZKP_NTT_K1SLAB && (layout_out == ZKP_NTT_NATURAL || layout_out == ZKP_NTT_COLUMNS));
    if (!ok) return fail(ZKP_E_ARG, "layout pair not supported: NATURAL -> K1SLAB | NATURAL, COLUMNS -> K1SLAB, K1SLAB -> NATURAL | COLUMNS");
    ShardCall c;
    ZCHK(shard_geom(log_n, W, chunks, &c.g));
    for (size_t g = 0; g < W; g++)
        if (!d_slabs[g]) return fail(ZKP_E_ARG, "null slab pointer");
    c.log_n = log_n;
    c.inverse = inverse ? 1 : 0;
    c.lin = layout_in;
    c.lout = layout_out;
    c.d_slabs = d_slabs;
    c.streams = streams;
    c.sync = streams == nullptr;
    return ntt_sharded_run(c);
} ZKP_CATCH_INT

int zkp_ntt_fr_sharded(uint64_t* data, unsigned log_n, int inverse, const uint64_t* coset) try {
    return ntt_fr_sharded_host(data, log_n, inverse, coset);
} ZKP_CATCH_INT

}  // extern "C"
