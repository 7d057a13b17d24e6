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
namespace {

struct ShardGeom {
    unsigned l1 = 0, l2 = 0, lw = 0;
    uint64_t G = 1, n1 = 0, n2 = 0, r1 = 0, r2 = 0, C = 1, cw = 0, slab = 0;
};

unsigned log2_exact(uint64_t v) {
    unsigned b = 0;
    while ((1ull << b) < v) b++;
    return b;
}

// the split is a function of (log_n, slots) only -- zkp_hip/dist.py: four_step_split is the same function, so that a vector left in
// the K1SLAB or COLUMNS layout by one transport can be read by the other
int shard_geometry(unsigned log_n, uint64_t G, unsigned chunks, ShardGeom* o) {
    if (G == 0 || (G & (G - 1)) || G > 64) return fail(ZKP_E_ARG, "the sharded transform needs a power-of-two number of device slots (at most 64)");
    if (log_n > 32) return fail(ZKP_E_ARG, "log_n > 32 (two-adicity of the field)");
    ShardGeom g;
    g.G = G;
    g.lw = log2_exact(G);
    g.l1 = std::max<unsigned>(std::min<unsigned>(8, (log_n + 1) / 2), g.lw);
    if (log_n < g.l1 + g.lw + 2)
        return fail(ZKP_E_ARG, "transform too small for " + std::to_string(G) + " slots: N2 / slots = 2^" + std::to_string((int)log_n - (int)g.l1 - (int)g.lw) +
                                   " columns per slot, at least four are needed (128-byte runs of the tile kernels)");
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
            return fail(ZKP_E_ARG, "chunks must be a power of two (at most 64) that leaves at least four columns per chunk: r2 = " + std::to_string(g.r2) +
                                       ", chunks = " + std::to_string(chunks) + " (it is part of the COLUMNS layout and is never adjusted silently)");
        g.C = chunks;
    }
    g.cw = g.r2 / g.C;
    g.slab = (1ull << log_n) / G;
    *o = g;
    return ZKP_OK;
}

// every thread arrives with its own verdict and leaves with the conjunction: a slot that failed takes the others out of the
// protocol at the same barrier, so nobody is left waiting for an event that will never be recorded
struct PhaseBarrier {
    std::mutex mu;
    std::condition_variable cv;
    size_t n = 1, arrived = 0;
    uint64_t gen = 0;
    bool ok = true;
    bool arrive(bool mine) {
        std::unique_lock<std::mutex> lk(mu);
        ok = ok && mine;
        if (++arrived == n) {
            arrived = 0;
            gen++;
            cv.notify_all();
        } else {
            const uint64_t g0 = gen;
            cv.wait(lk, [&] { return gen != g0; });
        }
        return ok;
    }
};

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

enum { SH_EV_PER_CHUNK = 3, SH_EV_EXTRA = 3 };  // SEND1(q), RECV1(q), SEND2(q); RECV2, SEND3, RECV3

// the work of slot g; every path through it passes the same barriers
int shard_job(ShardCall& c, size_t g, std::string* msg) {
    const ShardGeom& G = c.g;
    const uint64_t C = G.C, cw = G.cw, r1 = G.r1, r2 = G.r2, n1 = G.n1, n2 = G.n2, W = G.G;
    const uint64_t blk = r1 * cw, chunk = W * blk;  // one peer's block of one chunk; one chunk = the matrix [N1][cw]
    const unsigned lcw = log2_exact(cw), lC = log2_exact(C), lr1 = log2_exact(r1), lr2 = log2_exact(r2), lW = G.lw;
    auto SEND1 = [&](uint64_t q) { return (size_t)q; };
    auto RECV1 = [&](uint64_t q) { return (size_t)(C + q); };
    auto SEND2 = [&](uint64_t q) { return (size_t)(2 * C + q); };
    const size_t RECV2 = (size_t)(3 * C), SEND3 = RECV2 + 1, RECV3 = RECV2 + 2;

    CtxScope scope((int)g);
    int rc = scope.rc;
    if (rc != ZKP_OK) *msg = g_err;
    ShardSlot& me = c.s[g];
    struct Order {  // WsOrder, once the context is entered
        WsOrder* w = nullptr;
        ~Order() { delete w; }
    } order;
    auto step = [&](const std::function<int()>& f) -> bool {
        if (rc == ZKP_OK) {
            try {
                rc = f();
            } catch (...) {
                rc = on_exception();
            }
            if (rc != ZKP_OK) *msg = g_err;
        }
        return c.bar.arrive(rc == ZKP_OK);
    };
    auto wait_ev = [&](hipStream_t st, size_t p, size_t which) -> int {
        HIPCHK(hipStreamWaitEvent(st, c.s[p].ev[which], 0));
        return ZKP_OK;
    };
    auto record = [&](size_t which, hipStream_t st) -> int {
        HIPCHK(hipEventRecord(me.ev[which], st));
        return ZKP_OK;
    };
    auto peer = [&](uint64_t i) { return (size_t)((g + i) % W); };  // every slot starts with another partner
    // B_g[q][p] <- A_p[q][g] (or the other way round: the same block arithmetic serves both exchanges)
    auto pull_chunk = [&](uint64_t q, bool into_b, const std::function<int(size_t)>& before) -> int {
        for (uint64_t i = 0; i < W; i++) {
            const size_t p = peer(i);
            ZCHK(before(p));
            Fr* dst = (into_b ? me.b : me.a) + q * chunk + p * blk;
            const Fr* src = (into_b ? c.s[p].a : c.s[p].b) + q * chunk + g * blk;
            ZCHK(peer_copy(dst, me.device, src, c.s[p].device, sizeof(Fr) * blk, me.xs));
        }
        return ZKP_OK;
    };
    auto drain = [&]() {
        if (scope.rc == ZKP_OK) {
            if (me.xs) (void)hipStreamSynchronize(me.xs);
            (void)hipStreamSynchronize(me.main);
        }
    };
    const NttRemap gathered = [&] {  // logical n2 = (p, q, c) of row j at [q][p][j][c]
        NttRemap r;
        std::memset(&r, 0, sizeof r);
        r.on = 1;
        r.lo_bits = lcw;
        r.mid_bits = lC;
        r.mid_stride = chunk;
        r.hi_stride = blk;
        r.batch_stride = cw;
        return r;
    }();

    // ---- setup: buffers, streams, events, peer access; publish them to the other slots
    if (!step([&]() -> int {
            Ctx& cx = ctx();
            me.device = cx.device;
            me.main = c.streams ? reinterpret_cast<hipStream_t>(c.streams[g]) : (g_rt.multi ? cx.stream : nullptr);
            if (!c.streams && !c.host) HIPCHK(hipDeviceSynchronize());  // the slab's producer may be any stream of this device
            order.w = new WsOrder(me.main);
            const size_t bytes = sizeof(Fr) * G.slab;
            ZCHK(cx.xchg_a.ensure(bytes));
            ZCHK(cx.xchg_b.ensure(bytes));
            ZCHK(cx.xstream.ensure(hipStreamNonBlocking));
            const size_t nev = (size_t)(SH_EV_PER_CHUNK * C + SH_EV_EXTRA);
            while (cx.xev.size() < nev) {
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
                if (c.coset && !c.inverse) ZCHK(launch_coset_scale(me.x, G.slab, G.slab * g, c.log_n, 0, c.coset, me.main));
            } else {
                me.x = reinterpret_cast<Fr*>(c.d_slabs[g]);
            }
            return ZKP_OK;
        })) {
        drain();
        return rc != ZKP_OK ? rc : fail(ZKP_E_DEVICE, "another device slot failed");
    }
    bool alive = true;
    const bool flow_f = c.lin != ZKP_NTT_K1SLAB;
    if (flow_f) {
        const bool nat_in = c.lin == ZKP_NTT_NATURAL, nat_out = c.lout == ZKP_NTT_NATURAL;
        if (nat_in) {
            alive = step([&]() -> int {
                ProfScope ps("ntt_sharded_pack", me.main);
                for (uint64_t q = 0; q < C; q++) {
                    PermuteSpec sp;
                    std::memset(&sp, 0, sizeof sp);
                    sp.bits[1] = lW; sp.in_stride[1] = r2; sp.out_stride[1] = blk;   // h
                    sp.bits[2] = lr1; sp.in_stride[2] = n2; sp.out_stride[2] = cw;   // j
                    sp.bits[3] = lcw; sp.in_stride[3] = 1; sp.out_stride[3] = 1;     // c
                    ZCHK(launch_permute(me.x + q * cw, me.a + q * chunk, sp, me.main));
                    ZCHK(record(SEND1(q), me.main));
                }
                return ZKP_OK;
            });
            if (alive)
                alive = step([&]() -> int {
                    for (uint64_t q = 0; q < C; q++) {
                        ZCHK(pull_chunk(q, true, [&](size_t p) { return wait_ev(me.xs, p, SEND1(q)); }));
                        ZCHK(record(RECV1(q), me.xs));
                    }
                    return ZKP_OK;
                });
        }
        if (alive)
            alive = step([&]() -> int {
                ProfScope ps("ntt_sharded_columns", me.main);
                for (uint64_t q = 0; q < C; q++) {
                    if (nat_in) ZCHK(wait_ev(me.main, g, RECV1(q)));
                    ZCHK(run_ntt_axis0<Fr>((nat_in ? me.b : me.x) + q * chunk, me.b + q * chunk, G.l1, (size_t)cw, c.inverse, c.log_n,
                                           g * r2 + q * cw, me.main));
                    ZCHK(record(SEND2(q), me.main));
                }
                return ZKP_OK;
            });
        if (alive)
            alive = step([&]() -> int {
                for (uint64_t q = 0; q < C; q++) {
                    if (nat_in)  // A[q] is the source of everybody's first pull of this chunk
                        for (uint64_t i = 0; i < W; i++) ZCHK(wait_ev(me.xs, peer(i), RECV1(q)));
                    ZCHK(pull_chunk(q, false, [&](size_t p) { return wait_ev(me.xs, p, SEND2(q)); }));
                }
                ZCHK(record(RECV2, me.xs));
                ProfScope ps("ntt_sharded_exchange_wait", me.main);
                return wait_ev(me.main, g, RECV2);
            });
        if (alive)
            alive = step([&]() -> int {
                if (nat_out)  // the row transforms write B: not before everyone's second pull is through with it
                    for (uint64_t i = 0; i < W; i++) ZCHK(wait_ev(me.main, peer(i), RECV2));
                NttIo io;
                io.in_remap = &gathered;
                NttRemap packed;  // NATURAL out: output k2 = (h, c) of row j goes to B[h][j][c], the send block of slot h
                std::memset(&packed, 0, sizeof packed);
                packed.on = 1;
                packed.lo_bits = lr2;
                packed.hi_stride = r1 * r2;
                packed.batch_stride = r2;
                if (nat_out) io.out_remap = &packed;
                {
                    ProfScope ps("ntt_sharded_rows", me.main);
                    ZCHK(run_ntt<Fr>(me.a, nat_out ? me.b : me.x, G.l2, (size_t)r1, c.inverse, nullptr, me.main, &io));
                }
                if (nat_out) return record(SEND3, me.main);
                for (uint64_t i = 0; i < W; i++) ZCHK(wait_ev(me.main, peer(i), RECV2));  // B stays a source until then
                return ZKP_OK;
            });
        if (alive && nat_out) {
            alive = step([&]() -> int {
                for (uint64_t i = 0; i < W; i++) {
                    const size_t p = peer(i);
                    ZCHK(wait_ev(me.xs, p, SEND3));
                    ZCHK(peer_copy(me.a + p * r1 * r2, me.device, c.s[p].b + g * r1 * r2, c.s[p].device, sizeof(Fr) * r1 * r2, me.xs));
                }
                ZCHK(record(RECV3, me.xs));
                {
                    ProfScope ps("ntt_sharded_exchange_wait", me.main);
                    ZCHK(wait_ev(me.main, g, RECV3));
                }
                ProfScope ps("ntt_sharded_unpack", me.main);
                PermuteSpec sp;  // A[p][j][c] -> x[c][p r1 + j]: slot g's natural slab is k2 in [g r2, (g+1) r2), k = k1 + N1 k2
                std::memset(&sp, 0, sizeof sp);
                sp.bits[1] = lr2; sp.in_stride[1] = 1; sp.out_stride[1] = n1;        // c
                sp.bits[2] = lW; sp.in_stride[2] = r1 * r2; sp.out_stride[2] = r1;   // p
                sp.bits[3] = lr1; sp.in_stride[3] = r2; sp.out_stride[3] = 1;        // j
                ZCHK(launch_permute(me.a, me.x, sp, me.main));
                if (c.coset && c.inverse) ZCHK(launch_coset_scale(me.x, G.slab, G.slab * g, c.log_n, 1, c.coset, me.main));
                return ZKP_OK;
            });
            if (alive)
                alive = step([&]() -> int {
                    for (uint64_t i = 0; i < W; i++) ZCHK(wait_ev(me.main, peer(i), RECV3));
                    return ZKP_OK;
                });
        }
    } else {
        const bool cols_out = c.lout == ZKP_NTT_COLUMNS;
        alive = step([&]() -> int {
            NttIo io;
            io.out_remap = &gathered;  // output n2 = (h, q, c) of row j goes to A[q][h][j][c]
            io.tw_log_n = c.log_n;
            io.tw_row0 = g * r1;
            {
                ProfScope ps("ntt_sharded_rows", me.main);
                ZCHK(run_ntt<Fr>(me.x, me.a, G.l2, (size_t)r1, c.inverse, nullptr, me.main, &io));
            }
            return record(SEND1(0), me.main);
        });
        if (alive)
            alive = step([&]() -> int {
                for (uint64_t q = 0; q < C; q++) {
                    ZCHK(pull_chunk(q, true, [&](size_t p) { return wait_ev(me.xs, p, SEND1(0)); }));
                    ZCHK(record(RECV1(q), me.xs));
                }
                ProfScope ps("ntt_sharded_columns", me.main);
                for (uint64_t q = 0; q < C; q++) {
                    ZCHK(wait_ev(me.main, g, RECV1(q)));
                    ZCHK(run_ntt_axis0<Fr>(me.b + q * chunk, (cols_out ? me.x : me.b) + q * chunk, G.l1, (size_t)cw, c.inverse, 0, 0, me.main));
                    if (!cols_out) ZCHK(record(SEND2(q), me.main));
                }
                return ZKP_OK;
            });
        if (alive && cols_out)
            alive = step([&]() -> int {  // A stays the source of the others' pulls until their events
                for (uint64_t q = 0; q < C; q++)
                    for (uint64_t i = 0; i < W; i++) ZCHK(wait_ev(me.main, peer(i), RECV1(q)));
                return ZKP_OK;
            });
        if (alive && !cols_out) {
            alive = step([&]() -> int {
                for (uint64_t q = 0; q < C; q++) {
                    for (uint64_t i = 0; i < W; i++) ZCHK(wait_ev(me.xs, peer(i), RECV1(q)));
                    ZCHK(pull_chunk(q, false, [&](size_t p) { return wait_ev(me.xs, p, SEND2(q)); }));
                }
                ZCHK(record(RECV2, me.xs));
                {
                    ProfScope ps("ntt_sharded_exchange_wait", me.main);
                    ZCHK(wait_ev(me.main, g, RECV2));
                }
                ProfScope ps("ntt_sharded_unpack", me.main);
                PermuteSpec sp;  // x[j][p][q][c] = A[q][p][j][c]
                std::memset(&sp, 0, sizeof sp);
                sp.bits[0] = lC; sp.in_stride[0] = chunk; sp.out_stride[0] = cw;     // q
                sp.bits[1] = lW; sp.in_stride[1] = blk; sp.out_stride[1] = r2;       // p
                sp.bits[2] = lr1; sp.in_stride[2] = cw; sp.out_stride[2] = n2;       // j
                sp.bits[3] = lcw; sp.in_stride[3] = 1; sp.out_stride[3] = 1;         // c
                return launch_permute(me.a, me.x, sp, me.main);
            });
            if (alive)
                alive = step([&]() -> int {
                    for (uint64_t i = 0; i < W; i++) ZCHK(wait_ev(me.main, peer(i), RECV2));
                    return ZKP_OK;
                });
        }
    }
    if (!alive) {
        drain();
        return rc != ZKP_OK ? rc : fail(ZKP_E_DEVICE, "another device slot failed");
    }
    if (c.host) {
        hipError_t e = hipMemcpyAsync(c.host + 4 * G.slab * g, me.x, sizeof(Fr) * G.slab, hipMemcpyDeviceToHost, me.main);
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
    std::vector<int> rc(W, ZKP_OK);
    std::vector<std::string> msg(W);
    std::vector<std::function<void()>> jobs(W);
    for (size_t i = 0; i < W; i++)
        jobs[i] = [&, i] {
            try {
                rc[i] = shard_job(c, i, &msg[i]);
            } catch (...) {  // (a job must not leave the barriers: shard_job catches inside its steps)
                rc[i] = on_exception();
                msg[i] = g_err;
            }
            if (rc[i] != ZKP_OK && msg[i].empty()) msg[i] = g_err;
        };
    g_workers.run(jobs);
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
    return W > 1 && !(W & (W - 1)) && log_n >= min_log && shard_geometry(log_n, W, 0, &g) == ZKP_OK;
}

int ntt_fr_sharded_host(uint64_t* data, unsigned log_n, int inverse, const uint64_t* coset) {
    if (!data) return fail(ZKP_E_ARG, "data is null");
    size_t W = runtime_slots();
    if (W == 0) {
        ZCHK(zkp_init(-1));
        W = 1;
    }
    ShardCall c;
    ZCHK(shard_geometry(log_n, W, 0, &c.g));
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
    ZCHK(shard_geometry(log_n, W, chunks, &g));
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
    ZCHK(shard_geometry(log_n, W, chunks, &c.g));
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
