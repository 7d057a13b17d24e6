// msm_host.inc -- the MSM driver, included by api.hip inside its anonymous namespace.  msm_partial_batch: plan_msm (msm_plan.hpp)
// sizes the pass, an MsmPass walks the scalar ranges (sort, accumulate) and reduces the buckets, msm_host_tail finishes on the host.

#ifdef ZKP_MSM_CHECK  // diagnosis builds: wait for every kernel of the walk and say which one was reached
#define MSM_TRACE(stream, ridx, what) do { hipError_t e_ = hipStreamSynchronize(stream); fprintf(stderr, "ZKP_MSM_CHECK range %llu: %s done (%d)\n", (unsigned long long)(ridx), what, (int)e_); } while (0)
#else
#define MSM_TRACE(stream, ridx, what) do { } while (0)
#endif

// Host scalars fed range by range: the upload of range k+1 (copy stream) overlaps the kernels of range k (shared-bucket mode only:
// later ranges add into the same buckets).  Used by the host-pointer entry zkp_msm_g1.
struct MsmFeed {
    const uint64_t* h_scalars;  // n x 4 limbs on the host
    hipStream_t copy_stream;    // non-blocking
    hipEvent_t ev;
    MsmFeedRanges ranges;       // msm_feed_ranges
};

// What the accumulate of a range reads: one of plan.nbuf buffer sets, so that the sort of the next range can fill the other
struct RangeBuffers {
    uint32_t *sorted, *start, *perm;
    uint4* desc;                         // W x desc_cap (16-byte aligned first), then
    uint32_t *over, *over_b, *over_off;  // W x 2, W x over_cap, W x (over_cap + 1)
};

// One pass of the kernels over the plan's scalar ranges.  The workspaces are the slot's buffers (Ctx); grow() sizes them to the plan
// and names the parts carved out of them.
struct MsmPass {
    const MsmPlan& p;
    const zkp_bases* bases;
    const Fr* const* scalars;
    size_t count;
    const MsmFeed* feed;
    hipStream_t st, sst;  // accumulate + reduction; digits + sort (a second stream when ranges overlap)
    unsigned bits = 0;    // != 0: the bounded path (zkp_msm_g1_bits*): the digits kernels test every scalar against 2^bits
    Ctx& cx = ctx();
    const size_t W = p.g.nwin, nhi = p.sg.nhi;
    uint32_t *ptot, *pstart, *ghist, *gcur;  // counts = W x nchunk x nhi, then W x nhi, W x (nhi + 1), W x 256 size histogram, W x 256
    uint4* result_out;                       // pinned: W x c result points, then
    uint32_t* result_flags;                  // W flag words, then (bounded path)
    unsigned long long* violation;           // the scalar that broke the bound (msm_digits_bits_kernel), MSM_NO_VIOLATION: none
    RangeUpload up;                          // host feed: the uploader's job for the later ranges, joined when the pass ends

    std::array<std::tuple<const char*, DevBuf*, size_t>, 14> buffers() {
        const MsmSizes& b = p.bytes;
        return {{{"digits", &cx.digits, b.digits}, {"sorted", &cx.sorted, b.sorted}, {"counts", &cx.counts, b.counts},
                 {"entries", &cx.entries, b.entries}, {"start", &cx.start, b.start}, {"perm", &cx.perm, b.perm}, {"over", &cx.over, b.over},
                 {"pieces", &cx.pieces, b.pieces}, {"buckets", &cx.buckets, b.buckets}, {"parts", &cx.parts, b.parts},
                 {"pyr1", &cx.pyr1, b.pyr1}, {"odd0", &cx.odd0, b.odd0}, {"odd1", &cx.odd1, b.odd1}, {"result", &cx.result, b.result}}};
    }
    // The result points and flag words go straight to pinned host memory (5 KB over PCIe: a device-to-host copy would be one more
    // blit launch per MSM); the device `result` buffer holds the barrier counters of the last launch.
    int grow() {
        for (const auto& [name, buf, bytes] : buffers()) ZCHK(buf->ensure(bytes));
        ZCHK(cx.host_result.ensure(p.bytes.host_result + (bits ? 16 : 0), hipHostMallocPortable | hipHostMallocMapped));  // written by this slot's device
        ptot = cx.counts.get() + W * p.g.nchunk * nhi;
        pstart = ptot + W * nhi;
        ghist = pstart + W * (nhi + 1);
        gcur = ghist + W * 256;
        result_out = static_cast<uint4*>(cx.host_result.p);
        result_flags = reinterpret_cast<uint32_t*>(result_out + 16 * W * p.g.c);
        violation = reinterpret_cast<unsigned long long*>((reinterpret_cast<uintptr_t>(result_flags + W) + 7) & ~(uintptr_t)7);
        // (the previous pass of this slot was read before its entry returned: nothing on the device still writes here)
        if (bits) __atomic_store_n(violation, MSM_NO_VIOLATION, __ATOMIC_RELEASE);
        return ZKP_OK;
    }
    RangeBuffers range_buffers(size_t par) const {
        uint4* desc = reinterpret_cast<uint4*>(static_cast<char*>(cx.over.p) + par * p.over_bytes);
        uint32_t* over = reinterpret_cast<uint32_t*>(desc + W * p.desc_cap);
        return {cx.sorted.get() + par * W * p.g.n, cx.start.get() + par * W * (p.g.nb + 2), cx.perm.get() + par * W * p.g.nb, desc, over,
                over + 2 * W, over + 2 * W + W * p.over_cap};
    }
#ifdef ZKP_MSM_CHECK  // diagnosis builds: where every workspace lives, to place a faulting address
    void dump(size_t n) {
        static bool once = false;
        if (once) return;
        once = true;
        auto show = [](const char* name, const void* q, size_t bytes) {
            fprintf(stderr, "ZKP_MSM_CHECK %-10s %p .. %p (%zu bytes)\n", name, q, static_cast<const char*>(q) + bytes, bytes);
        };
        show("bases", bases->d_xy.p, (size_t)bases->n * 128 * std::max(bases->pre_planes, 1u));
        show("scalars", scalars[0], 32 * n);
        for (const auto& [name, buf, bytes] : buffers()) show(name, buf->p, buf->cap);
        show("host_res", cx.host_result.p, cx.host_result.cap);
        fprintf(stderr, "ZKP_MSM_CHECK geometry: n %zu range %llu first %llu rest %llu entries %llu nb %u nchunk %u over_cap %u desc_cap %u run_limit %u piece %u\n",
                n, (unsigned long long)p.range, (unsigned long long)p.lens[0], (unsigned long long)p.lens.back(), (unsigned long long)p.g.n,
                p.g.nb, p.g.nchunk, p.over_cap, p.desc_cap, p.g.run_limit, p.g.piece);
    }
#endif

    // Host feed, first range: uploaded by this thread; the later ones are handed to the slot's uploader thread first, which issues them
    // as soon as the first copy is in the stream (see Uploader)
    int feed_first_range() {
        Fr* const dst = const_cast<Fr*>(scalars[0]);
        if (p.lens.size() > 1) {
            while (cx.copy_events.size() < p.lens.size() - 1) {
                Event e;
                ZCHK(e.ensure(hipEventDisableTiming));
                cx.copy_events.push_back(std::move(e));
            }
            up.submit(uploader(cx.slot), std::vector<uint64_t>(p.lens.begin() + 1, p.lens.end()), p.lens[0],
                      [device = cx.device] { return hipSetDevice(device) == hipSuccess ? (int)ZKP_OK : (int)ZKP_E_DEVICE; },
                      [dst, f = *feed, evs = cx.copy_events.data()](size_t k, uint64_t o, uint64_t l) {
                          const bool ok = hipMemcpyAsync(dst + o, f.h_scalars + 4 * o, 32 * l, hipMemcpyHostToDevice, f.copy_stream) == hipSuccess &&
                                          hipEventRecord(evs[k], f.copy_stream) == hipSuccess;
                          return ok ? (int)ZKP_OK : (int)ZKP_E_DEVICE;
                      });
        }
        hipError_t e1 = hipMemcpyAsync(dst, feed->h_scalars, 32 * p.lens[0], hipMemcpyHostToDevice, feed->copy_stream);
        if (e1 == hipSuccess) e1 = hipEventRecord(feed->ev, feed->copy_stream);
        up.release(e1 == hipSuccess);
        HIPCHK(e1);
        return ZKP_OK;
    }

    // The scalar ranges in order.  With overlap the digits + sort of range r+1 run on `sst` under the accumulate of range r on `st`.
    int walk() {
        if (p.overlap) {  // the sort stream starts after whatever the caller enqueued on st (the scalars)
            ZCHK(cx.sort_stream.ensure(hipStreamNonBlocking));
            for (Event* e : {&cx.ev_sort[0], &cx.ev_sort[1], &cx.ev_acc[0], &cx.ev_acc[1], &cx.ev_begin}) ZCHK(e->ensure(hipEventDisableTiming));
            sst = cx.sort_stream;
            HIPCHK(hipEventRecord(cx.ev_begin, st));
            HIPCHK(hipStreamWaitEvent(sst, cx.ev_begin, 0));
        }
        for (size_t ridx = 0; ridx < p.lens.size(); ridx++) {
            const MsmRange r = range_geom(p, ridx);
            const size_t par = r.set;
            const RangeBuffers rb = range_buffers(par);
            if (p.overlap && ridx >= 2) HIPCHK(hipStreamWaitEvent(sst, cx.ev_acc[par], 0));  // range r-2 is done with this buffer set
            if (feed) {  // this range's scalars: host -> device on the copy stream, the kernels below wait for them
                if (ridx == 0)
                    ZCHK(feed_first_range());
                else if (!up.wait_issued(ridx))  // (host only: the GPU is busy with the ranges before)
                    return fail(ZKP_E_DEVICE, "upload of a scalar range failed");
                HIPCHK(hipStreamWaitEvent(sst, ridx == 0 ? feed->ev : cx.copy_events[ridx - 1], 0));
            }
            launch_sort(rb, r);
            if (p.overlap) {
                HIPCHK(hipEventRecord(cx.ev_sort[par], sst));
                HIPCHK(hipStreamWaitEvent(st, cx.ev_sort[par], 0));
            }
            {
                ProfScope ps("msm_accumulate", st, true);
                const AccLaunch a = acc_launch(p, r.g);
                launch_accumulate(rb, r, a);
                launch_combine(rb, r.g, a);
                MSM_TRACE(st, r.ridx, "combine");
                launch_fold(r.g);
            }
            if (p.overlap) HIPCHK(hipEventRecord(cx.ev_acc[par], st));
        }
        return ZKP_OK;
    }

    template <int TILE> void launch_partscatter(const MsmGeom& g) {
        hipLaunchKernelGGL(msm_partscatter_kernel<TILE>, dim3(g.nchunk, g.nwin), dim3(1024), p.ps_lds, sst,
                           cx.digits.get(), g, p.sg, cx.counts.get(), pstart, cx.entries.get());
    }
    // Digits and counting sort of range r (r.g.ns scalars from r.off)
    void launch_sort(const RangeBuffers& rb, const MsmRange& r) {
        const SortGeom& sg = p.sg;
        const MsmGeom& g = r.g;
        const SortLaunch sl = sort_launch(sg, g);
        {
            ProfScope ps("msm_digits", sst);
            DigitSources ds;  // digits laid out [msm][slice][scalar]: a shared-mode sort window is one msm (split planes: one half of one)
            for (size_t m = 0; m < count; m++) ds.scalars[m] = scalars[m] + r.off;
            const uint8_t* inf = bases->d_inf.p ? bases->d_inf.get() + r.off : nullptr;
            if (bits)  // indices in a violation count from the start of the vector: r.off
                hipLaunchKernelGGL(g.glv ? msm_digits_bits_kernel<true> : msm_digits_bits_kernel<false>, dim3(sl.digits_x, (unsigned)count),
                                   dim3(MSM_THREADS), 0, sst, ds, inf, g, p.nwin1, (uint32_t)bits, (uint64_t)r.off, violation, cx.digits.get());
            else
                hipLaunchKernelGGL(g.glv ? msm_digits_glv_kernel : msm_digits_kernel, dim3(sl.digits_x, (unsigned)count), dim3(MSM_THREADS), 0,
                                   sst, ds, inf, g, p.nwin1, cx.digits.get());
            MSM_TRACE(sst, r.ridx, "digits");
        }
        ProfScope ps("msm_sort", sst, true);
        hipLaunchKernelGGL(msm_parthist_kernel, dim3(g.nchunk, g.nwin), dim3(1024), 0, sst, cx.digits.get(), g, sg, cx.counts.get());
        MSM_TRACE(sst, r.ridx, "parthist");
        hipLaunchKernelGGL(msm_partprefix_kernel, dim3(sl.prefix_x, g.nwin), dim3(1024), 0, sst, cx.counts.get(), g, sg, ptot);
        hipLaunchKernelGGL(msm_partstart_kernel, dim3(g.nwin), dim3(64), 0, sst, ptot, sg, pstart, ghist, cx.result.get());
        MSM_TRACE(sst, r.ridx, "partprefix + partstart");
        switch (p.ps_tile) {
            case PS_TILE_SMALL: launch_partscatter<PS_TILE_SMALL>(g); break;
            case PS_TILE_MID: launch_partscatter<PS_TILE_MID>(g); break;
            default: launch_partscatter<PS_TILE_BIG>(g); break;
        }
        MSM_TRACE(sst, r.ridx, "partscatter");
        hipLaunchKernelGGL(msm_binsort_kernel, dim3(sg.nhi, g.nwin), dim3(1024), 0, sst, cx.entries.get(), g, sg, pstart, rb.start, rb.sorted, ghist);
        MSM_TRACE(sst, r.ridx, "binsort");
        hipLaunchKernelGGL(msm_rank_kernel, dim3(sl.rank_x, g.nwin), dim3(1024), 0, sst, rb.start, g, ghist, gcur, rb.perm);
        MSM_TRACE(sst, r.ridx, "rank");
        hipLaunchKernelGGL(msm_order_kernel, dim3(g.nwin), dim3(1024), 0, sst, rb.start, g, ghist, rb.perm, rb.over, rb.over_b, rb.over_off,
                           rb.desc, p.over_cap, p.desc_cap);
        MSM_TRACE(sst, r.ridx, "order");
    }

    // Accumulate the sorted range r into the buckets (a = acc_launch(p, r.g)); then launch_combine adds up the pieces of oversized
    // buckets and launch_fold the parts of split runs.  walk() calls the three in this order; the self-test hook of the reduction
    // (msm_reduce_selftest) calls the last two on bucket contents of its caller's.
    void launch_accumulate(const RangeBuffers& rb, const MsmRange& r, const AccLaunch& a) {
        const MsmGeom& g = r.g;
        const uint4* xy = static_cast<const uint4*>(bases->d_xy.p) + r.off * 8;
        uint4 *buckets = cx.buckets.get(), *pieces = cx.pieces.get(), *parts = cx.parts.get(), *carry = cx.pyr1.get();
        if (a.quad)
            hipLaunchKernelGGL(msm_accumulate_quad_kernel, dim3(a.grid), dim3(ACC_THREADS), 0, st, xy, rb.sorted, rb.start, rb.perm, rb.over, rb.desc,
                               p.desc_cap, a.bucket_blocks, a.extra_blocks, g, buckets, pieces, parts, clk_record(CLK_MSM_ACCUMULATE));
        else
            hipLaunchKernelGGL(msm_accumulate_kernel, dim3(a.grid), dim3(ACC_THREADS), 0, st, xy, rb.sorted, rb.start, rb.perm, rb.over, rb.desc,
                               p.desc_cap, a.bucket_blocks, a.extra_blocks, g, buckets, pieces, parts, carry, clk_record(CLK_MSM_ACCUMULATE));
        MSM_TRACE(st, r.ridx, "accumulate");
    }
    // One wave per oversized bucket adds its pieces up: into the bucket, or (g.more) into the hand-over array, which is pyr1
    void launch_combine(const RangeBuffers& rb, const MsmGeom& g, const AccLaunch& a) {
        hipLaunchKernelGGL(msm_combine_kernel, dim3(a.combine_x, g.nwin), dim3(64), 0, st, rb.over, rb.over_b,
                           rb.over_off, p.over_cap, p.desc_cap, g, cx.pieces.get(), cx.buckets.get(), cx.pyr1.get());
    }
    // buckets += parts, pairwise (the steps: plan_fold)
    void launch_fold(const MsmGeom& g) {
        for (uint32_t t = 0; t < g.split_log; t++)
            hipLaunchKernelGGL(p.fold[t].lane ? msm_fold_parts_lane_kernel : msm_fold_parts_kernel, dim3(p.fold[t].grid_x, p.fold[t].pairs),
                               dim3(MSM_THREADS), 0, st, cx.buckets.get(), cx.parts.get(), (uint64_t)g.nwin * g.nb, t);
    }

    // The weighted bucket sums: pyramid levels as their own launches, then the last levels (or only the gathering) in one launch
    // that writes the c result points and the flag word of every bucket set to pinned host memory
    void reduce() {
        const MsmGeom& g = p.g;
        const ReducePlan& red = p.red;
        for (size_t w = 0; w < W; w++) __atomic_store_n(result_flags + w, MSM_FLAG_PENDING, __ATOMIC_RELEASE);  // (the previous MSM's results were read before it returned)
        uint4* pyr[2] = {cx.buckets.get(), cx.pyr1.get()};
        uint4* odd[2] = {cx.odd0.get(), cx.odd1.get()};
        ProfScope ps("msm_bucket_reduce", st, true);
        for (uint32_t k = 0; k < red.nlevel; k++) {
            const PyrLaunch& v = red.level[k];
            const uint32_t l = v.level;
            hipLaunchKernelGGL(v.quad ? msm_pyramid_quad_kernel : msm_pyramid_kernel, dim3(v.grid_x, l + 1, g.nwin), dim3(MSM_THREADS), 0, st,
                               pyr[l & 1], pyr[(l + 1) & 1], odd[l & 1], odd[(l + 1) & 1], PyrLevel{l, v.half, g.nb, g.nwin});
        }
        if (red.tail_blocks) {
            // test hook (tests/test_gpu_parity.py): ask the barrier for one arrival more than there are workgroups, with a short
            // time-out -- the path a workgroup that never became resident would take: MSM_TAIL_TIMEOUT flag, ZKP_E_DEVICE
            const bool starve = knob_flag(KNOB_TEST_TAIL_STARVE);
            hipLaunchKernelGGL(msm_pyramid_tail_kernel, dim3(red.tail_blocks, g.nwin), dim3(red.tail_threads), 0, st, pyr[0], pyr[1], odd[0], odd[1],
                               red.nlevel, g.c, g.nb, cx.result.get(), result_out, result_flags, red.tail_blocks + (starve ? 1 : 0),
                               starve ? (1u << 12) : PYR_TAIL_SPIN_LIMIT);
        } else {  // every level already ran as its own launch: only the gathering is left
            const uint32_t fin = (g.c - 1) & 1;
            hipLaunchKernelGGL(msm_collect_kernel, dim3(g.nwin), dim3(64), 0, st, pyr[fin], pyr[fin ^ 1], odd[fin], g.nb, g.c, result_out,
                               result_flags);
        }
    }
};

// The host polls the result flags of the nwin bucket sets (MsmPlan::poll_result) or waits for the stream (poll_or_sync, dev_res.hpp)
int wait_msm_result(bool poll, size_t nwin, const uint32_t* flags, hipStream_t st) {
    ZCHK(poll_or_sync(poll && !knob_flag(KNOB_MSM_NO_POLL), st, [&] {
        for (size_t w = 0; w < nwin; w++)
            if (__atomic_load_n(flags + w, __ATOMIC_ACQUIRE) & MSM_FLAG_PENDING) return false;
        return true;
    }));
    for (size_t w = 0; w < nwin; w++)
        if (flags[w] & MSM_TAIL_TIMEOUT)
            return fail(ZKP_E_DEVICE, "bucket reduction: the workgroups of the last levels did not all become resident (device shared "
                                      "with another job?); no result was produced");
    return ZKP_OK;
}

// Serial tail on the host.  Per bucket set: V = S + sum_l 2^l U_l.  Per-window mode: total = sum_w 2^(c w) V_w, and every (w, l)
// lands on its own bit position c w + l, so ONE Horner chain over the positions does it with c W doublings.  Shared mode: the
// expanded bases already carry the 2^(c w) factors, total = V of the single bucket set.  Endomorphism-split planes (glv): an MSM has
// two bucket sets, total = V_1 + phi(V_2) with phi(X, Y, ZZ, ZZZ) = (beta X, Y, ZZ, ZZZ) -- the identity (ZZ = 0) stays the identity,
// and V_1 = +-phi(V_2) is the general add's doubling / cancelling case.
HXyzz glv_phi(HXyzz v) {
    static const HFq beta = HFq::load(GlvParams::BETA).to_mont();
    v.x = v.x * beta;
    return v;
}
void msm_host_tail(const uint32_t* host_res, size_t count, uint32_t wins_per_msm, uint32_t c, bool glv, HXyzz* out) {
    const auto t_tail0 = std::chrono::steady_clock::now();
    auto tail_set = [&](size_t m) {
        const uint32_t* res = host_res + m * wins_per_msm * c * 64;  // 64 words / point
        HXyzz total = HXyzz::infinity();
        for (int pos = (int)(wins_per_msm * c) - 1; pos >= 0; pos--) {
            total = total.dbl();
            const int w = pos / (int)c, l = pos % (int)c;
            const uint32_t* rw = res + (size_t)w * c * 64;
            if (l <= (int)c - 2) total = total.add(xyzz_from_internal(rw + (size_t)(1 + l) * 64));
            if (l == 0) total = total.add(xyzz_from_internal(rw));
        }
        return total;
    };
    auto tail = [&](size_t m) { out[m] = glv ? tail_set(2 * m).add(glv_phi(tail_set(2 * m + 1))) : tail_set(m); };
    if (count == 1)
        tail(0);
    else  // the tails of a batch are independent serial chains: spread over the resident host workers
        host_pool().run(std::function<void(size_t)>(tail), count);
    prof_host("msm_tail_host", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_tail0).count());
}

// out[m] = sum_i scalars[m][i] * bases[i] as extended-Jacobian points (host), for `count` scalar vectors of the same length over
// the same bases.  The vectors are stacked as extra windows of ONE pass through the kernels, so that a batch of small MSMs (the
// 3 + 1 + 3 + 2 commitments of a PLONK proof) fills the GPU and pays the latency-bound bucket reduction once.  With expanded bases
// (zkp_g1_bases_precompute) all windows of a scalar share one bucket set; with endomorphism-split planes
// (zkp_g1_bases_precompute_glv) every scalar vector is a batch of two over the same planes and out[m] = V_1 + phi(V_2).
// bits < MSM_BITS_WHOLE: the caller's bound on every canonical scalar.  The plan keeps the slices such scalars fill (plan_msm), the
// digits kernels check the bound, and a scalar that breaks it is ZKP_E_ARG with nothing written to `out`: the pass has run to its end by
// then (the violation arrives with the result flags, no launch and no wait of its own), so the workspaces serve the next call.
int msm_partial_batch(const zkp_bases* bases, const Fr* const* d_scalars, size_t count, size_t n, hipStream_t st, HXyzz* out,
                      const MsmFeed* feed = nullptr, unsigned bits = MSM_BITS_MAX) {
    MsmPlan p;
    if (const int rc = plan_msm({bases->n, bases->pre_c, bases->pre_planes, bases->pre_off, bases->pre_glv}, count, n, feed ? &feed->ranges : nullptr,
                                ctx().tail_max_waves, &p, bits))
        return fail(rc, p.error);
    const unsigned bound = bits < MSM_BITS_WHOLE ? bits : 0;
    if (p.lens.empty()) {
        for (size_t m = 0; m < count; m++) out[m] = HXyzz::infinity();
        return ZKP_OK;
    }
    MsmPass pass{p, bases, d_scalars, count, feed, st, st, bound};
    ZCHK(pass.grow());
#ifdef ZKP_MSM_CHECK
    pass.dump(n);
#endif
    const int walk_rc = pass.walk(), up_rc = pass.up.join();
    if (walk_rc != ZKP_OK || up_rc != ZKP_OK) {
        // an early return out of the walk can leave digits / sort kernels queued on the second stream that were never joined back
        // into st; the caller's WsOrder event covers st only, so drain them here before the workspaces can be handed to the next entry
        if (p.overlap) (void)hipStreamSynchronize(pass.sst);
        if (feed) (void)hipStreamSynchronize(feed->copy_stream);
        return walk_rc != ZKP_OK ? walk_rc : fail(ZKP_E_DEVICE, "upload of a scalar range failed");
    }
    HIPCHK(hipGetLastError());
    pass.reduce();
    HIPCHK(hipGetLastError());
#ifdef ZKP_MSM_CHECK
    {
        uint32_t chk[32];
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpyFromSymbol(chk, HIP_SYMBOL(g_msm_check), sizeof(chk)));
        for (int k = 0; k < 8; k++)
            if (chk[4 * k]) fprintf(stderr, "ZKP_MSM_CHECK class %d: %u violations, first (%u, %u)\n", k, chk[4 * k], chk[4 * k + 1], chk[4 * k + 2]);
    }
#endif
    if (count > 1 && !knob_flag(KNOB_POOL_NO_WARM)) host_pool().warm(std::chrono::microseconds(3000));  // the tails below run on the pool: wake it now
    ZCHK(wait_msm_result(p.poll_result, p.g.nwin, pass.result_flags, st));
    if (bound) {
        const unsigned long long v = __atomic_load_n(pass.violation, __ATOMIC_ACQUIRE);
        if (v != MSM_NO_VIOLATION)
            return fail(ZKP_E_ARG, "scalar " + std::to_string(v & 0xffffffffull) + " of vector " + std::to_string(v >> 32) + " is not below 2^" +
                                       std::to_string(bound) + " (the bound of the call)");
    }
    msm_host_tail(reinterpret_cast<const uint32_t*>(pass.result_out), count, p.g.shared ? 1u : p.nwin1, p.g.c, p.g.glv != 0, out);  // (the pool's threads are in no context)
    return ZKP_OK;
}

// Self-test hook (zkp_selftest_msm_sort_dev): the plan, the pass and the workspaces of msm_partial_batch, then launch_sort of ONE
// range and nothing else.  The range's sort outputs are filled with 0xFF first, so that a word no kernel owns is recognisable, and
// copied to the caller's buffers behind the sort.  out == nullptr: the geometry only, nothing touches the device.
int msm_sort_selftest(const zkp_bases* bases, const Fr* const* d_scalars, size_t count, size_t n, size_t range_index, hipStream_t st,
                      zkp_msm_sort_geometry* geom, const zkp_msm_sort_outputs* out, unsigned bits = MSM_BITS_MAX) {
    MsmPlan p;
    if (const int rc = plan_msm({bases->n, bases->pre_c, bases->pre_planes, bases->pre_off, bases->pre_glv}, count, n, nullptr, ctx().tail_max_waves, &p, bits))
        return fail(rc, p.error);
    if (range_index >= p.lens.size()) return fail(ZKP_E_ARG, "range index past the plan's scalar ranges");
    const MsmRange r = range_geom(p, range_index);
    const MsmGeom& g = r.g;
    const size_t W = g.nwin, wn = W * g.n;
    *geom = zkp_msm_sort_geometry{};
    geom->c = g.c, geom->nwin = g.nwin, geom->nb = g.nb, geom->nslice = g.nslice, geom->shared = g.shared, geom->glv = g.glv;
    geom->nchunk = g.nchunk, geom->lo_bits = p.sg.lo_bits, geom->nhi = p.sg.nhi, geom->run_limit = g.run_limit, geom->piece = g.piece;
    geom->over_cap = p.over_cap, geom->desc_cap = p.desc_cap, geom->ps_tile = (uint32_t)p.ps_tile;
    geom->nranges = (uint32_t)p.lens.size(), geom->range_index = (uint32_t)range_index;
    geom->n = g.n, geom->ns = g.ns, geom->chunk = g.chunk, geom->range_off = r.off, geom->range_len = r.len;
    std::memcpy(geom->off, g.off, sizeof(geom->off));
    static_assert(sizeof(geom->off) == sizeof(g.off), "zkp_msm_sort_geometry::off");
    const size_t words[ZKP_SORT_OUTPUTS] = {wn, 2 * wn, W * (p.sg.nhi + 1), W * 256, W * (g.nb + 2), wn, W * g.nb, 2 * W,
                                            W * p.over_cap, W * ((size_t)p.over_cap + 1), 4 * W * p.desc_cap};
    for (int k = 0; k < ZKP_SORT_OUTPUTS; k++) geom->out_words[k] = words[k];
    if (!out) return ZKP_OK;
    for (int k = 0; k < ZKP_SORT_OUTPUTS; k++) {
        if (!out->d_out[k]) return fail(ZKP_E_ARG, "null output buffer");
        if (out->words[k] < words[k]) return fail(ZKP_E_ARG, "output buffer too small (zkp_msm_sort_geometry::out_words)");
    }
    MsmPass pass{p, bases, d_scalars, count, nullptr, st, st, bits < MSM_BITS_WHOLE ? bits : 0u};  // (a scalar past the bound is not reported here)
    ZCHK(pass.grow());
    const RangeBuffers rb = pass.range_buffers(r.set);
    Ctx& cx = ctx();
    HIPCHK(hipMemsetAsync(rb.sorted, 0xFF, 4 * wn, st));
    HIPCHK(hipMemsetAsync(rb.start, 0xFF, 4 * W * (g.nb + 2), st));
    HIPCHK(hipMemsetAsync(rb.perm, 0xFF, 4 * W * g.nb, st));
    HIPCHK(hipMemsetAsync(rb.desc, 0xFF, p.over_bytes, st));  // desc, over, over_b, over_off of this buffer set
    HIPCHK(hipMemsetAsync(cx.entries.get(), 0xFF, 8 * wn, st));
    pass.launch_sort(rb, r);
    HIPCHK(hipGetLastError());
    const void* const src[ZKP_SORT_OUTPUTS] = {cx.digits.get(), cx.entries.get(), pass.pstart, pass.ghist, rb.start, rb.sorted, rb.perm,
                                               rb.over,         rb.over_b,        rb.over_off, rb.desc};
    for (int k = 0; k < ZKP_SORT_OUTPUTS; k++)
        if (words[k]) HIPCHK(hipMemcpyAsync(out->d_out[k], src[k], 4 * words[k], hipMemcpyDeviceToDevice, st));
    // the bounded digits kernel writes its violation word in the slot's pinned memory: be done with it before the next entry resets it
    if (pass.bits) HIPCHK(hipStreamSynchronize(st));
    return ZKP_OK;
}

// Self-test hook (zkp_selftest_msm_reduce_dev): what msm_partial_batch runs behind the accumulate -- launch_combine, launch_fold,
// reduce(), wait_msm_result -- on bucket contents of the caller's, in the slot's own workspaces.  The plan is put together from the
// pieces plan_msm uses (plan_fold, plan_reduce, acc_launch's combine grid); there are no bases, no scalars and no sort, so the hook does
// what the sort does for the reduction: it zeroes the barrier counters of the last-levels launch (msm_partstart_kernel in an MSM).
// Everything the reduction may read without having written it is filled with 0xFF bytes first.
int msm_reduce_selftest(const zkp_msm_reduce_io& in, hipStream_t st, zkp_msm_reduce_geometry* geom) {
    if (in.c < 2 || in.c > MSM_MAX_WINDOW_BITS) return fail(ZKP_E_ARG, "window width outside 2..24 bits");
    if (!in.nwin || in.nwin > 65535) return fail(ZKP_E_ARG, "bucket sets outside 1..65535");
    if (in.split_log > MSM_MAX_SPLIT_LOG) return fail(ZKP_E_ARG, "split_log above 2");
    const bool combine = in.d_over != nullptr;
    if (combine && (!in.over_cap || !in.desc_cap)) return fail(ZKP_E_ARG, "a combine block with over_cap or desc_cap 0");
    if (!combine && (in.resume || in.more)) return fail(ZKP_E_ARG, "resume / more without a combine block");
    Ctx& cx = ctx();
    MsmPlan p{};
    MsmGeom& g = p.g;
    g.c = in.c, g.nwin = in.nwin, g.nb = 1u << (in.c - 1), g.split_log = in.split_log;
    g.resume = in.resume ? 1u : 0u, g.more = in.more ? 1u : 0u;
    const size_t W = g.nwin, cap = W * g.nb, nparts = (1u << g.split_log) - 1;
    if (cap >= (1ull << 31)) return fail(ZKP_E_ARG, "nwin x 2^(c-1) >= 2^31");
    p.nwin1 = 1, p.nbuf = 1;
    p.over_cap = combine ? in.over_cap : 0u, p.desc_cap = combine ? in.desc_cap : 0u;
    if (combine && ((uint64_t)W * p.desc_cap >= (1ull << 24) || (uint64_t)W * p.over_cap >= (1ull << 24)))
        return fail(ZKP_E_ARG, "nwin x over_cap or nwin x desc_cap >= 2^24");
    p.over_bytes = ((4 * W * (2 + (size_t)p.over_cap + p.over_cap + 1) + 16 * W * (size_t)p.desc_cap) + 255) & ~(size_t)255;
    plan_fold(g.nwin, g.nb, g.split_log, p.fold);
    if (const int rc = plan_reduce(g.c, g.nwin, cx.tail_max_waves, &p.red, &p.error)) return fail(rc, p.error);
    const AccLaunch a = acc_launch(p, g);
    p.bytes = MsmSizes{};
    if (combine) p.bytes.over = p.over_bytes, p.bytes.pieces = 256 * W * (size_t)p.desc_cap;
    p.bytes.buckets = p.bytes.pyr1 = p.bytes.odd0 = p.bytes.odd1 = 256 * cap;
    p.bytes.parts = 256 * cap * nparts;
    p.bytes.result = 4 * PYR_BAR_STRIDE * W;
    p.bytes.host_result = 256 * W * g.c + 4 * W;

    *geom = zkp_msm_reduce_geometry{};
    geom->c = g.c, geom->nwin = g.nwin, geom->nb = g.nb, geom->split_log = g.split_log, geom->tail_max_waves = cx.tail_max_waves;
    geom->nlevel = p.red.nlevel, geom->tail_blocks = p.red.tail_blocks, geom->tail_threads = p.red.tail_threads;
    geom->combine_x = combine ? a.combine_x : 0u, geom->over_cap = p.over_cap, geom->desc_cap = p.desc_cap, geom->cap = cap;
    static_assert(sizeof(geom->level) / sizeof(geom->level[0]) == MSM_MAX_WINDOW_BITS, "zkp_msm_reduce_geometry::level");
    static_assert(sizeof(geom->fold) / sizeof(geom->fold[0]) == MSM_MAX_SPLIT_LOG, "zkp_msm_reduce_geometry::fold");
    for (uint32_t k = 0; k < p.red.nlevel; k++) geom->level[k] = {p.red.level[k].level, p.red.level[k].half, p.red.level[k].quad, p.red.level[k].grid_x};
    for (uint32_t t = 0; t < g.split_log; t++) geom->fold[t] = {p.fold[t].pairs, p.fold[t].lane, p.fold[t].grid_x};
    geom->bucket_words = geom->carry_words = 64 * cap, geom->parts_words = 64 * cap * nparts;
    geom->over_words = combine ? 2 * W : 0, geom->over_b_words = W * p.over_cap, geom->over_off_words = combine ? W * ((size_t)p.over_cap + 1) : 0;
    geom->pieces_words = 64 * W * (size_t)p.desc_cap, geom->result_words = 64 * W * g.c, geom->flag_words = W;
    if (!in.out_results) return ZKP_OK;

    auto short_of = [](const void* q, size_t have, size_t want) { return want && (!q || have < want); };
    if (short_of(in.d_buckets, in.buckets_words, geom->bucket_words) || short_of(in.d_parts, in.parts_words, geom->parts_words) ||
        short_of(in.out_results, in.out_results_words, geom->result_words) || short_of(in.out_flags, in.out_flags_words, geom->flag_words) ||
        (in.d_out_buckets && in.out_buckets_words < geom->bucket_words))
        return fail(ZKP_E_ARG, "null or too-small buffer (zkp_msm_reduce_geometry: the words of every buffer)");
    if (combine && (short_of(in.d_over, in.over_words, geom->over_words) || short_of(in.d_over_b, in.over_b_words, geom->over_b_words) ||
                    short_of(in.d_over_off, in.over_off_words, geom->over_off_words) || short_of(in.d_pieces, in.pieces_words, geom->pieces_words) ||
                    (g.resume && short_of(in.d_carry, in.carry_words, geom->carry_words)) ||
                    (g.more && short_of(in.d_out_carry, in.out_carry_words, geom->carry_words))))
        return fail(ZKP_E_ARG, "null or too-small buffer of the combine block (zkp_msm_reduce_geometry: the words of every buffer)");
    if (combine) {  // the kernel trusts the sort for these: candidates within over_cap, bucket ids 1..nb (its piece range it clamps itself)
        std::vector<uint32_t> over(2 * W), over_b(W * p.over_cap);
        HIPCHK(hipStreamSynchronize(st));
        HIPCHK(hipMemcpy(over.data(), in.d_over, 4 * over.size(), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(over_b.data(), in.d_over_b, 4 * over_b.size(), hipMemcpyDeviceToHost));
        for (size_t w = 0; w < W; w++) {
            if (over[2 * w] > p.over_cap) return fail(ZKP_E_ARG, "more oversized candidates than over_cap");
            for (uint32_t r = 0; r < over[2 * w]; r++)
                if (over_b[w * p.over_cap + r] < 1 || over_b[w * p.over_cap + r] > g.nb) return fail(ZKP_E_ARG, "bucket id of a candidate outside 1..2^(c-1)");
        }
    }

    MsmPass pass{p, nullptr, nullptr, 0, nullptr, st, st, 0u};
    ZCHK(pass.grow());
    const RangeBuffers rb = pass.range_buffers(0);
    for (DevBuf* b : {static_cast<DevBuf*>(&cx.buckets), static_cast<DevBuf*>(&cx.pyr1), static_cast<DevBuf*>(&cx.odd0), static_cast<DevBuf*>(&cx.odd1)})
        HIPCHK(hipMemsetAsync(b->p, 0xFF, b->cap, st));  // (buckets: a workspace larger than nwin sets keeps no stored point behind them)
    std::memset(cx.host_result.p, 0xFF, p.bytes.host_result);  // (nothing on the device writes here: the slot's previous entry has read its results)
    HIPCHK(hipMemsetAsync(cx.result.get(), 0, p.bytes.result, st));  // the barrier counters, one line per bucket set
    HIPCHK(hipMemcpyAsync(cx.buckets.get(), in.d_buckets, 256 * cap, hipMemcpyDeviceToDevice, st));
    if (nparts) HIPCHK(hipMemcpyAsync(cx.parts.get(), in.d_parts, 256 * cap * nparts, hipMemcpyDeviceToDevice, st));
    if (combine) {
        HIPCHK(hipMemcpyAsync(rb.over, in.d_over, 4 * geom->over_words, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(rb.over_b, in.d_over_b, 4 * geom->over_b_words, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(rb.over_off, in.d_over_off, 4 * geom->over_off_words, hipMemcpyDeviceToDevice, st));
        HIPCHK(hipMemcpyAsync(cx.pieces.get(), in.d_pieces, 4 * geom->pieces_words, hipMemcpyDeviceToDevice, st));
        if (g.resume) HIPCHK(hipMemcpyAsync(cx.pyr1.get(), in.d_carry, 256 * cap, hipMemcpyDeviceToDevice, st));
        pass.launch_combine(rb, g, a);
        HIPCHK(hipGetLastError());
        if (g.more) {  // the sums went to the hand-over array: there is nothing to fold or to reduce
            HIPCHK(hipMemcpyAsync(in.d_out_carry, cx.pyr1.get(), 256 * cap, hipMemcpyDeviceToDevice, st));
            if (in.d_out_buckets) HIPCHK(hipMemcpyAsync(in.d_out_buckets, cx.buckets.get(), 256 * cap, hipMemcpyDeviceToDevice, st));
            HIPCHK(hipStreamSynchronize(st));
            return ZKP_OK;
        }
        if (g.resume) HIPCHK(hipMemsetAsync(cx.pyr1.p, 0xFF, cx.pyr1.cap, st));  // the carry has been read: pyr1 is a pyramid buffer from here on
    }
    pass.launch_fold(g);
    HIPCHK(hipGetLastError());
    if (in.d_out_buckets) HIPCHK(hipMemcpyAsync(in.d_out_buckets, cx.buckets.get(), 256 * cap, hipMemcpyDeviceToDevice, st));
    pass.reduce();
    HIPCHK(hipGetLastError());
    const int rc = wait_msm_result(true, W, pass.result_flags, st);
    std::memcpy(in.out_flags, pass.result_flags, 4 * W);
    ZCHK(rc);
    std::memcpy(in.out_results, pass.result_out, 256 * W * g.c);
    return ZKP_OK;
}

int msm_partial(const zkp_bases* bases, const Fr* d_scalars, size_t n, hipStream_t st, HXyzz* out, unsigned bits = MSM_BITS_MAX) {
    return msm_partial_batch(bases, &d_scalars, 1, n, st, out, nullptr, bits);
}
