// ntt_host.inc -- the single-device NTT driver (run_ntt, run_ntt_axis0): per-field state, the device tables of a plan (its shape is
// ntt_plan.hpp's), the coset table cache, the two launchers.  Included by api.hip above Ctx, which holds one NttState per field.

template <class F> struct HostField;  // host <-> device field views
template <> struct HostField<Fr> {
    typedef HFr H;
    static Fr dev(const HFr& x) { Fr r; std::memcpy(r.l, x.l, 32); return r; }  // Montgomery on both sides
    // twiddle form of the kernels (fr29.hpp): w * 2^261 mod r sliced into 29-bit limbs
    static Fr29 tw(const HFr& x) {
        HFr y = x;
        for (int i = 0; i < 5; i++) y = y.dbl();
        Fr29 r;
        for (int i = 0; i < 9; i++) {
            const int bit = 29 * i, w = bit >> 6, sh = bit & 63;
            unsigned __int128 v = y.l[w];
            if (w + 1 < 4) v |= (unsigned __int128)y.l[w + 1] << 64;
            r.l[i] = (uint32_t)(v >> sh) & MASK29;
        }
        return r;
    }
    static HFr root(unsigned log_n) { return fr_root_of_unity(log_n); }
    static constexpr int CLK = CLK_NTT_FR;  // clock record of the pass kernels; kClkNames[CLK] is their profile label
};
template <> struct HostField<Gl> {
    typedef HGl H;
    static Gl dev(const HGl& x) { return Gl{x.from_mont().l[0]}; }  // device twiddles are canonical (ff.hpp)
    static Gl tw(const HGl& x) { return dev(x); }
    static HGl root(unsigned log_n) { return gl_root_of_unity(log_n); }
    static constexpr int CLK = CLK_NTT_GL;
};

// The device tables of one (log_n, direction, allow_wide): what its shape asks for
template <class F>
struct NttPlan {
    typedef typename NttOps<F>::W W;
    NttShape shape;
    const W* tw[4] = {nullptr, nullptr, nullptr, nullptr};  // radix twiddles of pass p (NttState::radix)
    const W* direct[3] = {nullptr, nullptr, nullptr};      // NttStridedShape::direct_len != 0 (NttState::powers)
    // the two-level table of omega_N; inverse plans: inter_lo times 1/n as well.  Pass 0 multiplies every element by one inter-pass twiddle
    // anyway, so reading it from that table applies the 1/n for free (no scaling product at the store of the last pass)
    TypedBuf<W> inter_lo, inter_hi, inter_lo_ninv;
    // pass 0's inter-pass twiddles as a matrix shaped like the data (pass0_uses_matrix); [1] = times 1/n.  Built on first use.
    TypedBuf<F> tw_matrix[2];
    typename HostField<F>::H n_inv;
};

// Everything the driver caches for one field on one device slot (Ctx)
template <class F>
struct NttState {
    typedef std::map<std::pair<unsigned, int>, DevBuf> PowTables;  // (k, inverse) -> powers of the 2^k-th root of unity
    PowTables radix;   // omega^j, j < 2^(k-1): the butterflies of a radix-2^k pass
    PowTables powers;  // omega^e, e < 2^k: direct inter-pass tables (get_plan, run_ntt_axis0)
    std::map<std::pair<unsigned, int>, NttPlan<F>> plans;  // (log_n, inverse | allow_wide << 1)
    // a few (size, direction, coset) tables: a PLONK proof alternates forward and inverse transforms on the 4n coset, and a
    // single entry was rebuilt four times per proof (115 us of pow_table launches)
    static constexpr int COSET_WAYS = 8;
    struct Coset {
        struct Key { unsigned log_n; int inverse; uint64_t g[4], c[4]; } key = {};  // the table c * g^e (g inverted when inverse), e < 2^log_n
        bool valid = false;
        TypedBuf<typename NttOps<F>::W> lo, hi;  // grow-only
        uint32_t h = 0;
    } coset[COSET_WAYS];
    unsigned coset_victim = 0;
};
template <class F> NttState<F>& ntt_state();  // of the current context; with ntt_scratch and clk_record defined below Ctx
DevBuf& ntt_scratch();
ClkRec* clk_record(int which);

template <class F>
int make_pow_table(const typename HostField<F>::H& base, const typename HostField<F>::H& c, uint32_t shift, uint32_t count, typename NttOps<F>::W* out, hipStream_t st) {
    hipLaunchKernelGGL(pow_table_kernel<F>, dim3((count + 255) / 256), dim3(256), 0, st, HostField<F>::dev(base),
                       HostField<F>::dev(c), shift, count, out);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

// The table of omega^e, e < count, omega = the 2^k-th root of unity (inverted for inverse transforms), found in `cache` or built.  It is
// shared by later calls on any stream: filled and drained before it is published, and also on a failure, before the table is freed.
template <class F>
int cached_pow_table(typename NttState<F>::PowTables& cache, unsigned k, int inverse, uint32_t count, const typename NttOps<F>::W** out, hipStream_t st) {
    typedef typename NttOps<F>::W W;
    const auto key = std::make_pair(k, inverse);
    auto it = cache.find(key);
    if (it == cache.end()) {
        typename HostField<F>::H w = HostField<F>::root(k);
        if (inverse) w = w.inverse();
        DevBuf tab;
        ZCHK(tab.ensure(sizeof(W) * count));
        int rc = make_pow_table<F>(w, HostField<F>::H::one(), 0, count, static_cast<W*>(tab.p), st);
        const hipError_t e = hipStreamSynchronize(st);
        if (rc == ZKP_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(st): ");
        if (rc != ZKP_OK) (void)hipGetLastError();
        ZCHK(rc);
        it = cache.emplace(key, std::move(tab)).first;
    }
    *out = static_cast<const W*>(it->second.p);
    return ZKP_OK;
}

template <class H>
H inv_pow2(unsigned k) { return H::from_u64(2).inverse().pow_u64(k); }  // 1 / 2^k

template <class F>
int get_plan(unsigned log_n, int inverse, bool allow_wide, NttPlan<F>** out, hipStream_t st) {
    typedef typename HostField<F>::H H;
    typedef typename NttOps<F>::W W;
    NttState<F>& state = ntt_state<F>();
    const auto key = std::make_pair(log_n, inverse | (allow_wide ? 2 : 0));
    auto it = state.plans.find(key);
    if (it == state.plans.end()) {
        NttPlan<F> pl;
        const NttShape& s = pl.shape = plan_ntt<NttOps<F>>(log_n, inverse, allow_wide, knob_flag(KNOB_NTT_NO_WIDE_PASS));
        pl.n_inv = inv_pow2<H>(log_n);
        for (int p = 0; p < s.passes; p++)
            ZCHK(cached_pow_table<F>(state.radix, (unsigned)s.r[p], inverse, 1u << (s.r[p] - 1), &pl.tw[p], st));
        for (int p = 1; p + 1 < s.passes; p++)
            if (s.strided[p].direct_len)  // omega_M^e, M = n >> log_outer
                ZCHK(cached_pow_table<F>(state.powers, log_n - s.strided[p].log_outer, inverse, (uint32_t)s.strided[p].direct_len, &pl.direct[p], st));
        if (s.passes > 1) {
            H w = HostField<F>::root(log_n);
            if (inverse) w = w.inverse();
            auto fill = [&](TypedBuf<W>& t, const H& c, uint32_t shift, uint32_t count) -> int {
                ZCHK(t.ensure(sizeof(W) * count));
                return make_pow_table<F>(w, c, shift, count, t.get(), st);
            };
            int rc = fill(pl.inter_lo, H::one(), 0, s.nlo);
            if (rc == ZKP_OK) rc = fill(pl.inter_hi, H::one(), s.h, s.nhi);
            if (rc == ZKP_OK && s.lo_ninv) rc = fill(pl.inter_lo_ninv, pl.n_inv, 0, s.nlo);
            // a plan that fails half-way is not cached, and `pl` gives back what it had allocated: the kernels filling the
            // tables may still be queued on st, so drain it first
            const hipError_t e = hipStreamSynchronize(st);
            if (rc == ZKP_OK && e != hipSuccess) rc = hip_fail(e, "hipStreamSynchronize(st): ");
            if (rc != ZKP_OK) (void)hipGetLastError();
            ZCHK(rc);
        }
        it = state.plans.emplace(key, std::move(pl)).first;
    }
    *out = &it->second;
    return ZKP_OK;
}

// The pass-0 twiddle matrix of a plan (times 1/n when ninv), made from the two-level tables on first use and held until zkp_shutdown.
// When the device has no room for it *out is null and the transform keeps the two-level tables instead of failing.  It is published in
// the cached plan only once it is filled: a failed fill must not leave a table of garbage behind for every later transform of this size.
template <class F>
int pass0_matrix(NttPlan<F>& pl, bool ninv, hipStream_t st, const F** out) {
    TypedBuf<F>& mat = pl.tw_matrix[ninv ? 1 : 0];
    if (!mat.p) {
        const uint64_t n = 1ull << pl.shape.log_n;
        const PowTab<F> inter = {(ninv ? pl.inter_lo_ninv : pl.inter_lo).get(), pl.inter_hi.get(), pl.shape.h};
        TypedBuf<F> fresh;
        if (hipMalloc(&fresh.p, sizeof(F) * n) != hipSuccess) {  // (not ensure: that would set the error message of a call that succeeds)
            (void)hipGetLastError();
        } else {
            hipLaunchKernelGGL(twiddle_matrix_kernel<F>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, inter, n, pl.shape.strided[0].inner, fresh.get());
            hipError_t fe = hipGetLastError();
            if (fe == hipSuccess) fe = hipStreamSynchronize(st);  // shared by later calls on any stream
            if (fe != hipSuccess) return fail(ZKP_E_DEVICE, std::string("twiddle matrix: ") + hipGetErrorString(fe));
            fresh.cap = sizeof(F) * n;
            mat = std::move(fresh);
        }
    }
    *out = mat.get();
    return ZKP_OK;
}

// two-level table of c * g^idx, idx < 2^log_n
template <class F>
int get_coset_tables(unsigned log_n, int inverse, const uint64_t* coset, const typename HostField<F>::H& c,
                     PowTab<F>* out, hipStream_t st) {
    typedef typename HostField<F>::H H;
    typedef typename NttOps<F>::W W;
    constexpr int WAYS = NttState<F>::COSET_WAYS;
    NttState<F>& state = ntt_state<F>();
    typename NttState<F>::Coset* ways = state.coset;
    typename NttState<F>::Coset::Key key = {log_n, inverse, {0, 0, 0, 0}, {0, 0, 0, 0}};
    std::memcpy(key.g, coset, sizeof(H));
    std::memcpy(key.c, c.l, sizeof(H));
    int way = -1, unused = -1;
    for (int i = WAYS - 1; i >= 0; i--) {
        if (ways[i].valid && std::memcmp(&ways[i].key, &key, sizeof key) == 0) way = i;
        if (!ways[i].valid) unused = i;
    }
    const bool hit = way >= 0;
    // a miss takes the first unused entry, else round-robin (tables still in use by enqueued kernels are rewritten in stream order)
    if (!hit) way = unused >= 0 ? unused : (int)(state.coset_victim++ % WAYS);
    auto& cc = ways[way];
    if (!hit) {
        cc.valid = false;
        const uint32_t h = (log_n + 1) / 2, nlo = 1u << h, nhi = 1u << (log_n - h);
        // a failing ensure leaves an empty (invalid, capacity 0) entry behind, never a dangling pointer with a stale capacity
        ZCHK(cc.lo.ensure(sizeof(W) * nlo));
        ZCHK(cc.hi.ensure(sizeof(W) * nhi));
        H g = H::load(coset);
        if (inverse) g = g.inverse();
        ZCHK(make_pow_table<F>(g, c, 0, nlo, cc.lo.get(), st));
        ZCHK(make_pow_table<F>(g, H::one(), h, nhi, cc.hi.get(), st));
        cc.h = h;
        cc.key = key;
        cc.valid = true;
    }
    out->lo = cc.lo.get();
    out->hi = cc.hi.get();
    out->h = cc.h;
    return ZKP_OK;
}

template <class F>
ScaleSpec<F> no_scale() {
    ScaleSpec<F> s;
    std::memset(&s, 0, sizeof s);  // (mode = SCALE_NONE = 0)
    return s;
}

// One strided pass of the shape sh.  chain: nothing was enqueued on st since the previous pass (ProfScope)
template <class F>
int launch_strided(const NttStridedParams<F>& sp, const NttStridedShape& sh, size_t batch, hipStream_t st, bool chain) {
    ProfScope ps(kClkNames[HostField<F>::CLK], st, chain);
    const dim3 grid((unsigned)sh.tiles, (unsigned)batch), block(NttOps<F>::THREADS);
    constexpr int T0 = NttOps<F>::LOG_T;  // tile widths: T0 (radix <= MAX_PASS_LOG) and, where the field has wide passes, T0 - 1, T0 - 2
    constexpr bool WIDE = NttOps<F>::WIDE_PASS_LOG > NttOps<F>::MAX_PASS_LOG;
    if (!WIDE || sh.log_t == T0) hipLaunchKernelGGL((ntt_pass_strided<F, T0>), grid, block, sh.lds, st, sp);
    else if constexpr (WIDE) {
        if (sh.log_t == T0 - 1) hipLaunchKernelGGL((ntt_pass_strided<F, T0 - 1>), grid, block, sh.lds, st, sp);
        else hipLaunchKernelGGL((ntt_pass_strided<F, T0 - 2>), grid, block, sh.lds, st, sp);
    }
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

template <class F>
int launch_last(const NttLastParams<F>& lp, const NttShape& s, size_t batch, hipStream_t st) {
    ProfScope ps(kClkNames[HostField<F>::CLK], st, s.passes > 1);  // passes of one transform are adjacent
    hipLaunchKernelGGL(ntt_pass_last<F>, dim3((unsigned)s.last.tiles, (unsigned)batch), dim3(NttOps<F>::THREADS), s.last.lds, st, lp);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

// Optional extras of a batched transform (the local pieces of the multi-GPU four-step NTT, zkp_hip/dist.py)
struct NttIo {
    const NttRemap* in_remap = nullptr;   // gathered input: logical element e of transform b at ntt_phys(...)
    const NttRemap* out_remap = nullptr;  // scattered output (same mapping on the natural output index)
    unsigned tw_log_n = 0;                // != 0: output k of transform b is multiplied by omega_{2^tw_log_n}^(+-(tw_row0 + b) k)
    uint64_t tw_row0 = 0;
};

template <class F>
int run_ntt(const F* d_in, F* d_data, unsigned log_n, size_t batch, int inverse, const uint64_t* coset, hipStream_t st,
            const NttIo* io = nullptr) {
    typedef typename HostField<F>::H H;
    if (log_n > 32) return fail(ZKP_E_ARG, "log_n > 32 (two-adicity of the field)");
    if (batch == 0 || log_n == 0) return ZKP_OK;  // size-1 transform is the identity (n^-1 = coset^0 = 1)
    if (batch > 65535) return fail(ZKP_E_ARG, "batch > 65535");
    inverse = inverse ? 1 : 0;
    NttPlan<F>* pl = nullptr;
    ZCHK(get_plan<F>(log_n, inverse, ((uint64_t)batch << log_n) >= (1ull << 19), &pl, st));
    const NttShape& s = pl->shape;
    const uint64_t n = 1ull << log_n;
    const int P = s.passes;
    // what is multiplied in at the first load (pre) and at the last store (post): the coset powers or the four-step twiddle, and
    // the 1/n of an inverse transform, which rides on whichever table is read anyway
    ScaleSpec<F> pre = no_scale<F>(), post = no_scale<F>();
    bool ninv_in_pass0 = false;  // ... on pass 0's inter-pass twiddles
    if (io && io->tw_log_n != 0) {
        if (coset) return fail(ZKP_E_ARG, "a coset and a four-step twiddle cannot be combined");
        if (!four_step_exponent_ok(io->tw_log_n, io->tw_row0, batch, log_n))
            return fail(ZKP_E_ARG, "four-step twiddle exponent (row0 + batch - 1) * (n - 1) must stay below 2^tw_log_n");
        post.mode = SCALE_POW_ROW;
        post.row0 = io->tw_row0;
        const H w = HostField<F>::root(io->tw_log_n);  // get_coset_tables inverts the base itself when inverse != 0
        ZCHK(get_coset_tables<F>(io->tw_log_n, inverse, w.l, inverse ? pl->n_inv : H::one(), &post.t, st));
    } else if (coset) {
        ScaleSpec<F>& sc = inverse ? post : pre;
        sc.mode = SCALE_POW;
        ZCHK(get_coset_tables<F>(log_n, inverse, coset, inverse ? pl->n_inv : H::one(), &sc.t, st));
    } else if (inverse && P == 1) {
        post.mode = SCALE_CONST;
        post.c = HostField<F>::tw(pl->n_inv);
    } else {
        ninv_in_pass0 = inverse != 0;
    }
    const NttRemap no_remap = {};
    const NttRemap& in_remap = (io && io->in_remap) ? *io->in_remap : no_remap;
    // the strided passes: d_in -> scratch, then in place
    F* work = d_data;
    if (P > 1) {
        ZCHK(ntt_scratch().ensure(sizeof(F) * n * batch));
        work = reinterpret_cast<F*>(ntt_scratch().p);
    }
    for (int p = 0; p + 1 < P; p++) {
        const NttStridedShape& sh = s.strided[p];
        NttStridedParams<F> sp;
        std::memset(&sp, 0, sizeof sp);
        sp.in = p == 0 ? d_in : work;
        sp.out = work;
        sp.tw = pl->tw[p];
        sp.n = n;
        sp.inner = sh.inner;
        sp.log_r = sh.log_r;
        const auto* direct = pl->direct[p];
        sp.tw_stride_log = direct ? 0 : sh.log_outer;
        sp.inter.lo = direct ? direct : ((p == 0 && ninv_in_pass0) ? pl->inter_lo_ninv : pl->inter_lo).get();
        sp.inter.hi = direct ? direct : pl->inter_hi.get();  // direct: never read, every exponent is below 2^h
        sp.inter.h = direct ? log_n - sh.log_outer : s.h;
        if (p == 0 && pass0_uses_matrix<NttOps<F>>(log_n, P, (unsigned)knob_int(KNOB_NTT_TW_MATRIX_MAX_LOG)))
            ZCHK(pass0_matrix<F>(*pl, ninv_in_pass0, st, &sp.tw_matrix));
        sp.pre = p == 0 ? pre : no_scale<F>();
        sp.clk = clk_record(HostField<F>::CLK);
        sp.remap = p == 0 ? in_remap : no_remap;
        ZCHK(launch_strided<F>(sp, sh, batch, st, p > 0));
    }
    // the last pass: natural order out
    NttLastParams<F> lp;
    std::memset(&lp, 0, sizeof lp);
    lp.in = P == 1 ? d_in : work;
    lp.out = d_data;
    lp.tw = pl->tw[P - 1];
    lp.n = n;
    lp.log_r = s.last.log_r;
    lp.log_r0 = s.last.log_r0;
    lp.log_m = s.last.log_m;
    lp.log_r1 = s.last.log_r1;
    lp.t_log = s.last.t_log;
    lp.pre = P == 1 ? pre : no_scale<F>();
    lp.post = post;
    lp.remap = P == 1 ? in_remap : no_remap;
    lp.out_remap = (io && io->out_remap) ? *io->out_remap : no_remap;
    lp.clk = clk_record(HostField<F>::CLK);
    return launch_last<F>(lp, s, batch, st);
}

template <class F>
int run_ntt(F* d_data, unsigned log_n, size_t batch, int inverse, const uint64_t* coset, hipStream_t st) {
    return run_ntt<F>(d_data, d_data, log_n, batch, inverse, coset, st, nullptr);
}

// Transforms of length 2^log_len along axis 0 of a row-major matrix [2^log_len][cols] (the columns are the contiguous
// direction), natural order in and out, every output (k, b) multiplied by omega_{2^tw_log_n}^(+-(col0 + b) k) when
// tw_log_n != 0 and by 1/2^log_len when inverse.  One or two strided passes (ntt_pass_strided): the last one stores the rows
// in natural order and applies the twiddle, so the matrix is read and written exactly once per pass and never transposed.
// This is the column half of the multi-GPU four-step transform: the all-to-all delivers [all rows][my columns].
template <class F>
int run_ntt_axis0(const F* d_in, F* d_out, unsigned log_len, size_t cols, int inverse, unsigned tw_log_n, uint64_t col0,
                  hipStream_t st) {
    typedef typename HostField<F>::H H;
    const NttAxis0Shape s = plan_ntt_axis0<NttOps<F>>(log_len, cols);
    if (s.error) return fail(ZKP_E_ARG, s.error);
    inverse = inverse ? 1 : 0;
    if (!four_step_exponent_ok(tw_log_n, col0, cols, log_len))
        return fail(ZKP_E_ARG, "four-step twiddle exponent (col0 + cols - 1) * (len - 1) must stay below 2^tw_log_n");
    NttState<F>& state = ntt_state<F>();
    // final factor table: c * base^e with c = 1/len for the inverse; base = the N-th root (or 1: a constant table)
    PowTab<F> fin;
    const H base = tw_log_n ? HostField<F>::root(tw_log_n) : H::one();
    ZCHK(get_coset_tables<F>(tw_log_n ? tw_log_n : log_len, inverse, base.l, inverse ? inv_pow2<H>(log_len) : H::one(), &fin, st));
    NttStridedParams<F> sp;
    std::memset(&sp, 0, sizeof sp);
    sp.n = (uint64_t)cols << log_len;
    sp.pre = no_scale<F>();
    sp.col_bits = s.col_bits;
    sp.clk = clk_record(HostField<F>::CLK);
    if (s.passes == 2) {
        // inter-pass twiddles omega_len^(k0 * d1): a direct table of `len` entries per (length, direction)
        ZCHK(cached_pow_table<F>(state.powers, log_len, inverse, 1u << log_len, &sp.inter.lo, st));
        ZCHK(ntt_scratch().ensure(sizeof(F) * sp.n));
        ZCHK(cached_pow_table<F>(state.radix, s.pass[0].log_r, inverse, 1u << (s.pass[0].log_r - 1), &sp.tw, st));
        sp.in = d_in;
        sp.out = reinterpret_cast<F*>(ntt_scratch().p);
        sp.inner = s.pass[0].inner;
        sp.log_r = s.pass[0].log_r;
        sp.inter.hi = sp.inter.lo;  // never read: every exponent is below 2^h
        sp.inter.h = log_len;
        ZCHK(launch_strided<F>(sp, s.pass[0], 1, st, false));
        d_in = sp.out;
    }
    const NttStridedShape& last = s.pass[s.passes - 1];
    ZCHK(cached_pow_table<F>(state.radix, last.log_r, inverse, 1u << (last.log_r - 1), &sp.tw, st));
    sp.in = d_in;
    sp.out = d_out;
    sp.inner = last.inner;
    sp.log_r = last.log_r;
    sp.axis0_last = 1;
    sp.tw_on = tw_log_n ? 1u : 0u;
    sp.outer_count = 1ull << last.log_outer;
    sp.col0 = col0;
    sp.inter = fin;
    return launch_strided<F>(sp, last, 1, st, false);
}
