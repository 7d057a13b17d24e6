// g1_ntt_host.inc -- zkp_g1_scale_dev, zkp_g1_ntt*, zkp_g1_bases_lagrange, the openers zkp_kzg_opener_* with zkp_kzg_open_cosets*,
// zkp_kzg_open_cosets_batch* and zkp_kzg_open_all* (one construction and one driver: all openings are the cosets of one point,
// log_l = 0, and one polynomial is the batch of one) and the verifier zkp_kzg_verify_coset
// (included at the end of api.hip, after verify_host.inc).  The kernels are in g1_ntt.hpp, every index and size in g1_ntt_plan.hpp.

namespace {

// Every (log_n, direction) row of twiddle constants (g1_ntt_plan.hpp: G1_NTT_TW_ROW), built once per process and uploaded once per slot
const std::vector<uint64_t>& g1_ntt_twiddle_rows() {
    static const std::vector<uint64_t> rows = [] {
        std::vector<uint64_t> t((size_t)(G1_NTT_MAX_LOG + 1) * 2 * G1_NTT_TW_ROW * 4);
        const HFr half = HFr::from_u64(2).inverse();
        HFr ninv = HFr::one();
        for (unsigned log_n = 0; log_n <= G1_NTT_MAX_LOG; log_n++, ninv = ninv * half)
            for (int inverse = 0; inverse < 2; inverse++) {
                uint64_t* row = &t[((size_t)log_n * 2 + inverse) * G1_NTT_TW_ROW * 4];
                HFr w = fr_root_of_unity(log_n);
                if (inverse) w = w.inverse();
                for (unsigned b = 0; b < G1_NTT_TW_ONE; b++, w = w.sqr()) w.store(row + 4 * b);
                HFr::one().store(row + 4 * G1_NTT_TW_ONE);
                ninv.store(row + 4 * G1_NTT_TW_NINV);
            }
        return t;
    }();
    return rows;
}
int g1_ntt_twiddle_row(unsigned log_n, int inverse, hipStream_t st, const Fr** row) {
    Ctx& c = ctx();
    const std::vector<uint64_t>& rows = g1_ntt_twiddle_rows();
    if (!c.g1_ntt_tw_ready) {
        ZCHK(c.g1_ntt_tw.ensure(8 * rows.size()));
        HIPCHK(hipMemcpyAsync(c.g1_ntt_tw.p, rows.data(), 8 * rows.size(), hipMemcpyHostToDevice, st));  // (the source is never freed)
        HIPCHK(hipStreamSynchronize(st));
        c.g1_ntt_tw_ready = true;
    }
    *row = reinterpret_cast<const Fr*>(c.g1_ntt_tw.p) + ((size_t)log_n * 2 + (inverse ? 1 : 0)) * G1_NTT_TW_ROW;
    return ZKP_OK;
}

// a vector of `cap` points in the plane-major workspace form, and the table its multiplying lanes use
struct G1NttVec {
    uint4* pts;
    uint64_t cap;
    uint4* table;
    uint64_t tcap;
};
G1NttVec g1_ntt_carve(void* base, unsigned log_n, const G1NttSizes& sz) {
    return G1NttVec{static_cast<uint4*>(base), (uint64_t)1 << log_n, reinterpret_cast<uint4*>(static_cast<char*>(base) + sz.points),
                    sz.table / G1_NTT_POINT_BYTES};
}

unsigned g1_ntt_blocks(uint64_t lanes, unsigned threads) { return (unsigned)((lanes + threads - 1) / threads); }

// launch(first, count) over the lanes [0, total) in pieces of at most G1_NTT_IO_LAUNCH, as the validation kernels: the load, store,
// gather, split and fold kernels, which take `first` and bound their own lanes
template <class Launch>
int g1_ntt_io_launches(uint64_t total, Launch&& launch) {
    for (uint64_t first = 0; first < total; first += G1_NTT_IO_LAUNCH) {
        launch(first, std::min<uint64_t>(G1_NTT_IO_LAUNCH, total - first));
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

template <bool RAW>
int g1_ntt_load(const void* d_pts, const uint8_t* d_inf, const G1NttLoadMap& map, const G1NttVec& v, hipStream_t st) {
    return g1_ntt_io_launches(map.count, [&](uint64_t first, uint64_t cnt) {
        hipLaunchKernelGGL(g1_ntt_load_kernel<RAW>, dim3(g1_ntt_blocks(cnt, MSM_THREADS)), dim3(MSM_THREADS), 0, st,
                           static_cast<const uint4*>(d_pts), d_inf, map, first, v.pts, v.cap);
    });
}
template <bool RAW>
int g1_ntt_store(const G1NttVec& v, uint64_t n, void* d_out, uint8_t* d_out_inf, hipStream_t st) {
    return g1_ntt_io_launches(n, [&](uint64_t first, uint64_t cnt) {
        hipLaunchKernelGGL(g1_ntt_store_kernel<RAW>, dim3(g1_ntt_blocks(cnt, MSM_THREADS)), dim3(MSM_THREADS), 0, st, v.pts, v.cap, first,
                           first + cnt, static_cast<uint4*>(d_out), d_out_inf);
    });
}

// v[i] <- [k_i] v[i] for i < n, in launches of at most G1_NTT_LAUNCH lanes; k_i = d_scalars[i * scalar_step]
int g1_ntt_mul(const G1NttVec& v, const Fr* d_scalars, unsigned scalar_step, uint64_t n, hipStream_t st) {
    for (uint64_t k = 0; k < g1_ntt_launches(n); k++) {
        const uint64_t cnt = g1_ntt_launch_lanes(n, k);
        hipLaunchKernelGGL(g1_ntt_mul_kernel, dim3(g1_ntt_blocks(cnt, G1_NTT_THREADS)), dim3(G1_NTT_THREADS), 0, st, v.pts, v.cap, d_scalars,
                           (uint32_t)scalar_step, k * G1_NTT_LAUNCH, (uint32_t)cnt, v.table, v.tcap);
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

// The stages over a vector loaded in bit-reversed order; natural order out.  scale: an inverse multiplies by n^-1 as well (without
// it the caller has folded that factor in elsewhere).  slices > 1: as many vectors, 2^log_n points apart behind v.pts, stage by
// stage together (unscaled only) -- a launch takes as many whole slices as G1_NTT_LAUNCH lanes and the table hold.  The kernel puts
// the table entries of grid row y at y * count, count <= lanes: nothing but `together` * lanes <= v.tcap, computed here, keeps them
// inside the table.
int g1_ntt_stages(const G1NttVec& v, unsigned log_n, int inverse, bool scale, hipStream_t st, uint64_t slices = 1) {
    if (!log_n) return ZKP_OK;
    const Fr* row = nullptr;
    ZCHK(g1_ntt_twiddle_row(log_n, inverse, st, &row));
    const uint64_t lanes = (uint64_t)1 << (log_n - 1);
    scale = scale && inverse;
    if (slices > 1 && scale) return fail(ZKP_E_ARG, "g1_ntt_stages: slices are transformed unscaled");
    const uint64_t together = std::max<uint64_t>(1, std::min<uint64_t>({slices, std::min(G1_NTT_LAUNCH, v.tcap) / lanes, 65535}));
    for (unsigned s = 0; s < log_n; s++) {
        const bool last_scaled = scale && s == log_n - 1;
        if (last_scaled) ZCHK(g1_ntt_mul(v, row + G1_NTT_TW_NINV, 0, lanes, st));  // the left operands
        for (uint64_t y = 0; y < slices; y += together)
            for (uint64_t k = 0; k < g1_ntt_launches(lanes); k++) {
                const uint64_t cnt = g1_ntt_launch_lanes(lanes, k);
                hipLaunchKernelGGL(g1_ntt_butterfly_kernel, dim3(g1_ntt_blocks(cnt, G1_NTT_THREADS), (unsigned)std::min(together, slices - y)),
                                   dim3(G1_NTT_THREADS), 0, st, v.pts + (y << log_n), v.cap, (uint32_t)log_n, (uint32_t)s,
                                   (uint32_t)(k * G1_NTT_LAUNCH), (uint32_t)cnt, row, last_scaled ? 1u : 0u, v.table, v.tcap);
                HIPCHK(hipGetLastError());
            }
    }
    return ZKP_OK;
}

// raw device points in place; the caller is inside the slot's context
int g1_ntt_raw_locked(void* d_xy, uint8_t* d_is_inf, unsigned log_n, int inverse, void* ws, hipStream_t st) {
    const uint64_t n = (uint64_t)1 << log_n;
    const G1NttVec v = g1_ntt_carve(ws, log_n, g1_ntt_sizes(log_n, n / 2));
    ZCHK(g1_ntt_load<true>(d_xy, d_is_inf, g1_ntt_load_plain(log_n), v, st));
    ZCHK(g1_ntt_stages(v, log_n, inverse, true, st));
    return g1_ntt_store<true>(v, n, d_xy, d_is_inf, st);
}

const char* const kShardedG1Ntt = "bases are sharded over several devices: a transform over points runs on one device "
                                  "(zkp_set_device + zkp_g1_bases_create* make single-device bases)";

}  // namespace

// log_l: one proof per coset of 2^log_l points; 0: all n openings.  work: (the partial sums,) u, the slice h, the scalars g and the
// lanes' table of one call of up to max_polys polynomials
struct zkp_kzg_opener : KzgHandle {
    unsigned group_log = 0;  // a lane of the multiply-accumulate pass sums 2^group_log terms (g1_coset_mac; one at most when l = 1)
    uint64_t max_polys = 1;  // polynomials of one call (zkp_kzg_open_cosets_batch*); the other entries open one
    DevBuf srs_hat;  // the l slices of the reversed SRS points, each transformed (NTT_2r): depends on the SRS, n and l only
};

extern "C" {

int zkp_g1_scale_dev(void* d_xy, uint8_t* d_is_inf, const void* d_scalars, size_t n, void* stream) try {
    if (n && (!d_xy || !d_scalars)) return fail(ZKP_E_ARG, "null argument");
    if (!n) return ZKP_OK;
    int slot = -1;
    ZCHK(slot_of_device_pointer(d_xy, &slot));
    CTX_ENTER(slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    const uint64_t step = std::min<uint64_t>(n, G1_NTT_LAUNCH);
    void* ws = nullptr;
    ZCHK(slot_workspace(2 * G1_NTT_POINT_BYTES * step, "zkp_g1_scale_dev", &ws));
    const G1NttVec v{static_cast<uint4*>(ws), step, static_cast<uint4*>(ws) + 16 * step, step};
    for (uint64_t off = 0; off < n; off += step) {
        const uint64_t cnt = std::min<uint64_t>(step, n - off);
        char* xy = static_cast<char*>(d_xy) + 96 * off;
        uint8_t* inf = d_is_inf ? d_is_inf + off : nullptr;
        ZCHK(g1_ntt_load<true>(xy, inf, G1NttLoadMap{cnt, cnt, 0, 1, 0}, v, st));
        ZCHK(g1_ntt_mul(v, static_cast<const Fr*>(d_scalars) + off, 1, cnt, st));
        ZCHK(g1_ntt_store<true>(v, cnt, xy, inf, st));
    }
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_ntt_dev(void* d_xy, uint8_t* d_is_inf, unsigned log_n, int inverse, void* stream) try {
    if (!d_xy || !d_is_inf) return fail(ZKP_E_ARG, "null argument");
    if (log_n > G1_NTT_MAX_LOG) return fail(ZKP_E_ARG, "log_n > 24");
    int slot = -1;
    ZCHK(slot_of_device_pointer(d_xy, &slot));
    CTX_ENTER(slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    void* ws = nullptr;
    ZCHK(slot_workspace(g1_ntt_sizes(log_n, ((uint64_t)1 << log_n) / 2).total, "zkp_g1_ntt_dev", &ws));
    return g1_ntt_raw_locked(d_xy, d_is_inf, log_n, inverse, ws, st);
} ZKP_CATCH_INT

int zkp_g1_ntt(uint64_t* xy, uint8_t* is_inf, unsigned log_n, int inverse) try {
    if (!xy || !is_inf) return fail(ZKP_E_ARG, "null argument");
    if (log_n > G1_NTT_MAX_LOG) return fail(ZKP_E_ARG, "log_n > 24");
    CTX_ENTER(-1);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t n = (size_t)1 << log_n;
    const size_t ws_bytes = g1_ntt_sizes(log_n, n / 2).total;
    void* ws = nullptr;
    ZCHK(slot_workspace(ws_bytes + 96 * n + n, "zkp_g1_ntt", &ws));
    char* d_xy = static_cast<char*>(ws) + ws_bytes;
    uint8_t* d_inf = reinterpret_cast<uint8_t*>(d_xy + 96 * n);
    HIPCHK(hipMemcpyAsync(d_xy, xy, 96 * n, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_inf, is_inf, n, hipMemcpyHostToDevice, st));
    ZCHK(g1_ntt_raw_locked(d_xy, d_inf, log_n, inverse, ws, st));
    HIPCHK(hipMemcpyAsync(xy, d_xy, 96 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(is_inf, d_inf, n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_bases_lagrange(const zkp_bases* srs, unsigned log_n, zkp_bases** out) try {
    if (!srs || !out) return fail(ZKP_E_ARG, "null argument");
    if (log_n > G1_NTT_MAX_LOG) return fail(ZKP_E_ARG, "log_n > 24");
    if (!srs->shards.empty()) return fail(ZKP_E_ARG, kShardedG1Ntt);
    const size_t n = (size_t)1 << log_n;
    if (srs->n < n) return fail(ZKP_E_SIZE, "the SRS has fewer than 2^log_n points");
    CTX_ENTER(srs->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    void* ws = nullptr;
    ZCHK(slot_workspace(g1_ntt_sizes(log_n, n / 2).total, "zkp_g1_bases_lagrange", &ws));
    const G1NttVec v = g1_ntt_carve(ws, log_n, g1_ntt_sizes(log_n, n / 2));
    zkp_bases* raw = nullptr;
    ZCHK(bases_alloc(n, true, &raw));
    std::unique_ptr<zkp_bases, void (*)(zkp_bases*)> b(raw, zkp_g1_bases_destroy);
    ZCHK(g1_ntt_load<false>(srs->d_xy.p, srs->d_inf.get(), g1_ntt_load_plain(log_n), v, st));  // plane 0 of an expansion: the points
    ZCHK(g1_ntt_stages(v, log_n, 1, true, st));
    ZCHK(g1_ntt_store<false>(v, n, b->d_xy.p, b->d_inf.get(), st));
    HIPCHK(hipStreamSynchronize(st));
    *out = b.release();
    return ZKP_OK;
} ZKP_CATCH_INT

void zkp_kzg_opener_destroy(zkp_kzg_opener* o) { handle_destroy(o); }

}  // extern "C"

namespace {

// (cosets: the call is one of zkp_kzg_open_cosets*, which take an opener of any log_l; zkp_kzg_open_all* one of log_l = 0 only)
int kzg_open_all_args(const zkp_kzg_opener* o, const void* coeffs, size_t len, const void* out_xy, const void* out_is_inf, bool cosets = false) {
    if (!o || !coeffs || !out_xy || !out_is_inf) return fail(ZKP_E_ARG, "null argument");
    if (o->log_l && !cosets) return fail(ZKP_E_ARG, "the opener was made for cosets (zkp_kzg_opener_create_cosets): zkp_kzg_open_cosets opens with it");
    if (len == 0) return fail(ZKP_E_ARG, "open of an empty polynomial (kzg/src/scheme.rs:112 expects at least 1)");
    if (len > ((size_t)1 << o->log_n)) return fail(ZKP_E_SIZE, "more coefficients than the opener's domain has points");
    return ZKP_OK;
}

// `rows` rows of 2^log_m scalars each, transformed in place (a batched transform takes at most 65535 rows)
int coset_fr_rows(Fr* g, unsigned log_m, uint64_t rows, hipStream_t st) {
    const uint64_t step = 32768;
    for (uint64_t first = 0; first < rows; first += step)
        ZCHK(run_ntt<Fr>(g + (first << log_m), log_m, (size_t)std::min<uint64_t>(step, rows - first), 0, nullptr, st));
    return ZKP_OK;
}

// where the pieces of an opener's `work` begin (g1_coset_sizes); every vector has room for max_polys polynomials
struct CosetWork {
    G1CosetSizes sz;
    G1CosetMac mac;  // of one polynomial
    uint4 *partial, *u, *h, *table;
    Fr* g;
    uint64_t tcap;
};
CosetWork coset_work(const zkp_kzg_opener* o) {
    CosetWork w;
    w.sz = g1_coset_sizes(o->log_n, o->log_l, o->group_log, o->max_polys);
    w.mac = g1_coset_mac(o->log_n, o->log_l, o->group_log);
    char* base = static_cast<char*>(o->work.p);
    w.partial = reinterpret_cast<uint4*>(base);
    w.u = reinterpret_cast<uint4*>(base + w.sz.partial);
    w.h = reinterpret_cast<uint4*>(base + w.sz.partial + w.sz.work);
    w.g = reinterpret_cast<Fr*>(base + w.sz.partial + w.sz.work + w.sz.slice);
    w.table = reinterpret_cast<uint4*>(base + w.sz.partial + w.sz.work + w.sz.slice + w.sz.scalars);
    w.tcap = w.sz.table / G1_NTT_POINT_BYTES;
    return w;
}

// the evaluations of `rows` polynomials on the whole domain: rows of n, natural order (coset k at k + j r)
int coset_evals(const void* d_coeffs, uint64_t rows, size_t len, size_t stride, unsigned log_n, void* d_out_evals, hipStream_t st) {
    const size_t n = (size_t)1 << log_n;
    HIPCHK(hipMemsetAsync(d_out_evals, 0, 32 * n * rows, st));
    if (rows == 1) HIPCHK(hipMemcpyAsync(d_out_evals, d_coeffs, 32 * len, hipMemcpyDeviceToDevice, st));
    else HIPCHK(hipMemcpy2DAsync(d_out_evals, 32 * n, d_coeffs, 32 * stride, 32 * len, rows, hipMemcpyDeviceToDevice, st));
    return coset_fr_rows(static_cast<Fr*>(d_out_evals), log_n, rows, st);
}

// One call of an opener over n_polys <= max_polys polynomials (rows of len coefficients, `stride` scalars apart), log_l = 0 (all
// openings, r = n) as any other and one polynomial as any other number: every step runs once, for all polynomials together.
// Everything on the device, on `st`; the caller is inside the opener's slot.  Outputs are polynomial-major.
int kzg_open_locked(const zkp_kzg_opener* o, const void* d_coeffs, uint64_t n_polys, size_t len, size_t stride, void* d_out_xy,
                    uint8_t* d_out_is_inf, void* d_out_evals, hipStream_t st) {
    const unsigned log_n = o->log_n, log_l = o->log_l, log_r = log_n - log_l, log_m = log_r + 1;
    const uint64_t n = (uint64_t)1 << log_n, r = (uint64_t)1 << log_r, l = (uint64_t)1 << log_l;
    const CosetWork w = coset_work(o);
    const G1CosetBatch bt = g1_coset_batch(log_n, log_l, o->group_log, n_polys, w.tcap);
    const G1NttVec u{w.u, o->max_polys * 2 * r, w.table, w.tcap}, h{w.h, o->max_polys * r, w.table, w.tcap};
    const Fr* row = nullptr;
    ZCHK(g1_ntt_twiddle_row(log_m, 1, st, &row));
    {   // the l rows of g of every polynomial, transformed as one batch; then every scalar times (2r)^-1, split
        ProfScope ps("kzg_open_scalars", st);
        ZCHK(g1_ntt_io_launches(n_polys * 2 * n, [&](uint64_t first, uint64_t cnt) {
            hipLaunchKernelGGL(g1_ntt_gather_kernel, dim3(g1_ntt_blocks(cnt, MSM_THREADS)), dim3(MSM_THREADS), 0, st,
                               static_cast<const Fr*>(d_coeffs), (uint64_t)len, (uint64_t)stride, n_polys, (uint32_t)log_n, (uint32_t)log_l, first, w.g);
        }));
        ZCHK(coset_fr_rows(w.g, log_m, n_polys * l, st));
        ZCHK(g1_ntt_io_launches(n_polys * 2 * n, [&](uint64_t first, uint64_t cnt) {
            hipLaunchKernelGGL(g1_ntt_split_kernel, dim3(g1_ntt_blocks(cnt, MSM_THREADS)), dim3(MSM_THREADS), 0, st, w.g, row + G1_NTT_TW_NINV,
                               first, n_polys * 2 * n);
        }));
    }
    {   // U_k = sum_b [g^_k] S^_k: the lanes' groups, then the fold of the partial sums into u (bit-reversed for the stages); one group
        // per output (always so at l = 1) writes u itself
        ProfScope ps("kzg_open_mac", st);
        const bool folded = w.mac.groups > 1;
        const uint64_t pcap = o->max_polys << bt.lanes_log;
        for (uint64_t k = 0; k < g1_coset_batch_launches(bt); k++) {
            const uint64_t cnt = g1_coset_batch_launch_lanes(bt, k);
            hipLaunchKernelGGL(g1_ntt_mac_kernel, dim3(g1_ntt_blocks(cnt, G1_NTT_THREADS)), dim3(G1_NTT_THREADS), 0, st,
                               static_cast<const uint4*>(o->srs_hat.p), 2 * n, reinterpret_cast<const uint32_t*>(w.g), (uint32_t)log_m,
                               w.mac.terms, (uint32_t)bt.lanes_log, k * bt.launch_lanes, (uint32_t)cnt, folded ? w.partial : u.pts, folded ? pcap : u.cap,
                               folded ? 0u : (uint32_t)log_m, w.table, w.tcap);
            HIPCHK(hipGetLastError());
        }
        for (unsigned i = 0; i < g1_coset_fold_steps(w.mac); i++) {
            const G1CosetFoldStep f = g1_coset_fold_step(log_n, log_l, w.mac, i);
            const unsigned step_log = g1_coset_fold_step_log(log_n, log_l, w.mac, i);
            ZCHK(g1_ntt_io_launches(n_polys * f.lanes, [&](uint64_t first, uint64_t cnt) {
                hipLaunchKernelGGL(g1_ntt_fold_kernel, dim3(g1_ntt_blocks(cnt, G1_NTT_THREADS)), dim3(G1_NTT_THREADS), 0, st, w.partial, pcap,
                                   (uint32_t)bt.lanes_log, (uint32_t)step_log, n_polys, first, u.pts, u.cap, f.last ? (uint32_t)log_m : 0u);
            }));
        }
    }
    {   // u of every polynomial stage by stage together; the proofs: NTT_r of the slices h, likewise
        ProfScope ps("kzg_open_transforms", st);
        ZCHK(g1_ntt_stages(u, log_m, 1, false, st, n_polys));
        ZCHK(g1_ntt_io_launches(n_polys * r, [&](uint64_t first, uint64_t cnt) {
            hipLaunchKernelGGL(g1_ntt_slice_kernel, dim3(g1_ntt_blocks(cnt, MSM_THREADS)), dim3(MSM_THREADS), 0, st, u.pts, u.cap,
                               g1_coset_slice_map(log_n, log_l), (uint32_t)log_m, n_polys, first, h.pts, h.cap);
        }));
        ZCHK(g1_ntt_stages(h, log_r, 0, false, st, n_polys));
        ZCHK(g1_ntt_store<true>(h, n_polys * r, d_out_xy, d_out_is_inf, st));
    }
    if (d_out_evals) ZCHK(coset_evals(d_coeffs, n_polys, len, stride, log_n, d_out_evals, st));
    return ZKP_OK;
}

// the device entries: nothing is allocated, nothing waited for
int kzg_open_dev(const zkp_kzg_opener* o, const void* d_coeffs, size_t len, void* d_out_xy, uint8_t* d_out_is_inf, void* d_out_evals,
                 void* stream, bool cosets) {
    ZCHK(kzg_open_all_args(o, d_coeffs, len, d_out_xy, d_out_is_inf, cosets));
    CTX_ENTER(o->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_open_locked(o, d_coeffs, 1, len, len, d_out_xy, d_out_is_inf, d_out_evals, st);
}

// the host entries (`what`: the entry's name), r = n / l proofs out
int kzg_open_host(const zkp_kzg_opener* o, const uint64_t* coeffs, size_t len, uint64_t* out_xy, uint8_t* out_is_inf, uint64_t* out_evals,
                  const char* what, bool cosets) {
    ZCHK(kzg_open_all_args(o, coeffs, len, out_xy, out_is_inf, cosets));
    CTX_ENTER(o->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t n = (size_t)1 << o->log_n, r = n >> o->log_l;
    void* ws = nullptr;  // coefficients | evaluations | points | flags
    ZCHK(slot_workspace(32 * len + 32 * n + 96 * r + r, what, &ws));
    char* d_coeffs = static_cast<char*>(ws);
    char* d_evals = d_coeffs + 32 * len;
    char* d_xy = d_evals + 32 * n;
    uint8_t* d_inf = reinterpret_cast<uint8_t*>(d_xy + 96 * r);
    HIPCHK(hipMemcpyAsync(d_coeffs, coeffs, 32 * len, hipMemcpyHostToDevice, st));
    ZCHK(kzg_open_locked(o, d_coeffs, 1, len, len, d_xy, d_inf, out_evals ? d_evals : nullptr, st));
    HIPCHK(hipMemcpyAsync(out_xy, d_xy, 96 * r, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_is_inf, d_inf, r, hipMemcpyDeviceToHost, st));
    if (out_evals) HIPCHK(hipMemcpyAsync(out_evals, d_evals, 32 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZKP_OK;
}

// zkp_kzg_open_cosets_batch*: every refusal, before anything is launched; *none: an empty batch, nothing to do
int kzg_open_batch_args(const zkp_kzg_opener* o, const void* coeffs, size_t n_polys, size_t len, size_t stride, const void* out_xy,
                        const void* out_is_inf, bool* none) {
    ZCHK(kzg_open_all_args(o, coeffs, len, out_xy, out_is_inf, true));
    if (stride < len) return fail(ZKP_E_ARG, "stride < len: the rows of coefficients overlap");
    if (n_polys > o->max_polys)
        return fail(ZKP_E_SIZE, "a batch of " + std::to_string(n_polys) + " polynomials on an opener made for " + std::to_string(o->max_polys) +
                                    " (max_polys of zkp_kzg_opener_create_cosets_batch)");
    *none = n_polys == 0;
    return ZKP_OK;
}

}  // namespace

extern "C" {

int zkp_kzg_opener_create_cosets_batch(const zkp_bases* srs, unsigned log_n, unsigned log_l, size_t max_polys, zkp_kzg_opener** out) try {
    if (!srs || !out) return fail(ZKP_E_ARG, "null argument");
    if (max_polys == 0 || max_polys > G1_COSET_MAX_POLYS) return fail(ZKP_E_ARG, "an opener takes 1 .. 4096 polynomials per call (max_polys)");
    if (!g1_coset_shape_ok(log_n, log_l)) return fail(ZKP_E_ARG, "an opener needs log_l < log_n <= 23");
    if (!srs->shards.empty()) return fail(ZKP_E_ARG, kShardedG1Ntt);
    const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l;
    if (srs->n < n - l) return fail(ZKP_E_SIZE, "the SRS has fewer than 2^log_n - 2^log_l points");
    CTX_ENTER(srs->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    auto o = handle_new<zkp_kzg_opener>(log_n, log_l);
    if (!o) return fail(ZKP_E_NOMEM, "host allocation failed");
    static_assert(kKnobs[KNOB_KZG_COSET_GROUP_LOG].hi == G1_COSET_MAX_GROUP_LOG && G1_COSET_GROUP_LOG <= G1_COSET_MAX_GROUP_LOG,
                  "knobs.hpp: g1_ntt_mac_kernel keeps the words of at most 2^G1_COSET_MAX_GROUP_LOG terms");
    o->group_log = (unsigned)knob_int(KNOB_KZG_COSET_GROUP_LOG, G1_COSET_GROUP_LOG);
    o->max_polys = max_polys;
    const G1CosetSizes sz = g1_coset_sizes(log_n, log_l, o->group_log, max_polys);
    ZCHK(reserve_or_refuse(sz.total, KNOB_KZG_OPENER_MAX_BYTES,
                           "zkp_kzg_opener_create_cosets: the workspaces of " + std::to_string(sz.total) + " bytes (" + std::to_string(sz.srs_hat) +
                               " kept slices + " + std::to_string(sz.total - sz.srs_hat) + " per call of max_polys " + std::to_string(max_polys) +
                               ") do not fit",
                           [&] { return o->srs_hat.grow(sz.srs_hat) == hipSuccess && o->work.grow(sz.total - sz.srs_hat) == hipSuccess; }));
    const CosetWork w = coset_work(o.get());
    // slice b: 2r points of the plane-major array of 2n, at b 2r; all of them are transformed where they stay, stage by stage together
    // (the table of these transforms is where the calls keep theirs)
    const G1NttVec all{static_cast<uint4*>(o->srs_hat.p), 2 * n, w.table, w.tcap};
    ZCHK(g1_ntt_io_launches(2 * n, [&](uint64_t first, uint64_t cnt) {
        hipLaunchKernelGGL(g1_ntt_load_slices_kernel, dim3(g1_ntt_blocks(cnt, MSM_THREADS)), dim3(MSM_THREADS), 0, st,
                           static_cast<const uint4*>(srs->d_xy.p), srs->d_inf.get(), (uint32_t)log_n, (uint32_t)log_l, first, all.pts, all.cap);
    }));
    ZCHK(g1_ntt_stages(all, log_n - log_l + 1, 0, false, st, l));
    {   // Everything a call builds on first use is built here, so that zkp_kzg_open_*_dev neither allocate nor wait: the plans, tables
        // and scratch of its Fr transforms (over the zeroed scalar area) and the constants of its point transforms
        // (a call of one polynomial and a call of max_polys may take different plans of an Fr transform, and the larger needs the
        // larger scratch: both are run)
        const Fr* row = nullptr;
        HIPCHK(hipMemsetAsync(w.g, 0, sz.scalars, st));
        for (const uint64_t polys : {(uint64_t)1, (uint64_t)max_polys}) {
            ZCHK(coset_fr_rows(w.g, log_n - log_l + 1, polys * l, st));
            ZCHK(coset_fr_rows(w.g, log_n, polys, st));
            if (max_polys == 1) break;
        }
        ZCHK(g1_ntt_twiddle_row(log_n - log_l + 1, 1, st, &row));
    }
    HIPCHK(hipStreamSynchronize(st));
    *out = o.release();
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_kzg_opener_create_cosets(const zkp_bases* srs, unsigned log_n, unsigned log_l, zkp_kzg_opener** out) {
    return zkp_kzg_opener_create_cosets_batch(srs, log_n, log_l, 1, out);
}

int zkp_kzg_open_cosets_batch_dev(const zkp_kzg_opener* o, const void* d_coeffs, size_t n_polys, size_t len, size_t stride, void* d_out_xy,
                                  uint8_t* d_out_is_inf, void* d_out_evals, void* stream) try {
    bool none = false;
    ZCHK(kzg_open_batch_args(o, d_coeffs, n_polys, len, stride, d_out_xy, d_out_is_inf, &none));
    if (none) return ZKP_OK;
    CTX_ENTER(o->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_open_locked(o, d_coeffs, n_polys, len, stride, d_out_xy, d_out_is_inf, d_out_evals, st);
} ZKP_CATCH_INT

// the rows are packed on the way to the device: what lies between len and stride is not read
int zkp_kzg_open_cosets_batch(const zkp_kzg_opener* o, const uint64_t* coeffs, size_t n_polys, size_t len, size_t stride, uint64_t* out_xy,
                              uint8_t* out_is_inf, uint64_t* out_evals) try {
    bool none = false;
    ZCHK(kzg_open_batch_args(o, coeffs, n_polys, len, stride, out_xy, out_is_inf, &none));
    if (none) return ZKP_OK;
    CTX_ENTER(o->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t n = (size_t)1 << o->log_n, r = n >> o->log_l, P = n_polys;
    void* ws = nullptr;  // coefficients | evaluations | points | flags
    ZCHK(slot_workspace(P * (32 * len + 32 * n + 96 * r + r), "zkp_kzg_open_cosets_batch", &ws));
    char* d_coeffs = static_cast<char*>(ws);
    char* d_evals = d_coeffs + 32 * len * P;
    char* d_xy = d_evals + 32 * n * P;
    uint8_t* d_inf = reinterpret_cast<uint8_t*>(d_xy + 96 * r * P);
    if (stride == len || P == 1) HIPCHK(hipMemcpyAsync(d_coeffs, coeffs, 32 * len * P, hipMemcpyHostToDevice, st));
    else HIPCHK(hipMemcpy2DAsync(d_coeffs, 32 * len, coeffs, 32 * stride, 32 * len, P, hipMemcpyHostToDevice, st));
    ZCHK(kzg_open_locked(o, d_coeffs, P, len, len, d_xy, d_inf, out_evals ? d_evals : nullptr, st));
    HIPCHK(hipMemcpyAsync(out_xy, d_xy, 96 * r * P, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(out_is_inf, d_inf, r * P, hipMemcpyDeviceToHost, st));
    if (out_evals) HIPCHK(hipMemcpyAsync(out_evals, d_evals, 32 * n * P, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_kzg_open_cosets_dev(const zkp_kzg_opener* o, const void* d_coeffs, size_t len, void* d_out_xy, uint8_t* d_out_is_inf, void* d_out_evals,
                            void* stream) try {
    return kzg_open_dev(o, d_coeffs, len, d_out_xy, d_out_is_inf, d_out_evals, stream, true);
} ZKP_CATCH_INT

int zkp_kzg_open_cosets(const zkp_kzg_opener* o, const uint64_t* coeffs, size_t len, uint64_t* out_xy, uint8_t* out_is_inf,
                        uint64_t* out_evals) try {
    return kzg_open_host(o, coeffs, len, out_xy, out_is_inf, out_evals, "zkp_kzg_open_cosets", true);
} ZKP_CATCH_INT

// all n openings: the cosets of one point, through an opener of log_l = 0
int zkp_kzg_opener_create(const zkp_bases* srs, unsigned log_n, zkp_kzg_opener** out) { return zkp_kzg_opener_create_cosets(srs, log_n, 0, out); }

int zkp_kzg_open_all_dev(const zkp_kzg_opener* o, const void* d_coeffs, size_t len, void* d_out_xy, uint8_t* d_out_is_inf, void* d_out_evals,
                         void* stream) try {
    return kzg_open_dev(o, d_coeffs, len, d_out_xy, d_out_is_inf, d_out_evals, stream, false);
} ZKP_CATCH_INT

int zkp_kzg_open_all(const zkp_kzg_opener* o, const uint64_t* coeffs, size_t len, uint64_t* out_xy, uint8_t* out_is_inf,
                     uint64_t* out_evals) try {
    return kzg_open_host(o, coeffs, len, out_xy, out_is_inf, out_evals, "zkp_kzg_open_all", false);
} ZKP_CATCH_INT

// e(W, [s^l]_2 - x^l G_2) == e(C - [I(s)]_1, G_2), I the interpolant of evals[j] at x w_l^j, j < l: coefficient i of I is x^-i times
// coefficient i of the inverse transform of size l of the evaluations (host, O(l log l)); [I(s)]_1 is zkp_kzg_commit over `srs`
int zkp_kzg_verify_coset(const zkp_bases* srs, const uint64_t g2_sl_xy[24], const uint64_t commit_xy[12], uint8_t commit_is_inf,
                         const uint64_t w_xy[12], uint8_t w_is_inf, const uint64_t x[4], unsigned log_l, const uint64_t* evals,
                         int* accepted) try {
    if (!srs || !g2_sl_xy || (!commit_is_inf && !commit_xy) || (!w_is_inf && !w_xy) || !x || !evals || !accepted)
        return fail(ZKP_E_ARG, "null argument");
    if (log_l >= G1_NTT_MAX_LOG - 1) return fail(ZKP_E_ARG, "log_l of a coset is below 23");
    const uint64_t l = (uint64_t)1 << log_l;
    if (srs->n < l) return fail(ZKP_E_SIZE, "the SRS has fewer than 2^log_l points");
    const G2Aff g2 = G2Aff::generator();
    G2Aff g2sl = G2Aff::infinity();
    ZCHK(g2_validate(g2_sl_xy, "[s^l]_2", &g2sl));
    ZCHK(g1_validate(commit_xy, commit_is_inf, "commitment"));
    ZCHK(g1_validate(w_xy, w_is_inf, "opening"));
    const HFr hx = HFr::load(x);
    if (hx == HFr::zero()) return fail(ZKP_E_ARG, "x = 0 is the shift of no coset");
    // inverse transform of the evaluations, decimation in time
    std::vector<HFr> c(l);
    for (uint64_t j = 0; j < l; j++) c[g1_ntt_bitrev((uint32_t)j, log_l)] = HFr::load(evals + 4 * j);
    const HFr w_inv = fr_root_of_unity(log_l).inverse();
    for (unsigned s = 0; s < log_l; s++) {
        const uint64_t half = (uint64_t)1 << s;
        HFr ws = w_inv;
        for (unsigned q = s + 1; q < log_l; q++) ws = ws.sqr();  // the root of order 2 half
        for (uint64_t blk = 0; blk < l; blk += 2 * half) {
            HFr tw = HFr::one();
            for (uint64_t j = 0; j < half; j++, tw = tw * ws) {
                const HFr a = c[blk + j], t = c[blk + j + half] * tw;
                c[blk + j] = a + t;
                c[blk + j + half] = a - t;
            }
        }
    }
    const HFr x_inv = hx.inverse();
    HFr scale = HFr::from_u64(l).inverse();
    std::vector<uint64_t> coeffs(4 * l);
    for (uint64_t i = 0; i < l; i++, scale = scale * x_inv) (c[i] * scale).store(&coeffs[4 * i]);
    uint64_t i_xy[12];
    uint8_t i_inf = 0;
    ZCHK(zkp_kzg_commit(srs, coeffs.data(), (size_t)l, i_xy, &i_inf));
    const G2Aff a = g2sl.add(g2.mul(hx.pow_u64(l).from_mont().l).neg());
    const HXyzz b = g1_load(commit_xy, commit_is_inf).add(g1_load(i_xy, i_inf).negate());
    *accepted = pairings_equal(g1_load(w_xy, w_is_inf), a, b, g2) ? 1 : 0;
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
