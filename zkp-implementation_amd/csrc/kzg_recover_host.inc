// kzg_recover_host.inc -- zkp_kzg_recoverer_* and zkp_kzg_recover_cosets*: the polynomial behind an extended blob from any half of
// its cosets (included at the end of api.hip, after g1_ntt_host.inc).  The kernels are in kzg_recover.hpp; the construction, every
// launch, index and size in kzg_recover_plan.hpp: the driver walks kzg_recover_step and launches nothing else.  A batch
// (zkp_kzg_recoverer_create_batch, zkp_kzg_recover_cosets_batch*) is the same walk with `polys` rows in the n-sized steps.

struct zkp_kzg_recoverer : KzgHandle {  // work: kzg_recover_sizes_batch
    unsigned leaf_log = 0;  // ZKP_KZG_RECOVER_LEAF_LOG as it was at creation
    uint64_t max_polys = 1;  // rows of one call (zkp_kzg_recover_cosets_batch*); the other entries recover one
    uint64_t g[4] = {}, gl[4] = {};  // the coset shift g = 7 and g^l, Montgomery
    FrPow2 rho;                      // the powers of rho = w^l, the root of the transforms of r
    mutable Stream side;             // the inversions of a call run here, beside the transforms of n on the caller's stream
    mutable Event fork, join;        // ... after `fork` on the caller's stream; the divide pass waits for `join`
    mutable HostStage stage;         // the missing-index list and the mask on their way to the device
};

namespace {

unsigned recover_blocks(uint64_t lanes) { return (unsigned)((lanes + KZG_RECOVER_THREADS - 1) / KZG_RECOVER_THREADS); }

// `batch` transforms of 2^log, contiguous, in pieces of KZG_RECOVER_NTT_BATCH
int recover_fr_rows(Fr* v, unsigned log, uint64_t batch, int inverse, hipStream_t st) {
    for (uint64_t first = 0; first < batch; first += KZG_RECOVER_NTT_BATCH)
        ZCHK(run_ntt<Fr>(v + (first << log), log, (size_t)std::min<uint64_t>(KZG_RECOVER_NTT_BATCH, batch - first), inverse, nullptr, st));
    return ZKP_OK;
}

int recover_args(const zkp_kzg_recoverer* rc, const void* evals, const uint8_t* present, size_t len, const void* out_coeffs, const void* flag,
                 uint64_t* missing) {
    if (!rc || !evals || !present || !out_coeffs || !flag) return fail(ZKP_E_ARG, "null argument");
    if (len == 0) return fail(ZKP_E_ARG, "recovery of an empty polynomial");
    const uint64_t n = (uint64_t)1 << rc->log_n, r = n >> rc->log_l;
    if (len > n) return fail(ZKP_E_SIZE, "more coefficients than the recoverer's domain has points");
    uint64_t m = 0;
    for (uint64_t k = 0; k < r; k++) m += present[k] ? 0 : 1;
    if (!kzg_recoverable(rc->log_n, rc->log_l, m, len))
        return fail(ZKP_E_SIZE, std::to_string(r - m) + " present cells of l = " + std::to_string(n / r) + " points do not determine len = " +
                                    std::to_string(len) + " coefficients");
    *missing = m;
    return ZKP_OK;
}

// zkp_kzg_recover_cosets_batch*: every refusal, before anything is launched -- the single entry's own first; *none: an empty
// batch, nothing to do
int recover_batch_args(const zkp_kzg_recoverer* rc, const void* evals, size_t n_polys, const uint8_t* present, size_t len, size_t stride, int layout,
                       const void* out_coeffs, const void* flag, uint64_t* missing, bool* none) {
    ZCHK(recover_args(rc, evals, present, len, out_coeffs, flag, missing));
    if (stride < len) return fail(ZKP_E_ARG, "stride < len: the rows of coefficients overlap");
    if (layout != KZG_RECOVER_NATURAL && layout != KZG_RECOVER_CELLS)
        return fail(ZKP_E_ARG, "layout " + std::to_string(layout) + " is neither ZKP_KZG_LAYOUT_NATURAL nor ZKP_KZG_LAYOUT_CELLS");
    if (n_polys > rc->max_polys)
        return fail(ZKP_E_SIZE, "a batch of " + std::to_string(n_polys) + " polynomials on a recoverer made for " + std::to_string(rc->max_polys) +
                                    " (max_polys of zkp_kzg_recoverer_create_batch)");
    *none = n_polys == 0;
    return ZKP_OK;
}

// One call, everything on the device but the mask, on `st`; the caller is inside the recoverer's slot and has checked the arguments.
// batched: zkp_kzg_recover_cosets_batch* -- `polys` rows, row p of the coefficients at `stride` scalars times p, the evaluations in
// and out in `layout`, a word per row; else the single entries, whose launches are what they were before there was a batch.
int kzg_recover_locked(const zkp_kzg_recoverer* rc, const void* d_evals, const uint8_t* present, uint64_t m, size_t len, void* d_out_coeffs,
                       void* d_out_evals, uint32_t* d_inconsistent, hipStream_t st, bool batched = false, uint64_t polys = 1, size_t stride = 0,
                       int layout = KZG_RECOVER_NATURAL) {
    static_assert(KZG_RECOVER_NATURAL == ZKP_KZG_LAYOUT_NATURAL && KZG_RECOVER_CELLS == ZKP_KZG_LAYOUT_CELLS, "zkp_hip.h: the layouts of the plan");
    const KzgRecoverPlan plan = kzg_recover_plan_batch(rc->log_n, rc->log_l, rc->leaf_log, m, polys, layout, rc->max_polys);
    const uint64_t n = (uint64_t)1 << plan.log_n, r = (uint64_t)1 << plan.log_r;
    const bool cells = layout == KZG_RECOVER_CELLS;
    const uint32_t log_n = plan.log_n, log_l = plan.log_l, log_r = plan.log_r, P = (uint32_t)polys;
    // a pointwise pass of a batch: the n indices by the groups of rows; a pass through the tiles of the transposition
    const dim3 rows_grid(recover_blocks(n), (unsigned)kzg_recover_row_groups(polys));
    const dim3 tiles_grid((unsigned)kzg_recover_tiles(log_n, log_l), (unsigned)kzg_recover_row_groups(polys));
    char* base = static_cast<char*>(rc->work.p);
    auto fr_at = [&](size_t off) { return reinterpret_cast<Fr*>(base + off); };
    const uint8_t* d_mask = reinterpret_cast<const uint8_t*>(base + plan.sz.mask);
    const Fr* evals = static_cast<const Fr*>(d_evals);
    HIPCHK(hipMemsetAsync(d_inconsistent, 0, sizeof(uint32_t) * polys, st));
    if (m) {
        ZCHK(rc->stage.acquire());
        uint32_t* roots = reinterpret_cast<uint32_t*>(static_cast<char*>(rc->stage.buf.p) + plan.sz.stage_roots);
        uint64_t at = 0;
        for (uint64_t k = 0; k < r; k++)
            if (!present[k]) roots[at++] = (uint32_t)k;
        for (; at < plan.roots; at++) roots[at] = KZG_RECOVER_PAD_ROOT;
        uint8_t* mask = reinterpret_cast<uint8_t*>(rc->stage.buf.p) + plan.sz.stage_mask;
        for (uint64_t k = 0; k < r; k++) mask[k] = present[k] ? 1 : 0;
        HIPCHK(hipMemcpyAsync(base + plan.sz.roots, roots, 4 * plan.roots, hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(base + plan.sz.mask, mask, r, hipMemcpyHostToDevice, st));
        ZCHK(rc->stage.sent(st));
    }
    // two recorded phases while profiling is on: the vanishing polynomial (up to its values on both domains) and everything behind it
    std::unique_ptr<ProfScope> phase(new ProfScope(m ? "kzg_recover_zs" : "kzg_recover_rest", st));
    for (unsigned i = 0; i < plan.steps; i++) {
        const KzgRecoverStep s = kzg_recover_step(plan, i);
        const dim3 block(KZG_RECOVER_THREADS), grid(recover_blocks(s.lanes));
        if (s.kind == KZG_RECOVER_MUL) {
            phase.reset();
            phase.reset(new ProfScope("kzg_recover_rest", st));
        }
        switch (s.kind) {
        case KZG_RECOVER_LEAF:
            hipLaunchKernelGGL(recover_leaf_kernel, dim3((unsigned)s.batch), dim3((unsigned)s.lanes), 0, st,
                               reinterpret_cast<const uint32_t*>(base + s.in), rc->rho, (uint32_t)s.log, fr_at(s.out));
            break;
        case KZG_RECOVER_PAD:
            hipLaunchKernelGGL(recover_pad_kernel, grid, block, 0, st, fr_at(s.in), fr_at(s.out), (uint32_t)s.log, s.lanes);
            break;
        case KZG_RECOVER_TREE_FWD: ZCHK(recover_fr_rows(fr_at(s.in), s.log, s.batch, 0, st)); break;
        case KZG_RECOVER_PAIR:
            hipLaunchKernelGGL(recover_pair_kernel, grid, block, 0, st, fr_at(s.in), fr_at(s.out), (uint32_t)s.log, s.lanes);
            break;
        case KZG_RECOVER_TREE_INV: ZCHK(recover_fr_rows(fr_at(s.in), s.log, s.batch, 1, st)); break;
        case KZG_RECOVER_ZS:
            hipLaunchKernelGGL(recover_zs_kernel, grid, block, 0, st, fr_at(s.in), plan.pad, m, r, fr_at(plan.sz.zs0), fr_at(plan.sz.zs1));
            break;
        case KZG_RECOVER_ZS_FWD: ZCHK(run_ntt<Fr>(fr_at(s.in), s.log, 1, 0, nullptr, st)); break;
        case KZG_RECOVER_ZS_SHIFT: ZCHK(run_ntt<Fr>(fr_at(s.in), s.log, 1, 0, rc->gl, st)); break;
        case KZG_RECOVER_MUL:
            if (!batched) hipLaunchKernelGGL(recover_mul_kernel, grid, block, 0, st, evals, d_mask, fr_at(s.in), (uint32_t)plan.log_r, n, fr_at(s.out));
            else if (cells) hipLaunchKernelGGL(recover_mul_cells_kernel, tiles_grid, block, 0, st, evals, d_mask, fr_at(s.in), log_n, log_l, P, fr_at(s.out));
            else hipLaunchKernelGGL(recover_mul_batch_kernel, rows_grid, block, 0, st, evals, d_mask, fr_at(s.in), log_r, log_n, P, fr_at(s.out));
            break;
        case KZG_RECOVER_COPY:
            if (cells) {  // the transposition alone, then the transform where it went
                hipLaunchKernelGGL(recover_mul_cells_kernel, tiles_grid, block, 0, st, evals, d_mask, static_cast<const Fr*>(nullptr), log_n, log_l, P,
                                   fr_at(s.out));
                HIPCHK(hipGetLastError());
                ZCHK(run_ntt<Fr>(fr_at(s.out), s.log, (size_t)s.batch, 1, nullptr, st));
            } else {
                ZCHK(run_ntt<Fr>(evals, fr_at(s.out), s.log, (size_t)s.batch, 1, nullptr, st));
            }
            break;
        case KZG_RECOVER_N_INV: ZCHK(run_ntt<Fr>(fr_at(s.in), s.log, (size_t)s.batch, 1, nullptr, st)); break;
        case KZG_RECOVER_N_SHIFT: ZCHK(run_ntt<Fr>(fr_at(s.in), s.log, (size_t)s.batch, 0, rc->g, st)); break;
        case KZG_RECOVER_INV:
            HIPCHK(hipEventRecord(rc->fork, st));
            HIPCHK(hipStreamWaitEvent(rc->side, rc->fork, 0));
            hipLaunchKernelGGL(recover_inv_kernel, grid, block, 0, rc->side, fr_at(s.in), r, s.lanes);
            HIPCHK(hipEventRecord(rc->join, rc->side));
            break;
        case KZG_RECOVER_DIV:
            HIPCHK(hipStreamWaitEvent(st, rc->join, 0));
            if (!batched) hipLaunchKernelGGL(recover_div_kernel, grid, block, 0, st, fr_at(s.out), fr_at(s.in), (uint32_t)plan.log_r, n);
            else hipLaunchKernelGGL(recover_div_batch_kernel, rows_grid, block, 0, st, fr_at(s.out), fr_at(s.in), log_r, log_n, P);
            break;
        case KZG_RECOVER_N_UNSHIFT: ZCHK(run_ntt<Fr>(fr_at(s.in), s.log, (size_t)s.batch, 1, rc->g, st)); break;
        case KZG_RECOVER_TAIL:
            if (!batched)
                hipLaunchKernelGGL(recover_tail_kernel, grid, block, 0, st, fr_at(s.in), n, (uint64_t)len, static_cast<Fr*>(d_out_coeffs),
                                   static_cast<Fr*>(d_out_evals), d_inconsistent);
            else  // (cell layout: the padded rows stay in vec, where EVALS transforms them for CELLS_OUT)
                hipLaunchKernelGGL(recover_tail_batch_kernel, rows_grid, block, 0, st, fr_at(s.in), log_n, (uint64_t)len, (uint64_t)stride, P,
                                   static_cast<Fr*>(d_out_coeffs), !d_out_evals ? nullptr : cells ? fr_at(s.out) : static_cast<Fr*>(d_out_evals),
                                   d_inconsistent);
            break;
        case KZG_RECOVER_EVALS:
            if (d_out_evals) ZCHK(run_ntt<Fr>(cells ? fr_at(s.out) : static_cast<Fr*>(d_out_evals), s.log, (size_t)s.batch, 0, nullptr, st));
            break;
        default:  // KZG_RECOVER_CELLS_OUT
            if (d_out_evals) hipLaunchKernelGGL(recover_cells_out_kernel, tiles_grid, block, 0, st, fr_at(s.in), log_n, log_l, P, static_cast<Fr*>(d_out_evals));
            break;
        }
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

}  // namespace

extern "C" {

void zkp_kzg_recoverer_destroy(zkp_kzg_recoverer* rc) { handle_destroy(rc); }

int zkp_kzg_recoverer_create_batch(unsigned log_n, unsigned log_l, size_t max_polys, zkp_kzg_recoverer** out) try {
    if (!out) return fail(ZKP_E_ARG, "null argument");
    if (max_polys == 0 || max_polys > KZG_RECOVER_MAX_POLYS) return fail(ZKP_E_ARG, "a recoverer takes 1 .. 4096 polynomials per call (max_polys)");
    if (!kzg_recover_shape_ok(log_n, log_l)) return fail(ZKP_E_ARG, "a recoverer needs log_l < log_n <= 23");
    CTX_ENTER(-1);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    auto rc = handle_new<zkp_kzg_recoverer>(log_n, log_l);
    if (!rc) return fail(ZKP_E_NOMEM, "host allocation failed");
    static_assert(kKnobs[KNOB_KZG_RECOVER_LEAF_LOG].hi == KZG_RECOVER_MAX_LEAF_LOG && KZG_RECOVER_LEAF_LOG <= KZG_RECOVER_MAX_LEAF_LOG &&
                      kKnobs[KNOB_KZG_RECOVER_LEAF_LOG].lo == 1,
                  "knobs.hpp: recover_leaf_kernel is one workgroup of at most 2^KZG_RECOVER_MAX_LEAF_LOG lanes");
    rc->leaf_log = (unsigned)knob_int(KNOB_KZG_RECOVER_LEAF_LOG, KZG_RECOVER_LEAF_LOG);
    rc->max_polys = max_polys;
    const HFr g = HFr::from_u64(7);
    g.store(rc->g);
    g.pow_u64((uint64_t)1 << log_l).store(rc->gl);
    rc->rho = fr_pow2_table(fr_root_of_unity(log_n - log_l));
    const KzgRecoverSizes sz = kzg_recover_sizes_batch(log_n, log_l, max_polys);
    ZCHK(reserve_or_refuse(sz.total, KNOB_KZG_RECOVER_MAX_BYTES,
                           "zkp_kzg_recoverer_create: the workspace of " + std::to_string(sz.total) + " bytes (and " + std::to_string(sz.stage_total) +
                               " pinned)" + (max_polys > 1 ? " for max_polys " + std::to_string(max_polys) : std::string()) + " does not fit",
                           [&] { return rc->work.grow(sz.total) == hipSuccess && rc->stage.make(sz.stage_total) == ZKP_OK; }));
    ZCHK(rc->side.ensure(hipStreamNonBlocking));
    ZCHK(rc->fork.ensure(hipEventDisableTiming));
    ZCHK(rc->join.ensure(hipEventDisableTiming));
    {   // Everything a call builds on first use is built here, so that zkp_kzg_recover_cosets_dev does not allocate: the plans, tables
        // and scratch of its transforms -- of n with and without the shift, of r, and of every size and batch of the deepest tree
        char* base = static_cast<char*>(rc->work.p);
        HIPCHK(hipMemsetAsync(base, 0, sz.total, st));
        Fr* vec = reinterpret_cast<Fr*>(base + sz.vec);
        // (a call of one row and a call of max_polys may take different plans of a transform of n -- a batch of 2^19 elements or
        // more takes the wide passes -- and the larger needs the larger scratch: both are run)
        for (const size_t polys : {(size_t)1, max_polys}) {
            ZCHK(run_ntt<Fr>(vec, log_n, polys, 0, rc->g, st));
            ZCHK(run_ntt<Fr>(vec, log_n, polys, 1, rc->g, st));
            ZCHK(run_ntt<Fr>(vec, log_n, polys, 0, nullptr, st));
            ZCHK(run_ntt<Fr>(vec, log_n, polys, 1, nullptr, st));
            if (max_polys == 1) break;
        }
        ZCHK(run_ntt<Fr>(reinterpret_cast<Fr*>(base + sz.zs0), log_n - log_l, 1, 0, nullptr, st));
        ZCHK(run_ntt<Fr>(reinterpret_cast<Fr*>(base + sz.zs1), log_n - log_l, 1, 0, rc->gl, st));
        // (a transform's plan also depends on whether its batch reaches 2^19 elements: the trees of 2^17 and 2^18 roots are the
        // largest whose forward and inverse transforms, and whose inverse ones, stay below that)
        const uint64_t r = (uint64_t)1 << (log_n - log_l);
        for (uint64_t m : {r - 1, (uint64_t)1 << 18, (uint64_t)1 << 17}) {
            if (m >= r) continue;
            const KzgRecoverPlan deep = kzg_recover_plan(log_n, log_l, rc->leaf_log, m);
            for (unsigned i = 0; i < deep.steps; i++) {
                const KzgRecoverStep s = kzg_recover_step(deep, i);
                if (s.kind == KZG_RECOVER_TREE_FWD || s.kind == KZG_RECOVER_TREE_INV)
                    ZCHK(recover_fr_rows(reinterpret_cast<Fr*>(base + s.in), s.log, s.batch, s.kind == KZG_RECOVER_TREE_INV, st));
            }
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    *out = rc.release();
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_kzg_recoverer_create(unsigned log_n, unsigned log_l, zkp_kzg_recoverer** out) { return zkp_kzg_recoverer_create_batch(log_n, log_l, 1, out); }

int zkp_kzg_recover_cosets_batch_dev(const zkp_kzg_recoverer* rc, const void* d_evals, size_t n_polys, const uint8_t* present, size_t len, size_t stride,
                                     int layout, void* d_out_coeffs, void* d_out_evals, uint32_t* d_inconsistent, void* stream) try {
    uint64_t m = 0;
    bool none = false;
    ZCHK(recover_batch_args(rc, d_evals, n_polys, present, len, stride, layout, d_out_coeffs, d_inconsistent, &m, &none));
    if (none) return ZKP_OK;
    CTX_ENTER(rc->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_recover_locked(rc, d_evals, present, m, len, d_out_coeffs, d_out_evals, d_inconsistent, st, true, n_polys, stride, layout);
} ZKP_CATCH_INT

int zkp_kzg_recover_cosets_batch(const zkp_kzg_recoverer* rc, const uint64_t* evals, size_t n_polys, const uint8_t* present, size_t len, int layout,
                                 uint64_t* out_coeffs, uint64_t* out_evals, uint8_t* consistent) try {
    uint64_t m = 0;
    bool none = false;
    ZCHK(recover_batch_args(rc, evals, n_polys, present, len, len, layout, out_coeffs, consistent, &m, &none));
    if (none) return ZKP_OK;
    CTX_ENTER(rc->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t n = (size_t)1 << rc->log_n, P = n_polys;
    void* ws = nullptr;  // evaluations in | coefficients | evaluations out | the words
    ZCHK(slot_workspace(P * (32 * n + 32 * len + 32 * n + 4), "zkp_kzg_recover_cosets_batch", &ws));
    char* d_evals = static_cast<char*>(ws);
    char* d_coeffs = d_evals + 32 * n * P;
    char* d_out_evals = d_coeffs + 32 * len * P;
    uint32_t* d_flags = reinterpret_cast<uint32_t*>(d_out_evals + 32 * n * P);
    HIPCHK(hipMemcpyAsync(d_evals, evals, 32 * n * P, hipMemcpyHostToDevice, st));
    ZCHK(kzg_recover_locked(rc, d_evals, present, m, len, d_coeffs, out_evals ? d_out_evals : nullptr, d_flags, st, true, P, len, layout));
    std::vector<uint32_t> flags(P, 0);
    HIPCHK(hipMemcpyAsync(out_coeffs, d_coeffs, 32 * len * P, hipMemcpyDeviceToHost, st));
    if (out_evals) HIPCHK(hipMemcpyAsync(out_evals, d_out_evals, 32 * n * P, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(flags.data(), d_flags, 4 * P, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (size_t p = 0; p < P; p++) consistent[p] = flags[p] ? 0 : 1;
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_kzg_recover_cosets_dev(const zkp_kzg_recoverer* rc, const void* d_evals, const uint8_t* present, size_t len, void* d_out_coeffs,
                               void* d_out_evals, uint32_t* d_inconsistent, void* stream) try {
    uint64_t m = 0;
    ZCHK(recover_args(rc, d_evals, present, len, d_out_coeffs, d_inconsistent, &m));
    CTX_ENTER(rc->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_recover_locked(rc, d_evals, present, m, len, d_out_coeffs, d_out_evals, d_inconsistent, st);
} ZKP_CATCH_INT

int zkp_kzg_recover_cosets(const zkp_kzg_recoverer* rc, const uint64_t* evals, const uint8_t* present, size_t len, uint64_t* out_coeffs,
                           uint64_t* out_evals, int* consistent) try {
    uint64_t m = 0;
    ZCHK(recover_args(rc, evals, present, len, out_coeffs, consistent, &m));
    CTX_ENTER(rc->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t n = (size_t)1 << rc->log_n;
    void* ws = nullptr;  // evaluations in | coefficients | evaluations out | the word
    ZCHK(slot_workspace(32 * n + 32 * len + 32 * n + 32, "zkp_kzg_recover_cosets", &ws));
    char* d_evals = static_cast<char*>(ws);
    char* d_coeffs = d_evals + 32 * n;
    char* d_out_evals = d_coeffs + 32 * len;
    uint32_t* d_flag = reinterpret_cast<uint32_t*>(d_out_evals + 32 * n);
    HIPCHK(hipMemcpyAsync(d_evals, evals, 32 * n, hipMemcpyHostToDevice, st));
    ZCHK(kzg_recover_locked(rc, d_evals, present, m, len, d_coeffs, out_evals ? d_out_evals : nullptr, d_flag, st));
    uint32_t flag = 0;
    HIPCHK(hipMemcpyAsync(out_coeffs, d_coeffs, 32 * len, hipMemcpyDeviceToHost, st));
    if (out_evals) HIPCHK(hipMemcpyAsync(out_evals, d_out_evals, 32 * n, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(&flag, d_flag, sizeof flag, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *consistent = flag ? 0 : 1;
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
