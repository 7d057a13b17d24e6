// kzg_evals_host.inc -- zkp_kzg_eval_opener_*, zkp_kzg_commit_evals_batch*, zkp_kzg_open_evals_batch*, zkp_kzg_open_evals_field_dev
// and zkp_selftest_fr_inverse_dev: commitments and openings of a batch of polynomials given by their values on the domain, with no
// transform (included at the end of api.hip, after kzg_cells_host.inc).  The formulas, every launch, index and size are in
// kzg_evals_plan.hpp, the kernels in kzg_evals.hpp; the points are sums of the MSM driver over the borrowed Lagrange-basis handle.

struct zkp_kzg_eval_opener : KzgHandle {  // work: kzg_evals_sizes
    int order = KZG_EVALS_NATURAL;
    uint64_t max_polys = 1;
    const zkp_bases* lagrange = nullptr;  // borrowed: [L_j(s)]_1, j < n, in natural order
    Fr w, ninv;                           // the root of the domain and 1 / n, Montgomery
    KzgEvalsSizes sz;
};

namespace {

// Everything of a call that is checked before anything is launched; *none: an empty batch, nothing to do
int evals_args(const zkp_kzg_eval_opener* o, bool nulls, size_t n_polys, bool* none) {
    if (!o || (n_polys && nulls)) return fail(ZKP_E_ARG, "null argument");
    if (n_polys > o->max_polys)
        return fail(ZKP_E_SIZE, "a batch of " + std::to_string(n_polys) + " polynomials on an opener made for " + std::to_string(o->max_polys) +
                                    " (max_polys of zkp_kzg_eval_opener_create)");
    *none = n_polys == 0;
    return ZKP_OK;
}

// The field half on `st`: y and the quotients in natural order from resident rows and points.  The caller is inside the opener's slot
// and has checked the arguments.  Walks kzg_evals_step and launches nothing else; allocates nothing, waits for nothing.
int kzg_evals_field_locked(const zkp_kzg_eval_opener* o, const void* d_evals, size_t n_polys, const void* d_z, void* d_y, void* d_quotient,
                           hipStream_t st) {
    static_assert(KZG_EVALS_NATURAL == ZKP_KZG_ORDER_NATURAL && KZG_EVALS_BITREV == ZKP_KZG_ORDER_BITREV, "zkp_hip.h: the orders of the plan");
    static_assert(kKnobs[KNOB_KZG_EVALS_INVERSE].lo == 0 && kKnobs[KNOB_KZG_EVALS_INVERSE].hi == 1 && (KZG_EVALS_INVERSE == 0 || KZG_EVALS_INVERSE == 1),
                  "knobs.hpp: the two inversions of kzg_evals.hpp");
    const int method = (int)knob_int(KNOB_KZG_EVALS_INVERSE, KZG_EVALS_INVERSE);
    char* base = static_cast<char*>(o->work.p);
    const Fr* roots = reinterpret_cast<const Fr*>(base + o->sz.roots);
    Fr* dinv = reinterpret_cast<Fr*>(base + o->sz.dinv);
    Fr* partial = reinterpret_cast<Fr*>(base + o->sz.partial);
    Fr* partial2 = reinterpret_cast<Fr*>(base + o->sz.partial2);
    uint32_t* hit = reinterpret_cast<uint32_t*>(base + o->sz.hit);
    const Fr* evals = static_cast<const Fr*>(d_evals);
    const Fr* z = static_cast<const Fr*>(d_z);
    Fr* y = static_cast<Fr*>(d_y);
    Fr* quotient = static_cast<Fr*>(d_quotient);
    const uint32_t log_n = o->log_n;
    ProfScope phase("kzg_evals_field", st);
    for (unsigned i = 0; i < KZG_EVALS_STEPS; i++) {
        const KzgEvalsStep s = kzg_evals_step(log_n, n_polys, i);
        const dim3 grid(s.grid_x, s.grid_y), block(KZG_EVALS_THREADS);
        switch (s.kind) {
        case KZG_EVALS_PRESET: HIPCHK(hipMemsetAsync(hit, 0xFF, 4 * n_polys, st)); break;
        case KZG_EVALS_INVERT:
            if (method) hipLaunchKernelGGL(evals_invert_kernel<1>, grid, block, 0, st, evals, z, roots, log_n, o->order, dinv, hit, partial);
            else hipLaunchKernelGGL(evals_invert_kernel<0>, grid, block, 0, st, evals, z, roots, log_n, o->order, dinv, hit, partial);
            break;
        case KZG_EVALS_Y: hipLaunchKernelGGL(evals_y_kernel, grid, block, 0, st, evals, z, partial, hit, log_n, o->order, o->ninv, y); break;
        case KZG_EVALS_QUOTIENT:
            hipLaunchKernelGGL(evals_quotient_kernel, grid, block, 0, st, evals, roots, dinv, y, hit, log_n, o->order, quotient, partial2);
            break;
        case KZG_EVALS_QM: hipLaunchKernelGGL(evals_qm_kernel, grid, block, 0, st, roots, partial2, hit, log_n, quotient); break;
        }
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

// out[p] = the MSM of row p of `rows` (natural order) over the Lagrange handle, p < n_polys, as affine points in host memory:
// groups of kzg_evals_group, one batch_to_affine for all.  Blocks.
int kzg_evals_points_locked(const zkp_kzg_eval_opener* o, const Fr* rows, size_t n_polys, hipStream_t st, uint64_t* out_xy, uint8_t* out_is_inf) {
    static_assert(KZG_EVALS_MSM_GROUP == MSM_MAX_BATCH && 2 * KZG_EVALS_MSM_GROUP_SPLIT == MSM_MAX_BATCH, "msm_plan.hpp: the MSMs of one pass");
    const size_t n = (size_t)1 << o->log_n;
    const bool split = o->lagrange->pre_glv != 0;
    std::vector<HXyzz> sums(n_polys);
    {
        ProfScope phase("kzg_evals_points", st);
        for (uint64_t k = 0; k < kzg_evals_groups(n_polys, split); k++) {
            const KzgEvalsGroup g = kzg_evals_group(n_polys, split, k);
            const Fr* vectors[MSM_MAX_BATCH];
            for (uint64_t m = 0; m < g.count; m++) vectors[m] = rows + ((g.first + m) << o->log_n);
            ZCHK(msm_partial_batch(o->lagrange, vectors, (size_t)g.count, n, st, sums.data() + g.first));
        }
    }
    batch_to_affine(sums.data(), n_polys, out_xy, out_is_inf);
    return ZKP_OK;
}

// The rows as the scalars of the commitments: themselves for a natural-order handle, gathered into the workspace otherwise
int kzg_evals_commit_locked(const zkp_kzg_eval_opener* o, const void* d_evals, size_t n_polys, hipStream_t st, uint64_t* out_xy, uint8_t* out_is_inf) {
    const Fr* rows = static_cast<const Fr*>(d_evals);
    if (o->order != KZG_EVALS_NATURAL) {
        Fr* nat = reinterpret_cast<Fr*>(static_cast<char*>(o->work.p) + o->sz.rows);
        const uint64_t n = (uint64_t)1 << o->log_n;
        hipLaunchKernelGGL(evals_gather_kernel, dim3((unsigned)((n + KZG_EVALS_THREADS - 1) / KZG_EVALS_THREADS), (unsigned)n_polys),
                           dim3(KZG_EVALS_THREADS), 0, st, rows, (uint32_t)o->log_n, o->order, nat);
        HIPCHK(hipGetLastError());
        rows = nat;
    }
    return kzg_evals_points_locked(o, rows, n_polys, st, out_xy, out_is_inf);
}

int kzg_evals_open_locked(const zkp_kzg_eval_opener* o, const void* d_evals, size_t n_polys, const void* d_z, hipStream_t st, uint64_t* out_xy,
                          uint8_t* out_is_inf, uint64_t* out_y) {
    char* base = static_cast<char*>(o->work.p);
    Fr* y = reinterpret_cast<Fr*>(base + o->sz.y);
    Fr* quotient = reinterpret_cast<Fr*>(base + o->sz.rows);
    ZCHK(kzg_evals_field_locked(o, d_evals, n_polys, d_z, y, quotient, st));
    HIPCHK(hipMemcpyAsync(out_y, y, 32 * n_polys, hipMemcpyDeviceToHost, st));
    const int rc = kzg_evals_points_locked(o, quotient, n_polys, st, out_xy, out_is_inf);
    HIPCHK(hipStreamSynchronize(st));  // (also behind a failed MSM: the copy into the caller's memory is not left in flight)
    return rc;
}

}  // namespace

extern "C" {

void zkp_kzg_eval_opener_destroy(zkp_kzg_eval_opener* o) { handle_destroy(o); }

int zkp_kzg_eval_opener_create(const zkp_bases* lagrange, unsigned log_n, int order, size_t max_polys, zkp_kzg_eval_opener** out) try {
    if (!lagrange || !out) return fail(ZKP_E_ARG, "null argument");
    if (!kzg_evals_shape_ok(log_n)) return fail(ZKP_E_ARG, "an evaluation-form opener needs 1 <= log_n <= 24");
    if (order != KZG_EVALS_NATURAL && order != KZG_EVALS_BITREV)
        return fail(ZKP_E_ARG, "order " + std::to_string(order) + " is neither ZKP_KZG_ORDER_NATURAL nor ZKP_KZG_ORDER_BITREV");
    if (max_polys == 0 || max_polys > KZG_EVALS_MAX_POLYS)
        return fail(ZKP_E_ARG, "an evaluation-form opener takes 1 .. 4096 polynomials per call (max_polys)");
    if (!lagrange->shards.empty())
        return fail(ZKP_E_ARG, "bases are sharded over several devices: an evaluation-form opener takes single-device bases "
                               "(zkp_set_device + zkp_g1_bases_lagrange make single-device bases)");
    const uint64_t n = (uint64_t)1 << log_n;
    if (lagrange->n < n) return fail(ZKP_E_SIZE, "the Lagrange basis has " + std::to_string(lagrange->n) + " points, fewer than 2^log_n = " + std::to_string(n));
    CTX_ENTER(lagrange->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    auto o = handle_new<zkp_kzg_eval_opener>(log_n, 0);
    if (!o) return fail(ZKP_E_NOMEM, "host allocation failed");
    o->order = order;
    o->max_polys = max_polys;
    o->lagrange = lagrange;
    const HFr w = fr_root_of_unity(log_n);
    o->w = HostField<Fr>::dev(w);
    o->ninv = HostField<Fr>::dev(HFr::from_u64(n).inverse_fermat());
    o->sz = kzg_evals_sizes(log_n, max_polys);
    ZCHK(reserve_or_refuse(o->sz.total, KNOB_KZG_EVALS_MAX_BYTES,
                           "zkp_kzg_eval_opener_create: the workspace of " + std::to_string(o->sz.total) + " bytes" +
                               (max_polys > 1 ? " for max_polys " + std::to_string(max_polys) : std::string()) + " does not fit",
                           [&] { return o->work.grow(o->sz.total) == hipSuccess; }));
    hipLaunchKernelGGL(evals_roots_kernel, dim3((unsigned)((n + KZG_EVALS_THREADS - 1) / KZG_EVALS_THREADS)), dim3(KZG_EVALS_THREADS), 0, st, o->w,
                       (uint32_t)log_n, reinterpret_cast<Fr*>(static_cast<char*>(o->work.p) + o->sz.roots));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));
    *out = o.release();
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_kzg_open_evals_field_dev(const zkp_kzg_eval_opener* o, const void* d_evals, size_t n_polys, const void* d_z, void* d_out_y,
                                 void* d_out_quotient, void* stream) try {
    bool none = false;
    ZCHK(evals_args(o, !d_evals || !d_z || !d_out_y || !d_out_quotient, n_polys, &none));
    if (none) return ZKP_OK;
    CTX_ENTER(o->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_evals_field_locked(o, d_evals, n_polys, d_z, d_out_y, d_out_quotient, st);
} ZKP_CATCH_INT

int zkp_kzg_open_evals_batch_dev(const zkp_kzg_eval_opener* o, const void* d_evals, size_t n_polys, const void* d_z, void* stream,
                                 uint64_t* out_xy, uint8_t* out_is_inf, uint64_t* out_y) try {
    bool none = false;
    ZCHK(evals_args(o, !d_evals || !d_z || !out_xy || !out_is_inf || !out_y, n_polys, &none));
    if (none) return ZKP_OK;
    CTX_ENTER(o->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_evals_open_locked(o, d_evals, n_polys, d_z, st, out_xy, out_is_inf, out_y);
} ZKP_CATCH_INT

int zkp_kzg_open_evals_batch(const zkp_kzg_eval_opener* o, const uint64_t* evals, size_t n_polys, const uint64_t* z, uint64_t* out_xy,
                             uint8_t* out_is_inf, uint64_t* out_y) try {
    bool none = false;
    ZCHK(evals_args(o, !evals || !z || !out_xy || !out_is_inf || !out_y, n_polys, &none));
    if (none) return ZKP_OK;
    CTX_ENTER(o->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t n = (size_t)1 << o->log_n, P = n_polys;
    void* ws = nullptr;  // the rows | the points
    ZCHK(slot_workspace(32 * n * P + 32 * P, "zkp_kzg_open_evals_batch", &ws));
    char* d_evals = static_cast<char*>(ws);
    char* d_z = d_evals + 32 * n * P;
    HIPCHK(hipMemcpyAsync(d_evals, evals, 32 * n * P, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_z, z, 32 * P, hipMemcpyHostToDevice, st));
    return kzg_evals_open_locked(o, d_evals, P, d_z, st, out_xy, out_is_inf, out_y);
} ZKP_CATCH_INT

int zkp_kzg_commit_evals_batch_dev(const zkp_kzg_eval_opener* o, const void* d_evals, size_t n_polys, void* stream, uint64_t* out_xy,
                                   uint8_t* out_is_inf) try {
    bool none = false;
    ZCHK(evals_args(o, !d_evals || !out_xy || !out_is_inf, n_polys, &none));
    if (none) return ZKP_OK;
    CTX_ENTER(o->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_evals_commit_locked(o, d_evals, n_polys, st, out_xy, out_is_inf);
} ZKP_CATCH_INT

int zkp_kzg_commit_evals_batch(const zkp_kzg_eval_opener* o, const uint64_t* evals, size_t n_polys, uint64_t* out_xy, uint8_t* out_is_inf) try {
    bool none = false;
    ZCHK(evals_args(o, !evals || !out_xy || !out_is_inf, n_polys, &none));
    if (none) return ZKP_OK;
    CTX_ENTER(o->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t n = (size_t)1 << o->log_n, P = n_polys;
    void* ws = nullptr;
    ZCHK(slot_workspace(32 * n * P, "zkp_kzg_commit_evals_batch", &ws));
    HIPCHK(hipMemcpyAsync(ws, evals, 32 * n * P, hipMemcpyHostToDevice, st));
    return kzg_evals_commit_locked(o, ws, P, st, out_xy, out_is_inf);
} ZKP_CATCH_INT

int zkp_selftest_fr_inverse_dev(const void* d_in, size_t n, int method, void* d_out, void* stream) try {
    if (n && (!d_in || !d_out)) return fail(ZKP_E_ARG, "null argument");
    if (method != 0 && method != 1) return fail(ZKP_E_ARG, "method must be 0 (division steps) or 1 (the Fermat power)");
    if (n > (size_t)1 << 24) return fail(ZKP_E_SIZE, "a self-test takes at most 2^24 cases");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    hipLaunchKernelGGL(fr_inverse_selftest_kernel, dim3((unsigned)((n + FR_INVERSE_SELFTEST_THREADS - 1) / FR_INVERSE_SELFTEST_THREADS)),
                       dim3(FR_INVERSE_SELFTEST_THREADS), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const Fr*>(d_in),
                       reinterpret_cast<Fr*>(d_out), (uint64_t)n, method);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
