// kzg_cells_host.inc -- zkp_kzg_cell_verifier_*, zkp_kzg_verify_cells* and zkp_kzg_cells_aggregate_dev: any number of cells of any
// number of commitments behind one pairing check (included at the end of api.hip, after kzg_recover_host.inc).  The equation, the
// grouping tables and every size are in kzg_cells_plan.hpp, the kernels in kzg_cells.hpp; the points are validated with the kernels
// of g1_check.hpp and summed by the MSM driver; the two pairings are the host's (verify_host.inc).

struct zkp_kzg_cell_verifier : KzgHandle {  // work: kzg_cells_sizes
    unsigned chunk_log = 0;  // ZKP_KZG_CELLS_CHUNK_LOG as it was at creation
    uint64_t max_cells = 0, max_commits = 0;
    const zkp_bases* srs = nullptr;  // borrowed: [(sum rho_i I_i)(s)]_1 is an MSM of l terms over it
    G2Aff g2sl = G2Aff::infinity();  // [s^l]_2, validated at creation
    FrPow2 rho;                      // the powers of w^l
    Fr r_mont;                       // r = n / l as a residue
    KzgCellsSizes sz;
    mutable HostStage stage;                // the tables on their way to the device
    mutable std::vector<uint32_t> scratch;  // where the sorts count (host)
};

namespace {

const char* const kG1StatusWord[4] = {"valid", "canonical", "curve", "subgroup"};

unsigned cells_blocks(uint64_t lanes) { return (unsigned)((lanes + KZG_CELLS_THREADS - 1) / KZG_CELLS_THREADS); }

// Everything of a call that is checked before anything is launched
int cells_args(const zkp_kzg_cell_verifier* v, size_t n_commits, size_t n_cells, const uint32_t* commit_index, const uint32_t* coset_index) {
    if (n_cells > v->max_cells)
        return fail(ZKP_E_SIZE, std::to_string(n_cells) + " cells: the verifier was made for " + std::to_string(v->max_cells));
    if (n_commits > v->max_commits)
        return fail(ZKP_E_SIZE, std::to_string(n_commits) + " commitments: the verifier was made for " + std::to_string(v->max_commits));
    const uint64_t r = (uint64_t)1 << (v->log_n - v->log_l);
    for (size_t i = 0; i < n_cells; i++) {
        if (coset_index[i] >= r)
            return fail(ZKP_E_ARG, "cell " + std::to_string(i) + ": coset " + std::to_string(coset_index[i]) + " of " + std::to_string(r));
        if (commit_index[i] >= n_commits)
            return fail(ZKP_E_ARG, "cell " + std::to_string(i) + ": commitment " + std::to_string(commit_index[i]) + " of " +
                                       std::to_string(n_commits));
    }
    return ZKP_OK;
}

// The field half on `st`: the three outputs from resident evaluations and weights.  The caller is inside the verifier's slot and has
// checked the arguments.  Waits for nothing but the previous call's copy out of the staging buffer; allocates nothing.
int kzg_cells_aggregate_locked(const zkp_kzg_cell_verifier* v, size_t n_commits, size_t n_cells, const uint32_t* commit_index,
                               const uint32_t* coset_index, const void* d_evals, const void* d_weights, void* d_out_interp,
                               void* d_out_commit_weights, void* d_out_proof_scalars, hipStream_t st) {
    const unsigned log_l = v->log_l, log_r = v->log_n - log_l;
    const uint64_t n = (uint64_t)1 << v->log_n, l = (uint64_t)1 << log_l;
    char* base = static_cast<char*>(v->work.p);
    ZCHK(v->stage.acquire());
    uint32_t* table = static_cast<uint32_t*>(v->stage.buf.p);
    const KzgCellsTables t = kzg_cells_tables(v->log_n, log_l, v->chunk_log, commit_index, coset_index, n_cells, n_commits, v->scratch.data(), table);
    if (t.words > v->sz.table_words) return fail(ZKP_E_DEVICE, "internal error: the tables of a call outgrew the verifier's");
    HIPCHK(hipMemcpyAsync(base + v->sz.table, table, 4 * t.words, hipMemcpyHostToDevice, st));
    ZCHK(v->stage.sent(st));
    const uint32_t* d_table = reinterpret_cast<const uint32_t*>(base + v->sz.table);
    Fr* a = reinterpret_cast<Fr*>(base + v->sz.a);
    Fr* partial = reinterpret_cast<Fr*>(base + v->sz.partial);
    Fr* cpartial = reinterpret_cast<Fr*>(base + v->sz.cpartial);
    const Fr* evals = static_cast<const Fr*>(d_evals);
    const Fr* weights = static_cast<const Fr*>(d_weights);
    const dim3 block(KZG_CELLS_THREADS);
    for (unsigned i = 0; i < KZG_CELLS_STEPS; i++) {
        const KzgCellsStep s = kzg_cells_step(log_l, t, i);
        const dim3 grid(cells_blocks(s.lanes));
        switch (s.kind) {
        case KZG_CELLS_ZERO: HIPCHK(hipMemsetAsync(a, 0, 32 * n, st)); break;
        case KZG_CELLS_AGGREGATE:
            if (s.lanes)
                hipLaunchKernelGGL(cells_aggregate_kernel, grid, block, 0, st, evals, weights, d_table + t.by_coset, d_table + t.chunk_start,
                                   (uint32_t)log_l, log_l >= 6 ? 1u : 0u, s.lanes, partial);
            break;
        case KZG_CELLS_COMBINE:
            if (s.lanes)
                hipLaunchKernelGGL(cells_combine_kernel, grid, block, 0, st, partial, d_table + t.used_coset, d_table + t.seg_chunk,
                                   (uint32_t)log_l, (uint32_t)log_r, s.lanes, a);
            break;
        case KZG_CELLS_NTT: ZCHK(run_ntt<Fr>(a, v->log_n, 1, 1, nullptr, st)); break;
        case KZG_CELLS_TAIL:
            hipLaunchKernelGGL(cells_tail_kernel, grid, block, 0, st, a, v->r_mont, l, static_cast<Fr*>(d_out_interp));
            break;
        case KZG_CELLS_SCALARS:
            if (s.lanes)
                hipLaunchKernelGGL(cells_scalars_kernel, grid, block, 0, st, weights, d_table + t.cell_coset, d_table + t.by_commit,
                                   d_table + t.cchunk_start, v->rho, t.cells, t.cchunks, static_cast<Fr*>(d_out_proof_scalars), cpartial);
            break;
        case KZG_CELLS_COMMITS:
            if (s.lanes)
                hipLaunchKernelGGL(cells_commits_kernel, grid, block, 0, st, cpartial, d_table + t.cseg_chunk, t.commits,
                                   static_cast<Fr*>(d_out_commit_weights));
            break;
        }
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

// One verification with everything but the index arrays resident, on `st`; blocks (the pairings are the host's).  The caller is
// inside the verifier's slot and has checked the arguments; n_cells > 0.
int kzg_verify_cells_locked(const zkp_kzg_cell_verifier* v, const void* d_commits_xy, const uint8_t* d_commits_inf, size_t n_commits,
                            size_t n_cells, const uint32_t* commit_index, const uint32_t* coset_index, const void* d_evals,
                            const void* d_proofs_xy, const uint8_t* d_proofs_inf, const void* d_weights, hipStream_t st, int* accepted) {
    const size_t M = n_commits, N = n_cells, l = (size_t)1 << v->log_l;
    char* base = static_cast<char*>(v->work.p);
    Fr* interp = reinterpret_cast<Fr*>(base + v->sz.interp);
    Fr* sc_right = reinterpret_cast<Fr*>(base + v->sz.sc_right);
    Fr* sc_left = reinterpret_cast<Fr*>(base + v->sz.sc_left);
    {   // [sum rho per commitment ..., rho_i c_i ...] and [0 ..., rho_i ...], and the coefficients of sum rho_i I_i
        ProfScope phase("kzg_cells_field", st);
        ZCHK(kzg_cells_aggregate_locked(v, M, N, commit_index, coset_index, d_evals, d_weights, interp, sc_right, sc_right + M, st));
        HIPCHK(hipMemsetAsync(sc_left, 0, 32 * M, st));
        HIPCHK(hipMemcpyAsync(sc_left + M, d_weights, 32 * N, hipMemcpyDeviceToDevice, st));
    }
    HXyzz sums[2], at_s;
    {
        ProfScope phase("kzg_cells_points", st);
        // every point is checked before any is used: the batched equation says nothing about points outside G1
        G1CheckReport* d_rep = reinterpret_cast<G1CheckReport*>(base + v->sz.report);
        static const G1CheckReport kEmpty[2] = {kEmptyReport, kEmptyReport};
        G1CheckReport rep[2];
        HIPCHK(hipMemcpyAsync(d_rep, kEmpty, sizeof kEmpty, hipMemcpyHostToDevice, st));
        ZCHK(g1_check_launch(g1_validate_raw_kernel, 96, d_commits_xy, d_commits_inf, M, 0, nullptr, d_rep, st));
        ZCHK(g1_check_launch(g1_validate_raw_kernel, 96, d_proofs_xy, d_proofs_inf, N, 0, nullptr, d_rep + 1, st));
        HIPCHK(hipMemcpyAsync(rep, d_rep, sizeof rep, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        for (int k = 0; k < 2; k++)
            if (rep[k].first != ~0ull)
                return fail(ZKP_E_ARG, std::string(k ? "proofs[" : "commits[") + std::to_string(rep[k].first >> 2) + "] is not a point of G1 (" +
                                           kG1StatusWord[rep[k].first & 3] + ")");
        // the transient handle over [C_0 .. C_(M-1), W_0 .. W_(N-1)], unexpanded
        zkp_bases* raw = nullptr;
        ZCHK(bases_alloc(M + N, true, &raw));
        std::unique_ptr<zkp_bases, void (*)(zkp_bases*)> pts(raw, zkp_g1_bases_destroy);
        uint4* internal = static_cast<uint4*>(pts->d_xy.p);
        hipLaunchKernelGGL(g1_to_internal_kernel, dim3((unsigned)((M + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS), 0, st,
                           static_cast<const uint4*>(d_commits_xy), (uint64_t)M, internal);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(g1_to_internal_kernel, dim3((unsigned)((N + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS), 0, st,
                           static_cast<const uint4*>(d_proofs_xy), (uint64_t)N, internal + 8 * M);
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemsetAsync(pts->d_inf.p, 0, M + N, st));
        if (d_commits_inf) HIPCHK(hipMemcpyAsync(pts->d_inf.get(), d_commits_inf, M, hipMemcpyDeviceToDevice, st));
        if (d_proofs_inf) HIPCHK(hipMemcpyAsync(pts->d_inf.get() + M, d_proofs_inf, N, hipMemcpyDeviceToDevice, st));
        const Fr* vectors[2] = {sc_right, sc_left};
        int rc = msm_partial_batch(pts.get(), vectors, 2, M + N, st, sums);
        if (rc == ZKP_OK) rc = msm_partial(v->srs, interp, l, st, &at_s);
        if (rc != ZKP_OK) {
            (void)hipStreamSynchronize(st);  // the handle goes before this entry returns: nothing may still read it
            return rc;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    const HXyzz right = sums[0].add(at_s.negate());
    *accepted = pairings_equal(sums[1], v->g2sl, right, G2Aff::generator()) ? 1 : 0;
    prof_host("kzg_cells_pairing", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return ZKP_OK;
}

}  // namespace

extern "C" {

void zkp_kzg_cell_verifier_destroy(zkp_kzg_cell_verifier* v) { handle_destroy(v); }

int zkp_kzg_cell_verifier_create(const zkp_bases* srs, const uint64_t g2_sl_xy[24], unsigned log_n, unsigned log_l, size_t max_cells,
                                 size_t max_commits, zkp_kzg_cell_verifier** out) try {
    if (!srs || !g2_sl_xy || !out) return fail(ZKP_E_ARG, "null argument");
    if (!kzg_cells_shape_ok(log_n, log_l)) return fail(ZKP_E_ARG, "a cell verifier needs log_l < log_n <= 23");
    if (!max_cells || !max_commits || max_cells > KZG_CELLS_MAX_COUNT || max_commits > KZG_CELLS_MAX_COUNT)
        return fail(ZKP_E_ARG, "a cell verifier is made for 1 .. 2^30 cells and as many commitments");
    if (!srs->shards.empty()) return fail(ZKP_E_ARG, "bases are sharded over several devices: a cell verifier takes a single-device SRS "
                                                            "(zkp_set_device + zkp_g1_bases_create* make single-device bases)");
    const uint64_t n = (uint64_t)1 << log_n, l = (uint64_t)1 << log_l, r = n >> log_l;
    if (srs->n < l) return fail(ZKP_E_SIZE, "the SRS has fewer than 2^log_l points");
    G2Aff g2sl = G2Aff::infinity();
    ZCHK(g2_validate(g2_sl_xy, "[s^l]_2", &g2sl));
    CTX_ENTER(srs->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    auto v = handle_new<zkp_kzg_cell_verifier>(log_n, log_l);
    if (!v) return fail(ZKP_E_NOMEM, "host allocation failed");
    static_assert(kKnobs[KNOB_KZG_CELLS_CHUNK_LOG].hi == KZG_CELLS_MAX_CHUNK_LOG && KZG_CELLS_CHUNK_LOG <= KZG_CELLS_MAX_CHUNK_LOG &&
                      kKnobs[KNOB_KZG_CELLS_CHUNK_LOG].lo == 0,
                  "knobs.hpp: the chunk log of kzg_cells_plan.hpp");
    v->chunk_log = (unsigned)knob_int(KNOB_KZG_CELLS_CHUNK_LOG, KZG_CELLS_CHUNK_LOG);
    v->max_cells = max_cells;
    v->max_commits = max_commits;
    v->srs = srs;
    v->g2sl = g2sl;
    v->rho = fr_pow2_table(fr_root_of_unity(log_n - log_l));
    v->r_mont = HostField<Fr>::dev(HFr::from_u64(r));
    v->sz = kzg_cells_sizes(log_n, log_l, v->chunk_log, max_cells, max_commits);
    const KzgCellsSizes& sz = v->sz;
    ZCHK(reserve_or_refuse(sz.total, KNOB_COUNT,
                           "zkp_kzg_cell_verifier_create: the workspace of " + std::to_string(sz.total) + " bytes (and " +
                               std::to_string(sz.stage_total) + " pinned) does not fit",
                           [&] { return v->work.grow(sz.total) == hipSuccess && v->stage.make(sz.stage_total) == ZKP_OK; }));
    v->scratch.resize(sz.scratch_words);
    // the plan, table and scratch of the one transform are built here, not by the first call
    HIPCHK(hipMemsetAsync(v->work.p, 0, sz.partial, st));
    ZCHK(run_ntt<Fr>(reinterpret_cast<Fr*>(static_cast<char*>(v->work.p) + sz.a), log_n, 1, 1, nullptr, st));
    HIPCHK(hipStreamSynchronize(st));
    *out = v.release();
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_kzg_cells_aggregate_dev(const zkp_kzg_cell_verifier* v, size_t n_commits, size_t n_cells, const uint32_t* commit_index,
                                const uint32_t* coset_index, const void* d_evals, const void* d_weights, void* d_out_interp,
                                void* d_out_commit_weights, void* d_out_proof_scalars, void* stream) try {
    if (!v || !d_out_interp || (n_commits && !d_out_commit_weights) ||
        (n_cells && (!commit_index || !coset_index || !d_evals || !d_weights || !d_out_proof_scalars)))
        return fail(ZKP_E_ARG, "null argument");
    ZCHK(cells_args(v, n_commits, n_cells, commit_index, coset_index));
    CTX_ENTER(v->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_cells_aggregate_locked(v, n_commits, n_cells, commit_index, coset_index, d_evals, d_weights, d_out_interp, d_out_commit_weights,
                                      d_out_proof_scalars, st);
} ZKP_CATCH_INT

int zkp_kzg_verify_cells_dev(const zkp_kzg_cell_verifier* v, const void* d_commits_xy, const uint8_t* d_commits_is_inf, size_t n_commits,
                             size_t n_cells, const uint32_t* commit_index, const uint32_t* coset_index, const void* d_evals,
                             const void* d_proofs_xy, const uint8_t* d_proofs_is_inf, const void* d_weights, void* stream, int* accepted) try {
    if (!v || !accepted || (n_cells && (!d_commits_xy || !commit_index || !coset_index || !d_evals || !d_proofs_xy || !d_weights)))
        return fail(ZKP_E_ARG, "null argument");
    ZCHK(cells_args(v, n_commits, n_cells, commit_index, coset_index));
    if (!n_cells) {
        *accepted = 1;
        return ZKP_OK;
    }
    CTX_ENTER(v->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_verify_cells_locked(v, d_commits_xy, d_commits_is_inf, n_commits, n_cells, commit_index, coset_index, d_evals, d_proofs_xy,
                                   d_proofs_is_inf, d_weights, st, accepted);
} ZKP_CATCH_INT

int zkp_kzg_verify_cells(const zkp_kzg_cell_verifier* v, const uint64_t* commits_xy, const uint8_t* commits_is_inf, size_t n_commits,
                         size_t n_cells, const uint32_t* commit_index, const uint32_t* coset_index, const uint64_t* evals,
                         const uint64_t* proofs_xy, const uint8_t* proofs_is_inf, const uint64_t* weights, int* accepted) try {
    if (!v || !accepted || (n_cells && (!commits_xy || !commit_index || !coset_index || !evals || !proofs_xy || !weights)))
        return fail(ZKP_E_ARG, "null argument");
    ZCHK(cells_args(v, n_commits, n_cells, commit_index, coset_index));
    if (!n_cells) {
        *accepted = 1;
        return ZKP_OK;
    }
    CTX_ENTER(v->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t M = n_commits, N = n_cells, l = (size_t)1 << v->log_l;
    void* ws = nullptr;  // evaluations | weights | commitments | proofs | the flags of both
    ZCHK(slot_workspace(32 * N * l + 32 * N + 96 * M + 96 * N + M + N, "zkp_kzg_verify_cells", &ws));
    char* d_evals = static_cast<char*>(ws);
    char* d_weights = d_evals + 32 * N * l;
    char* d_commits = d_weights + 32 * N;
    char* d_proofs = d_commits + 96 * M;
    uint8_t* d_cinf = reinterpret_cast<uint8_t*>(d_proofs + 96 * N);
    uint8_t* d_pinf = d_cinf + M;
    HIPCHK(hipMemcpyAsync(d_evals, evals, 32 * N * l, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_weights, weights, 32 * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_commits, commits_xy, 96 * M, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_proofs, proofs_xy, 96 * N, hipMemcpyHostToDevice, st));
    if (commits_is_inf) HIPCHK(hipMemcpyAsync(d_cinf, commits_is_inf, M, hipMemcpyHostToDevice, st));
    if (proofs_is_inf) HIPCHK(hipMemcpyAsync(d_pinf, proofs_is_inf, N, hipMemcpyHostToDevice, st));
    return kzg_verify_cells_locked(v, d_commits, commits_is_inf ? d_cinf : nullptr, M, N, commit_index, coset_index, d_evals, d_proofs,
                                   proofs_is_inf ? d_pinf : nullptr, d_weights, st, accepted);
} ZKP_CATCH_INT

}  // extern "C"
