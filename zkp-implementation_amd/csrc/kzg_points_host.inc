// kzg_points_host.inc -- zkp_kzg_point_verifier_*, zkp_kzg_verify_points*, zkp_kzg_verify_points_find_bad*, zkp_kzg_points_aggregate_dev
// and zkp_kzg_verify_evals_batch_dev: any number of point openings of any number of commitments behind one pairing check (included at
// the end of api.hip, after kzg_evals_host.inc, whose field half gives the blob form its values).  The equation, the grouping tables,
// the launches and every size are in kzg_points_plan.hpp, the kernels in kzg_points.hpp; the points are validated with the kernels
// of g1_check.hpp and summed by the MSM driver; the two pairings are the host's (verify_host.inc).

struct zkp_kzg_point_verifier : KzgHandle {  // work: kzg_points_sizes
    unsigned chunk_log = 0;  // ZKP_KZG_CELLS_CHUNK_LOG as it was at creation
    uint64_t max_openings = 0, max_commits = 0;
    G2Aff g2s = G2Aff::infinity();  // [s]_2, validated at creation
    KzgPointsSizes sz;
    mutable HostStage stage;                // the table on its way to the device
    mutable std::vector<uint32_t> scratch;  // where the sort counts (host)
    // zkp_kzg_verify_points_each* (pairing_host.inc): the pairing checker over (G_2, [s]_2) and the workspace of the left points, both
    // made on first use, so that creating a verifier costs what it did
    mutable zkp_pairing_checker* each = nullptr;
    mutable DevBuf each_ws;
    ~zkp_kzg_point_verifier() { zkp_pairing_checker_destroy(each); }
};

namespace {

// Everything of a call that is checked before anything is launched
int points_args(const zkp_kzg_point_verifier* v, size_t n_commits, size_t n_openings, const uint32_t* commit_index) {
    if (n_openings > v->max_openings)
        return fail(ZKP_E_SIZE, std::to_string(n_openings) + " openings: the verifier was made for " + std::to_string(v->max_openings));
    if (n_commits > v->max_commits)
        return fail(ZKP_E_SIZE, std::to_string(n_commits) + " commitments: the verifier was made for " + std::to_string(v->max_commits));
    if (!commit_index) {
        if (n_commits != n_openings)
            return fail(ZKP_E_ARG, "no commit_index: opening i belongs to commitment i, so " + std::to_string(n_openings) + " openings need as many commitments, not " +
                                       std::to_string(n_commits));
        return ZKP_OK;
    }
    for (size_t i = 0; i < n_openings; i++)
        if (commit_index[i] >= n_commits)
            return fail(ZKP_E_ARG, "opening " + std::to_string(i) + ": commitment " + std::to_string(commit_index[i]) + " of " + std::to_string(n_commits));
    return ZKP_OK;
}

// The field half on `st` over n_openings openings (a whole batch, or a slice of one: every pointer is the slice's first element):
// the four outputs from resident points, values and weights.  The caller is inside the verifier's slot and has checked the
// arguments.  Walks kzg_points_step and launches nothing else.  Waits for nothing but the previous call's copy out of the staging
// buffer; allocates nothing.
int kzg_points_field_locked(const zkp_kzg_point_verifier* v, size_t n_commits, size_t n_openings, const uint32_t* commit_index, const void* d_z,
                            const void* d_y, const void* d_weights, void* d_out_commit_weights, void* d_out_rz, void* d_out_r, void* d_out_neg_sum,
                            hipStream_t st) {
    char* base = static_cast<char*>(v->work.p);
    KzgPointsTables t;
    if (commit_index) {
        ZCHK(v->stage.acquire());
        uint32_t* table = static_cast<uint32_t*>(v->stage.buf.p);
        t = kzg_points_tables(v->chunk_log, commit_index, n_openings, n_commits, v->scratch.data(), table);
        if (t.words > v->sz.table_words) return fail(ZKP_E_DEVICE, "internal error: the table of a call outgrew the verifier's");
        HIPCHK(hipMemcpyAsync(base + v->sz.table, table, 4 * t.words, hipMemcpyHostToDevice, st));
        ZCHK(v->stage.sent(st));
    } else {
        t = kzg_points_tables(v->chunk_log, nullptr, n_openings, n_commits, nullptr, nullptr);
    }
    const uint32_t* d_table = reinterpret_cast<const uint32_t*>(base + v->sz.table);
    Fr* cpartial = reinterpret_cast<Fr*>(base + v->sz.cpartial);
    Fr* ypartial = reinterpret_cast<Fr*>(base + v->sz.ypartial);
    const Fr* weights = static_cast<const Fr*>(d_weights);
    Fr* commit_weights = static_cast<Fr*>(d_out_commit_weights);
    const dim3 block(KZG_CELLS_THREADS);
    for (unsigned i = 0; i < KZG_POINTS_STEPS; i++) {
        const KzgPointsStep s = kzg_points_step(t, i);
        if (!s.blocks) continue;
        const dim3 grid((unsigned)s.blocks);
        switch (s.kind) {
        case KZG_POINTS_SCALARS:
            hipLaunchKernelGGL(points_scalars_kernel, grid, block, 0, st, weights, static_cast<const Fr*>(d_z), static_cast<const Fr*>(d_y), t.openings,
                               static_cast<Fr*>(d_out_rz), static_cast<Fr*>(d_out_r), t.identity ? commit_weights : nullptr, ypartial);
            break;
        case KZG_POINTS_FINISH:
            hipLaunchKernelGGL(points_finish_kernel, grid, block, 0, st, ypartial, kzg_points_blocks(t.openings), static_cast<Fr*>(d_out_neg_sum));
            break;
        case KZG_POINTS_CHUNKS:
            hipLaunchKernelGGL(points_chunks_kernel, grid, block, 0, st, weights, d_table + t.by_commit, d_table + t.cchunk_start, t.cchunks, cpartial);
            break;
        case KZG_POINTS_COMMITS:
            hipLaunchKernelGGL(cells_commits_kernel, grid, block, 0, st, cpartial, d_table + t.cseg_chunk, t.commits, commit_weights);
            break;
        }
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

// What a check reads: the whole batch, resident, and the handle over [C_0 .. C_(M-1), W_0 .. W_(N-1), G]
struct PointsBatch {
    size_t M, N;
    const uint32_t* commit_index;  // host, or null
    const Fr *z, *y, *weights;
    const zkp_bases* pts;
};

// One pairing check of the openings [lo, hi) of the batch, all M commitments behind them: the scalars of every other opening are
// zero, those of a commitment no opening of the slice names too.  Blocks.
int kzg_points_check(const zkp_kzg_point_verifier* v, const PointsBatch& b, size_t lo, size_t hi, hipStream_t st, int* ok) {
    const size_t M = b.M, N = b.N, all = M + N + 1;
    char* base = static_cast<char*>(v->work.p);
    Fr* sc_right = reinterpret_cast<Fr*>(base + v->sz.sc_right);
    Fr* sc_left = reinterpret_cast<Fr*>(base + v->sz.sc_left);
    {   // [sum r per commitment ..., r_i z_i ..., -sum r_i y_i] and [0 ..., r_i ..., 0]
        ProfScope phase("kzg_points_field", st);
        HIPCHK(hipMemsetAsync(sc_right, 0, 32 * all, st));
        HIPCHK(hipMemsetAsync(sc_left, 0, 32 * all, st));
        ZCHK(kzg_points_field_locked(v, b.commit_index ? M : hi - lo, hi - lo, b.commit_index ? b.commit_index + lo : nullptr, b.z + lo, b.y + lo,
                                     b.weights + lo, b.commit_index ? sc_right : sc_right + lo, sc_right + M + lo, sc_left + M + lo, sc_right + M + N, st));
    }
    HXyzz sums[2];
    {
        ProfScope phase("kzg_points_points", st);
        const Fr* vectors[2] = {sc_right, sc_left};
        ZCHK(msm_partial_batch(b.pts, vectors, 2, all, st, sums));
    }
    const auto t0 = std::chrono::steady_clock::now();
    *ok = pairings_equal(sums[1], v->g2s, sums[0], G2Aff::generator()) ? 1 : 0;
    prof_host("kzg_points_pairing", std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return ZKP_OK;
}

// The whole batch, and when it fails and the caller asked, the bisection: the lower half of the failing slice is always the one
// tested, so the index found is the lowest whose opening fails
int kzg_points_checks(const zkp_kzg_point_verifier* v, const PointsBatch& b, hipStream_t st, int* accepted, size_t* first_bad) {
    int ok = 0;
    ZCHK(kzg_points_check(v, b, 0, b.N, st, &ok));
    *accepted = ok;
    if (!first_bad) return ZKP_OK;
    *first_bad = SIZE_MAX;
    if (ok) return ZKP_OK;
    size_t lo = 0, hi = b.N;
    while (hi - lo > 1) {
        const size_t mid = (size_t)kzg_points_bisect_mid(lo, hi);
        ZCHK(kzg_points_check(v, b, lo, mid, st, &ok));
        if (ok) lo = mid;
        else hi = mid;
    }
    *first_bad = lo;
    return ZKP_OK;
}

// One verification with everything but the index array resident, on `st`; blocks (the pairings are the host's).  The caller is
// inside the verifier's slot and has checked the arguments; n_openings > 0.  first_bad: null, or where the lowest failing index goes.
int kzg_verify_points_locked(const zkp_kzg_point_verifier* v, const void* d_commits_xy, const uint8_t* d_commits_inf, size_t n_commits,
                             size_t n_openings, const uint32_t* commit_index, const void* d_z, const void* d_y, const void* d_proofs_xy,
                             const uint8_t* d_proofs_inf, const void* d_weights, hipStream_t st, int* accepted, size_t* first_bad) {
    const size_t M = n_commits, N = n_openings;
    char* base = static_cast<char*>(v->work.p);
    std::unique_ptr<zkp_bases, void (*)(zkp_bases*)> pts(nullptr, zkp_g1_bases_destroy);
    {
        ProfScope phase("kzg_points_points", st);
        // every point is checked before any is used, once for the whole batch: the batched equation says nothing about points outside G1
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
        // the transient handle over [C_0 .. C_(M-1), W_0 .. W_(N-1), G], unexpanded
        zkp_bases* raw = nullptr;
        ZCHK(bases_alloc(M + N + 1, true, &raw));
        pts.reset(raw);
        uint4* internal = static_cast<uint4*>(pts->d_xy.p);
        const struct { const void* src; size_t count, at; } parts[3] = {{d_commits_xy, M, 0}, {d_proofs_xy, N, M}, {base + v->sz.gen, 1, M + N}};
        for (const auto& p : parts) {
            hipLaunchKernelGGL(g1_to_internal_kernel, dim3((unsigned)((p.count + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS), 0, st,
                               static_cast<const uint4*>(p.src), (uint64_t)p.count, internal + 8 * p.at);
            if (hipGetLastError() != hipSuccess) {
                (void)hipStreamSynchronize(st);  // the handle goes before this entry returns: nothing may still read it
                return fail(ZKP_E_DEVICE, "g1_to_internal_kernel: the launch failed");
            }
        }
        int rc = hipMemsetAsync(pts->d_inf.p, 0, M + N + 1, st) == hipSuccess ? ZKP_OK : ZKP_E_DEVICE;
        if (rc == ZKP_OK && d_commits_inf && hipMemcpyAsync(pts->d_inf.get(), d_commits_inf, M, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = ZKP_E_DEVICE;
        if (rc == ZKP_OK && d_proofs_inf && hipMemcpyAsync(pts->d_inf.get() + M, d_proofs_inf, N, hipMemcpyDeviceToDevice, st) != hipSuccess) rc = ZKP_E_DEVICE;
        if (rc != ZKP_OK) {
            (void)hipStreamSynchronize(st);
            return fail(rc, "the flags of the call's points could not be copied");
        }
    }
    const PointsBatch b = {M, N, commit_index, static_cast<const Fr*>(d_z), static_cast<const Fr*>(d_y), static_cast<const Fr*>(d_weights), pts.get()};
    const int rc = kzg_points_checks(v, b, st, accepted, first_bad);
    if (rc != ZKP_OK) (void)hipStreamSynchronize(st);  // the handle goes before this entry returns: nothing may still read it
    return rc;
}

// The shared front of the four verifying entries: null arguments, the call's sizes and index, and the empty batch
int points_entry_args(const zkp_kzg_point_verifier* v, bool nulls, size_t n_commits, size_t n_openings, const uint32_t* commit_index, int* accepted,
                      size_t* first_bad, bool want_bad, bool* none) {
    if (!v || !accepted || (want_bad && !first_bad) || (n_openings && nulls)) return fail(ZKP_E_ARG, "null argument");
    ZCHK(points_args(v, n_commits, n_openings, commit_index));
    *none = n_openings == 0;
    if (*none) {
        *accepted = 1;
        if (want_bad) *first_bad = SIZE_MAX;
    }
    return ZKP_OK;
}

int verify_points_dev_entry(const zkp_kzg_point_verifier* v, const void* d_commits_xy, const uint8_t* d_commits_is_inf, size_t n_commits,
                            size_t n_openings, const uint32_t* commit_index, const void* d_z, const void* d_y, const void* d_proofs_xy,
                            const uint8_t* d_proofs_is_inf, const void* d_weights, void* stream, int* accepted, size_t* first_bad, bool want_bad) {
    bool none = false;
    ZCHK(points_entry_args(v, !d_commits_xy || !d_z || !d_y || !d_proofs_xy || !d_weights, n_commits, n_openings, commit_index, accepted, first_bad,
                           want_bad, &none));
    if (none) return ZKP_OK;
    CTX_ENTER(v->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_verify_points_locked(v, d_commits_xy, d_commits_is_inf, n_commits, n_openings, commit_index, d_z, d_y, d_proofs_xy, d_proofs_is_inf,
                                    d_weights, st, accepted, want_bad ? first_bad : nullptr);
}

int verify_points_host_entry(const zkp_kzg_point_verifier* v, const uint64_t* commits_xy, const uint8_t* commits_is_inf, size_t n_commits,
                             size_t n_openings, const uint32_t* commit_index, const uint64_t* z, const uint64_t* y, const uint64_t* proofs_xy,
                             const uint8_t* proofs_is_inf, const uint64_t* weights, int* accepted, size_t* first_bad, bool want_bad) {
    bool none = false;
    ZCHK(points_entry_args(v, !commits_xy || !z || !y || !proofs_xy || !weights, n_commits, n_openings, commit_index, accepted, first_bad, want_bad,
                           &none));
    if (none) return ZKP_OK;
    CTX_ENTER(v->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t M = n_commits, N = n_openings;
    void* ws = nullptr;  // points z | values y | weights | commitments | proofs | the flags of both
    ZCHK(slot_workspace(3 * 32 * N + 96 * M + 96 * N + M + N, "zkp_kzg_verify_points", &ws));
    char* d_z = static_cast<char*>(ws);
    char* d_y = d_z + 32 * N;
    char* d_weights = d_y + 32 * N;
    char* d_commits = d_weights + 32 * N;
    char* d_proofs = d_commits + 96 * M;
    uint8_t* d_cinf = reinterpret_cast<uint8_t*>(d_proofs + 96 * N);
    uint8_t* d_pinf = d_cinf + M;
    HIPCHK(hipMemcpyAsync(d_z, z, 32 * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_y, y, 32 * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_weights, weights, 32 * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_commits, commits_xy, 96 * M, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_proofs, proofs_xy, 96 * N, hipMemcpyHostToDevice, st));
    if (commits_is_inf) HIPCHK(hipMemcpyAsync(d_cinf, commits_is_inf, M, hipMemcpyHostToDevice, st));
    if (proofs_is_inf) HIPCHK(hipMemcpyAsync(d_pinf, proofs_is_inf, N, hipMemcpyHostToDevice, st));
    return kzg_verify_points_locked(v, d_commits, commits_is_inf ? d_cinf : nullptr, M, N, commit_index, d_z, d_y, d_proofs,
                                    proofs_is_inf ? d_pinf : nullptr, d_weights, st, accepted, want_bad ? first_bad : nullptr);
}

}  // namespace

extern "C" {

void zkp_kzg_point_verifier_destroy(zkp_kzg_point_verifier* v) { handle_destroy(v); }

int zkp_kzg_point_verifier_create(const uint64_t g2s_xy[24], size_t max_openings, size_t max_commits, zkp_kzg_point_verifier** out) try {
    if (!g2s_xy || !out) return fail(ZKP_E_ARG, "null argument");
    if (!max_openings || !max_commits || max_openings > KZG_CELLS_MAX_COUNT || max_commits > KZG_CELLS_MAX_COUNT)
        return fail(ZKP_E_ARG, "a point verifier is made for 1 .. 2^30 openings and as many commitments");
    G2Aff g2s = G2Aff::infinity();
    ZCHK(g2_validate(g2s_xy, "[s]_2", &g2s));
    CTX_ENTER(-1);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    auto v = handle_new<zkp_kzg_point_verifier>(0, 0);
    if (!v) return fail(ZKP_E_NOMEM, "host allocation failed");
    v->chunk_log = (unsigned)knob_int(KNOB_KZG_CELLS_CHUNK_LOG, KZG_CELLS_CHUNK_LOG);
    v->max_openings = max_openings;
    v->max_commits = max_commits;
    v->g2s = g2s;
    v->sz = kzg_points_sizes(v->chunk_log, max_openings, max_commits);
    const KzgPointsSizes& sz = v->sz;
    ZCHK(reserve_or_refuse(sz.total, KNOB_COUNT,
                           "zkp_kzg_point_verifier_create: the workspace of " + std::to_string(sz.total) + " bytes (and " +
                               std::to_string(sz.stage_total) + " pinned) does not fit",
                           [&] { return v->work.grow(sz.total) == hipSuccess && v->stage.make(sz.stage_total) == ZKP_OK; }));
    v->scratch.resize(sz.scratch_words);
    uint64_t gen[12];
    uint8_t gen_inf = 0;
    g1_generator_host().to_affine(gen, &gen_inf);
    HIPCHK(hipMemcpyAsync(static_cast<char*>(v->work.p) + sz.gen, gen, sizeof gen, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // (gen is this frame's)
    *out = v.release();
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_kzg_points_aggregate_dev(const zkp_kzg_point_verifier* v, size_t n_commits, size_t n_openings, const uint32_t* commit_index, const void* d_z,
                                 const void* d_y, const void* d_weights, void* d_out_commit_weights, void* d_out_rz, void* d_out_r,
                                 void* d_out_neg_sum, void* stream) try {
    if (!v || !d_out_neg_sum || (n_commits && !d_out_commit_weights) || (n_openings && (!d_z || !d_y || !d_weights || !d_out_rz || !d_out_r)))
        return fail(ZKP_E_ARG, "null argument");
    ZCHK(points_args(v, n_commits, n_openings, commit_index));
    CTX_ENTER(v->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_points_field_locked(v, n_commits, n_openings, commit_index, d_z, d_y, d_weights, d_out_commit_weights, d_out_rz, d_out_r, d_out_neg_sum,
                                   st);
} ZKP_CATCH_INT

int zkp_kzg_verify_points_dev(const zkp_kzg_point_verifier* v, const void* d_commits_xy, const uint8_t* d_commits_is_inf, size_t n_commits,
                              size_t n_openings, const uint32_t* commit_index, const void* d_z, const void* d_y, const void* d_proofs_xy,
                              const uint8_t* d_proofs_is_inf, const void* d_weights, void* stream, int* accepted) try {
    return verify_points_dev_entry(v, d_commits_xy, d_commits_is_inf, n_commits, n_openings, commit_index, d_z, d_y, d_proofs_xy, d_proofs_is_inf,
                                   d_weights, stream, accepted, nullptr, false);
} ZKP_CATCH_INT

int zkp_kzg_verify_points_find_bad_dev(const zkp_kzg_point_verifier* v, const void* d_commits_xy, const uint8_t* d_commits_is_inf, size_t n_commits,
                                       size_t n_openings, const uint32_t* commit_index, const void* d_z, const void* d_y, const void* d_proofs_xy,
                                       const uint8_t* d_proofs_is_inf, const void* d_weights, void* stream, int* accepted, size_t* first_bad) try {
    return verify_points_dev_entry(v, d_commits_xy, d_commits_is_inf, n_commits, n_openings, commit_index, d_z, d_y, d_proofs_xy, d_proofs_is_inf,
                                   d_weights, stream, accepted, first_bad, true);
} ZKP_CATCH_INT

int zkp_kzg_verify_points(const zkp_kzg_point_verifier* v, const uint64_t* commits_xy, const uint8_t* commits_is_inf, size_t n_commits,
                          size_t n_openings, const uint32_t* commit_index, const uint64_t* z, const uint64_t* y, const uint64_t* proofs_xy,
                          const uint8_t* proofs_is_inf, const uint64_t* weights, int* accepted) try {
    return verify_points_host_entry(v, commits_xy, commits_is_inf, n_commits, n_openings, commit_index, z, y, proofs_xy, proofs_is_inf, weights,
                                    accepted, nullptr, false);
} ZKP_CATCH_INT

int zkp_kzg_verify_points_find_bad(const zkp_kzg_point_verifier* v, const uint64_t* commits_xy, const uint8_t* commits_is_inf, size_t n_commits,
                                   size_t n_openings, const uint32_t* commit_index, const uint64_t* z, const uint64_t* y, const uint64_t* proofs_xy,
                                   const uint8_t* proofs_is_inf, const uint64_t* weights, int* accepted, size_t* first_bad) try {
    return verify_points_host_entry(v, commits_xy, commits_is_inf, n_commits, n_openings, commit_index, z, y, proofs_xy, proofs_is_inf, weights,
                                    accepted, first_bad, true);
} ZKP_CATCH_INT

int zkp_kzg_verify_evals_batch_dev(const zkp_kzg_point_verifier* v, const zkp_kzg_eval_opener* o, const void* d_evals, size_t n_polys, const void* d_z,
                                   const void* d_commits_xy, const uint8_t* d_commits_is_inf, const void* d_proofs_xy, const uint8_t* d_proofs_is_inf,
                                   const void* d_weights, void* stream, int* accepted) try {
    if (!v || !o || !accepted || (n_polys && (!d_evals || !d_z || !d_commits_xy || !d_proofs_xy || !d_weights))) return fail(ZKP_E_ARG, "null argument");
    if (o->slot != v->slot)
        return fail(ZKP_E_ARG, "the opener lives on slot " + std::to_string(o->slot) + ", the verifier on slot " + std::to_string(v->slot) +
                                   ": the values are formed where they are checked");
    bool none = false;
    ZCHK(evals_args(o, false, n_polys, &none));
    ZCHK(points_args(v, n_polys, n_polys, nullptr));
    if (none) {
        *accepted = 1;
        return ZKP_OK;
    }
    CTX_ENTER(v->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    // y_p = f_p(z_p) by the opener's field half (the quotients it also forms stay in the opener's workspace, unused)
    Fr* y = reinterpret_cast<Fr*>(static_cast<char*>(v->work.p) + v->sz.y);
    ZCHK(kzg_evals_field_locked(o, d_evals, n_polys, d_z, y, static_cast<char*>(o->work.p) + o->sz.rows, st));
    return kzg_verify_points_locked(v, d_commits_xy, d_commits_is_inf, n_polys, n_polys, nullptr, d_z, y, d_proofs_xy, d_proofs_is_inf, d_weights, st,
                                    accepted, nullptr);
} ZKP_CATCH_INT

}  // extern "C"
