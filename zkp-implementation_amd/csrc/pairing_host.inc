// pairing_host.inc -- zkp_pairing_checker_*, zkp_pairing_check_batch* and the self-test hooks zkp_selftest_fq12_dev /
// zkp_selftest_miller_dev: many pairing-product checks over k fixed G2 points per launch, a verdict byte per check (included at the
// end of api.hip, after kzg_points_host.inc).  The kernels are pairing.hip's (pairing.hpp has the design); the G2 walks are the
// host's affine code, done once at creation (pairing_host.hpp prepare_g2_lines); the points are validated with the kernels of
// g1_check.hpp.

struct zkp_pairing_checker : KzgHandle {  // work: the prepared lines | the Miller values of a call | the validation report
    int k = 0;
    uint32_t q_inf_mask = 0;  // bit j: Q_j is the identity
    uint64_t max_checks = 0, stride = 0;
    size_t off_f = 0, off_report = 0;
};

namespace {

int pairing_checker_args(const zkp_pairing_checker* c, size_t n_checks) {
    if (n_checks > c->max_checks)
        return fail(ZKP_E_SIZE, std::to_string(n_checks) + " checks: the checker was made for " + std::to_string(c->max_checks));
    return ZKP_OK;
}

// The k points of every check, validated as zkp_kzg_verify_points validates its points; blocks
int pairing_validate_locked(const zkp_pairing_checker* c, const void* d_p_xy, const uint8_t* d_p_is_inf, size_t n_checks, hipStream_t st) {
    G1CheckReport* d_rep = reinterpret_cast<G1CheckReport*>(static_cast<char*>(c->work.p) + c->off_report);
    G1CheckReport rep;
    HIPCHK(hipMemcpyAsync(d_rep, &kEmptyReport, sizeof kEmptyReport, hipMemcpyHostToDevice, st));
    ZCHK(g1_check_launch(g1_validate_raw_kernel, 96, d_p_xy, d_p_is_inf, n_checks * (size_t)c->k, 0, nullptr, d_rep, st));
    HIPCHK(hipMemcpyAsync(&rep, d_rep, sizeof rep, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (rep.first != ~0ull) {
        const uint64_t at = rep.first >> 2;
        return fail(ZKP_E_ARG, "p[" + std::to_string(at) + "] (check " + std::to_string(at / c->k) + ", pair " + std::to_string(at % c->k) +
                                   ") is not a point of G1 (" + kG1StatusWord[rep.first & 3] + ")");
    }
    return ZKP_OK;
}

// The two launches of a call.  The caller is inside the checker's slot and has checked the arguments; n_checks > 0.
int pairing_check_locked(const zkp_pairing_checker* c, const void* d_p_xy, const uint8_t* d_p_is_inf, size_t n_checks, int validate, uint8_t* d_ok,
                         void* d_out_fq12, hipStream_t st) {
    if (validate) ZCHK(pairing_validate_locked(c, d_p_xy, d_p_is_inf, n_checks, st));
    char* base = static_cast<char*>(c->work.p);
    {
        ProfScope phase("pairing_miller", st);
        pairing_miller_launch(st, base, c->q_inf_mask, c->k, d_p_xy, d_p_is_inf, (uint64_t)n_checks, base + c->off_f, c->stride, 1);
        HIPCHK(hipGetLastError());
    }
    {
        ProfScope phase("pairing_final_exp", st, true);
        pairing_final_exp_launch(st, base + c->off_f, c->stride, (uint64_t)n_checks, d_ok, d_out_fq12);
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

// A checker of the slot the caller has entered, over k prepared points (lines: k x PAIRING_LINE_WORDS; mask bit j: Q_j is the identity)
int pairing_checker_make_locked(const std::vector<uint64_t>& lines, int k, uint32_t mask, size_t max_checks, hipStream_t st, zkp_pairing_checker** out) {
    auto c = handle_new<zkp_pairing_checker>(0, 0);
    if (!c) return fail(ZKP_E_NOMEM, "host allocation failed");
    c->k = k;
    c->q_inf_mask = mask;
    c->max_checks = max_checks;
    c->stride = (max_checks + PAIRING_THREADS - 1) / PAIRING_THREADS * PAIRING_THREADS;
    c->off_f = k * PAIRING_LINE_BYTES;
    c->off_report = c->off_f + PAIRING_F12_BYTES * c->stride;
    const size_t total = c->off_report + sizeof(G1CheckReport);
    ZCHK(reserve_or_refuse(total, KNOB_COUNT,
                           "zkp_pairing_checker_create: the workspace of " + std::to_string(total) + " bytes (" + std::to_string(k * PAIRING_LINE_BYTES) +
                               " of prepared lines, " + std::to_string(PAIRING_F12_BYTES) + " per check) does not fit",
                           [&] { return c->work.grow(total) == hipSuccess; }));
    HIPCHK(hipMemcpyAsync(c->work.p, lines.data(), 8 * lines.size(), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));  // (lines is this frame's)
    *out = c.release();
    return ZKP_OK;
}

}  // namespace

extern "C" {

void zkp_pairing_checker_destroy(zkp_pairing_checker* c) { handle_destroy(c); }

int zkp_pairing_checker_create(const uint64_t* g2_xy, const uint8_t* g2_is_inf, size_t k, size_t max_checks, zkp_pairing_checker** out) try {
    if (!g2_xy || !out) return fail(ZKP_E_ARG, "null argument");
    if (k < 1 || k > (size_t)PAIRING_MAX_K) return fail(ZKP_E_ARG, "a pairing checker takes 1 .. 8 G2 points");
    if (!max_checks || max_checks > (size_t)1 << 24) return fail(ZKP_E_ARG, "a pairing checker is made for 1 .. 2^24 checks");
    std::vector<uint64_t> lines(k * PAIRING_LINE_WORDS, 0);
    uint32_t mask = 0;
    for (size_t j = 0; j < k; j++) {
        if (g2_is_inf && g2_is_inf[j]) {
            mask |= 1u << j;
            continue;
        }
        G2Aff q = G2Aff::infinity();
        ZCHK(g2_validate(g2_xy + 24 * j, ("g2[" + std::to_string(j) + "]").c_str(), &q));
        prepare_g2_lines(q, lines.data() + j * PAIRING_LINE_WORDS);
    }
    CTX_ENTER(-1);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    return pairing_checker_make_locked(lines, (int)k, mask, max_checks, st, out);
} ZKP_CATCH_INT

int zkp_pairing_check_batch_dev(const zkp_pairing_checker* c, const void* d_p_xy, const uint8_t* d_p_is_inf, size_t n_checks, int validate,
                                uint8_t* d_ok, void* d_out_fq12, void* stream) try {
    if (!c || (n_checks && (!d_p_xy || (!d_ok && !d_out_fq12)))) return fail(ZKP_E_ARG, "null argument");
    ZCHK(pairing_checker_args(c, n_checks));
    if (!n_checks) return ZKP_OK;
    CTX_ENTER(c->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return pairing_check_locked(c, d_p_xy, d_p_is_inf, n_checks, validate, d_ok, d_out_fq12, st);
} ZKP_CATCH_INT

int zkp_pairing_check_batch(const zkp_pairing_checker* c, const uint64_t* p_xy, const uint8_t* p_is_inf, size_t n_checks, int validate, uint8_t* ok,
                            uint64_t* out_fq12) try {
    if (!c || (n_checks && (!p_xy || (!ok && !out_fq12)))) return fail(ZKP_E_ARG, "null argument");
    ZCHK(pairing_checker_args(c, n_checks));
    if (!n_checks) return ZKP_OK;
    CTX_ENTER(c->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t pts = n_checks * (size_t)c->k;
    void* ws = nullptr;  // the values out | the points | their flags | the verdicts
    ZCHK(slot_workspace(PAIRING_F12_BYTES * n_checks + 96 * pts + pts + n_checks, "zkp_pairing_check_batch", &ws));
    char* d_out = static_cast<char*>(ws);
    char* d_p = d_out + PAIRING_F12_BYTES * n_checks;
    uint8_t* d_inf = reinterpret_cast<uint8_t*>(d_p + 96 * pts);
    uint8_t* d_ok = d_inf + pts;
    HIPCHK(hipMemcpyAsync(d_p, p_xy, 96 * pts, hipMemcpyHostToDevice, st));
    if (p_is_inf) HIPCHK(hipMemcpyAsync(d_inf, p_is_inf, pts, hipMemcpyHostToDevice, st));
    ZCHK(pairing_check_locked(c, d_p, p_is_inf ? d_inf : nullptr, n_checks, validate, ok ? d_ok : nullptr, out_fq12 ? d_out : nullptr, st));
    if (ok) HIPCHK(hipMemcpyAsync(ok, d_ok, n_checks, hipMemcpyDeviceToHost, st));
    if (out_fq12) HIPCHK(hipMemcpyAsync(out_fq12, d_out, PAIRING_F12_BYTES * n_checks, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_selftest_fq12_dev(int op, const void* d_a, const void* d_b, size_t n, void* d_out, void* stream) try {
    if (op < 0 || op >= ST_FQ12_OPS) return fail(ZKP_E_ARG, "unknown Fq12 self-test operation");
    const bool two = op == ST_FQ12_MUL || op == ST_FQ12_MUL_LINE;
    if (n && (!d_a || !d_out || (two && !d_b))) return fail(ZKP_E_ARG, "null argument");
    if (d_out && (d_out == d_a || d_out == d_b)) return fail(ZKP_E_ARG, "d_out must not be an operand");
    if (n > (size_t)1 << 24) return fail(ZKP_E_SIZE, "a self-test takes at most 2^24 cases");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    selftest_fq12_launch(op, reinterpret_cast<hipStream_t>(stream), d_a, d_b, d_out, (uint64_t)n);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_selftest_miller_dev(const zkp_pairing_checker* c, const void* d_p_xy, const uint8_t* d_p_is_inf, size_t n_checks, void* d_out_fq12,
                            void* stream) try {
    if (!c || (n_checks && (!d_p_xy || !d_out_fq12))) return fail(ZKP_E_ARG, "null argument");
    ZCHK(pairing_checker_args(c, n_checks));
    if (!n_checks) return ZKP_OK;
    CTX_ENTER(c->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    pairing_miller_launch(st, c->work.p, c->q_inf_mask, c->k, d_p_xy, d_p_is_inf, (uint64_t)n_checks, d_out_fq12, 1, PAIRING_F12_VEC);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"

// ---- zkp_kzg_verify_points_each*: a verdict per opening on the point verifier (kzg_points_host.inc).  One lane per opening forms
// (C_m(i) + [z_i]W_i - [y_i]G, -W_i) (kzg_points_each.hpp) and the verifier's own checker over (G_2, [s]_2), made on first use,
// judges every pair.

namespace {

constexpr size_t KZG_EACH_MAX = (size_t)1 << 24;  // what one pairing checker takes

// The workspace of a call over n openings: three planes of points, the pairs and their flags, the verdicts, the index
struct EachLayout {
    uint64_t cap;
    size_t ws_w, ws_g, ws_t, pairs, flags, ok, index, total;
    explicit EachLayout(size_t n) {
        cap = (n + G1_NTT_THREADS - 1) / G1_NTT_THREADS * G1_NTT_THREADS;
        ws_w = 0;
        ws_g = ws_w + 256 * cap;
        ws_t = ws_g + 256 * cap;
        pairs = ws_t + 256 * cap;
        flags = pairs + 192 * cap;
        ok = flags + 2 * cap;
        index = ok + cap;
        total = index + 4 * cap;
    }
};

// Everything resident but the index (host).  The caller is inside the verifier's slot and has checked the arguments; n_openings > 0.
// Blocks: the count comes back.
int kzg_verify_points_each_locked(const zkp_kzg_point_verifier* v, const void* d_commits_xy, const uint8_t* d_commits_inf, size_t n_commits,
                                  size_t n_openings, const uint32_t* commit_index, const void* d_z, const void* d_y, const void* d_proofs_xy,
                                  const uint8_t* d_proofs_inf, uint8_t* d_ok, uint8_t* ok_host, size_t* n_bad, hipStream_t st) {
    const size_t M = n_commits, N = n_openings;
    if (N > KZG_EACH_MAX) return fail(ZKP_E_SIZE, std::to_string(N) + " openings: a verdict per opening is given for at most 2^24 per call");
    char* vbase = static_cast<char*>(v->work.p);
    if (!v->each) {  // the first call pays for the two G2 walks and the checker's workspace
        std::vector<uint64_t> lines(2 * PAIRING_LINE_WORDS, 0);
        prepare_g2_lines(G2Aff::generator(), lines.data());
        prepare_g2_lines(v->g2s, lines.data() + PAIRING_LINE_WORDS);
        ZCHK(pairing_checker_make_locked(lines, 2, 0, (size_t)std::min<uint64_t>(v->max_openings, KZG_EACH_MAX), st, &v->each));
    }
    const EachLayout lay(N);
    if (lay.total > v->each_ws.cap)
        ZCHK(reserve_or_refuse(lay.total, KNOB_COUNT, "zkp_kzg_verify_points_each: the workspace of " + std::to_string(lay.total) + " bytes does not fit",
                               [&] { return v->each_ws.grow(lay.total) == hipSuccess; }, v->each_ws.cap));
    char* base = static_cast<char*>(v->each_ws.p);
    {   // every point is checked before any is used, as zkp_kzg_verify_points does
        ProfScope phase("kzg_each_points", st);
        G1CheckReport* d_rep = reinterpret_cast<G1CheckReport*>(vbase + v->sz.report);
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
        if (commit_index) HIPCHK(hipMemcpyAsync(base + lay.index, commit_index, 4 * N, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(points_each_kernel, dim3((unsigned)(lay.cap / G1_NTT_THREADS)), dim3(G1_NTT_THREADS), 0, st,
                           static_cast<const uint4*>(d_commits_xy), d_commits_inf, commit_index ? reinterpret_cast<const uint32_t*>(base + lay.index) : nullptr,
                           static_cast<const uint4*>(d_proofs_xy), d_proofs_inf, static_cast<const Fr*>(d_z), static_cast<const Fr*>(d_y),
                           reinterpret_cast<const uint4*>(vbase + v->sz.gen), (uint64_t)N, reinterpret_cast<uint4*>(base + lay.ws_w),
                           reinterpret_cast<uint4*>(base + lay.ws_g), reinterpret_cast<uint4*>(base + lay.ws_t), lay.cap,
                           reinterpret_cast<uint4*>(base + lay.pairs), reinterpret_cast<uint8_t*>(base + lay.flags));
        HIPCHK(hipGetLastError());
    }
    uint8_t* ok_dev = d_ok ? d_ok : reinterpret_cast<uint8_t*>(base + lay.ok);
    ZCHK(pairing_check_locked(v->each, base + lay.pairs, reinterpret_cast<const uint8_t*>(base + lay.flags), N, 0, ok_dev, nullptr, st));
    std::vector<uint8_t> tmp;
    if (!ok_host) {
        tmp.resize(N);
        ok_host = tmp.data();
    }
    HIPCHK(hipMemcpyAsync(ok_host, ok_dev, N, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (n_bad) {
        size_t bad = 0;
        for (size_t i = 0; i < N; i++) bad += ok_host[i] ? 0 : 1;
        *n_bad = bad;
    }
    return ZKP_OK;
}

int each_entry_args(const zkp_kzg_point_verifier* v, bool nulls, size_t n_commits, size_t n_openings, const uint32_t* commit_index, size_t* n_bad) {
    if (!v || (n_openings && nulls)) return fail(ZKP_E_ARG, "null argument");
    ZCHK(points_args(v, n_commits, n_openings, commit_index));
    if (!n_openings && n_bad) *n_bad = 0;
    return ZKP_OK;
}

}  // namespace

extern "C" {

int zkp_kzg_verify_points_each_dev(const zkp_kzg_point_verifier* v, const void* d_commits_xy, const uint8_t* d_commits_is_inf, size_t n_commits,
                                   size_t n_openings, const uint32_t* commit_index, const void* d_z, const void* d_y, const void* d_proofs_xy,
                                   const uint8_t* d_proofs_is_inf, uint8_t* d_ok, size_t* n_bad, void* stream) try {
    ZCHK(each_entry_args(v, !d_commits_xy || !d_z || !d_y || !d_proofs_xy || !d_ok, n_commits, n_openings, commit_index, n_bad));
    if (!n_openings) return ZKP_OK;
    CTX_ENTER(v->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return kzg_verify_points_each_locked(v, d_commits_xy, d_commits_is_inf, n_commits, n_openings, commit_index, d_z, d_y, d_proofs_xy, d_proofs_is_inf,
                                         d_ok, nullptr, n_bad, st);
} ZKP_CATCH_INT

int zkp_kzg_verify_points_each(const zkp_kzg_point_verifier* v, const uint64_t* commits_xy, const uint8_t* commits_is_inf, size_t n_commits,
                               size_t n_openings, const uint32_t* commit_index, const uint64_t* z, const uint64_t* y, const uint64_t* proofs_xy,
                               const uint8_t* proofs_is_inf, uint8_t* ok, size_t* n_bad) try {
    ZCHK(each_entry_args(v, !commits_xy || !z || !y || !proofs_xy || !ok, n_commits, n_openings, commit_index, n_bad));
    if (!n_openings) return ZKP_OK;
    CTX_ENTER(v->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t M = n_commits, N = n_openings;
    void* ws = nullptr;  // points z | values y | commitments | proofs | the flags of both
    ZCHK(slot_workspace(2 * 32 * N + 96 * M + 96 * N + M + N, "zkp_kzg_verify_points_each", &ws));
    char* d_z = static_cast<char*>(ws);
    char* d_y = d_z + 32 * N;
    char* d_commits = d_y + 32 * N;
    char* d_proofs = d_commits + 96 * M;
    uint8_t* d_cinf = reinterpret_cast<uint8_t*>(d_proofs + 96 * N);
    uint8_t* d_pinf = d_cinf + M;
    HIPCHK(hipMemcpyAsync(d_z, z, 32 * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_y, y, 32 * N, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_commits, commits_xy, 96 * M, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_proofs, proofs_xy, 96 * N, hipMemcpyHostToDevice, st));
    if (commits_is_inf) HIPCHK(hipMemcpyAsync(d_cinf, commits_is_inf, M, hipMemcpyHostToDevice, st));
    if (proofs_is_inf) HIPCHK(hipMemcpyAsync(d_pinf, proofs_is_inf, N, hipMemcpyHostToDevice, st));
    return kzg_verify_points_each_locked(v, d_commits, commits_is_inf ? d_cinf : nullptr, M, N, commit_index, d_z, d_y, d_proofs,
                                         proofs_is_inf ? d_pinf : nullptr, nullptr, ok, n_bad, st);
} ZKP_CATCH_INT

}  // extern "C"
