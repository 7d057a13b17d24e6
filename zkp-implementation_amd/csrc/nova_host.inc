// nova_host.inc -- host driver of Nova folding (included at the end of api.hip, after plonk_host.inc whose device open it reuses).
//
// Mirrors nova/src/nifs (NIFS::{prover, prove, verify}), nova/src/r1cs (is_r1cs_satisfied) and nova/src/transcript.rs.  The R1CS
// matrices are uploaded once as CSR (zkp_nova_r1cs_create); the cross term, the relaxed-R1CS residual and the witness fold are the
// kernels of csrc/nova.hpp; commitments and openings are the resident MSM and the PLONK scan / evaluation kernels
// (open_eval_div_dev); the instance fold, the transcript and the verifier are host code.

struct zkp_nova_r1cs {
    const zkp_bases* srs = nullptr;
    int slot = 0;
    uint32_t rows = 0, nv = 0, nio = 0;
    DevBuf mem;           // one allocation: per matrix row_ptr | cols | vals, then the two row lists
    NovaCsr m[3];
    const uint32_t* short_rows = nullptr;
    const uint32_t* long_rows = nullptr;
    uint32_t n_short = 0, n_long = 0;
    Fr* d_x = nullptr;    // 2 x num_io (+ 1): x of the two z vectors of a launch
    Fr* d_t = nullptr;    // rows: T of the last prover call
    unsigned long long* d_count = nullptr;  // trimmed length / violated rows
    DevBuf stage;         // zkp_nova_nifs_prover / _prove: the host vectors
};

namespace {

int nova_check_csr(const zkp_csr* m, size_t rows, uint64_t ncols, const char* name) {
    if (!m || !m->row_ptr || (m->row_ptr[rows] && (!m->cols || !m->vals)))
        return fail(ZKP_E_ARG, std::string("null argument (matrix ") + name + ")");
    if (m->row_ptr[0] != 0) return fail(ZKP_E_ARG, std::string("matrix ") + name + ": row_ptr[0] must be 0");
    for (size_t i = 0; i < rows; i++)
        if (m->row_ptr[i + 1] < m->row_ptr[i])
            return fail(ZKP_E_ARG, std::string("matrix ") + name + ": row_ptr decreases at row " + std::to_string(i));
    const uint64_t nnz = m->row_ptr[rows];
    for (uint64_t e = 0; e < nnz; e++)
        if (m->cols[e] >= ncols)
            return fail(ZKP_E_ARG, std::string("matrix ") + name + ": column " + std::to_string(m->cols[e]) +
                                       " >= num_vars + num_io + 1");
    return ZKP_OK;
}

NovaRows nova_rows(const zkp_nova_r1cs* r, bool long_list) {
    NovaRows R;
    for (int k = 0; k < 3; k++) R.m[k] = r->m[k];
    R.nv = r->nv;
    R.nio = r->nio;
    R.list = long_list ? r->long_rows : r->short_rows;
    R.count = long_list ? r->n_long : r->n_short;
    return R;
}

// x (host, num_io Fr) of z vector k into the handle's device copy
int nova_put_x(zkp_nova_r1cs* r, int k, const uint64_t* x, hipStream_t st) {
    if (r->nio) HIPCHK(hipMemcpyAsync(r->d_x + (size_t)k * r->nio, x, 32 * (size_t)r->nio, hipMemcpyHostToDevice, st));
    return ZKP_OK;
}

NovaZ nova_zv(const zkp_nova_r1cs* r, int k, const void* d_w, const uint64_t u[4]) {
    NovaZ z;
    z.w = reinterpret_cast<const Fr*>(d_w);
    z.x = r->d_x + (size_t)k * r->nio;
    z.u = fr_dev(HFr::load(u));
    return z;
}

int nova_cross_locked(zkp_nova_r1cs* r, const void* d_w1, const uint64_t* x1, const uint64_t u1[4], const void* d_w2,
                      const uint64_t* x2, const uint64_t u2[4], Fr* d_t, hipStream_t st) {
    ZCHK(nova_put_x(r, 0, x1, st));
    ZCHK(nova_put_x(r, 1, x2, st));
    NovaZPair zp;
    zp.z[0] = nova_zv(r, 0, d_w1, u1);
    zp.z[1] = nova_zv(r, 1, d_w2, u2);
    if (r->n_short)
        hipLaunchKernelGGL(nova_cross_short_kernel, dim3((r->n_short + NOVA_THREADS - 1) / NOVA_THREADS), dim3(NOVA_THREADS), 0, st,
                           nova_rows(r, false), zp, d_t);
    if (r->n_long) hipLaunchKernelGGL(nova_cross_long_kernel, dim3(r->n_long), dim3(NOVA_WAVE), 0, st, nova_rows(r, true), zp, d_t);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

int nova_fold_locked(zkp_nova_r1cs* r, const HFr& rr, const void* e1, const void* w1, const void* e2, const void* w2, const void* t,
                     void* e_out, void* w_out, hipStream_t st) {
    const uint64_t n = std::max(r->rows, r->nv);
    hipLaunchKernelGGL(nova_fold_kernel, dim3((unsigned)((n + NOVA_THREADS - 1) / NOVA_THREADS)), dim3(NOVA_THREADS), 0, st,
                       reinterpret_cast<const Fr*>(e1), reinterpret_cast<const Fr*>(t), reinterpret_cast<const Fr*>(e2),
                       reinterpret_cast<Fr*>(e_out), (uint64_t)r->rows, reinterpret_cast<const Fr*>(w1), reinterpret_cast<const Fr*>(w2),
                       reinterpret_cast<Fr*>(w_out), (uint64_t)r->nv, fr_dev(rr), fr_dev(rr * rr));
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

// DensePolynomial::from_coefficients_vec's trimmed length of n device coefficients (synchronises st)
int nova_trim_len(zkp_nova_r1cs* r, const Fr* d, uint64_t n, hipStream_t st, uint64_t* len) {
    HIPCHK(hipMemsetAsync(r->d_count, 0, 8, st));
    hipLaunchKernelGGL(fr_trim_len_kernel, dim3((unsigned)((n + PK_THREADS - 1) / PK_THREADS)), dim3(PK_THREADS), 0, st, d, n, r->d_count);
    HIPCHK(hipGetLastError());
    unsigned long long h = 0;
    HIPCHK(hipMemcpyAsync(&h, r->d_count, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *len = h;
    return ZKP_OK;
}

// commit_vector (kzg/src/scheme.rs:63-67) of n device coefficients: the semantics of zkp_kzg_commit
int nova_commit_locked(zkp_nova_r1cs* r, const Fr* d, uint64_t n, hipStream_t st, HXyzz* out) {
    uint64_t len = 0;
    ZCHK(nova_trim_len(r, d, n, st, &len));
    const size_t have = r->srs->n;
    if (have == 0 || len > have) return fail(ZKP_E_SIZE, "SRS shorter than the polynomial (kzg/src/scheme.rs:86)");
    *out = HXyzz::infinity();
    if (!len) return ZKP_OK;
    return msm_partial(r->srs, d, (size_t)len, st, out);
}

// open_vector (kzg/src/scheme.rs:132-142) of n device coefficients at z, on the device: the values zkp_kzg_open returns
int nova_open_locked(zkp_nova_r1cs* r, const Fr* d, uint64_t n, const HFr& z, hipStream_t st, uint64_t out_xy[12], uint8_t* out_inf,
                     uint64_t out_eval[4]) {
    uint64_t len = 0;
    ZCHK(nova_trim_len(r, d, n, st, &len));
    HXyzz w = HXyzz::infinity();
    HFr y = HFr::zero();
    if (len) {  // a zero vector opens to y = 0 and the identity, as zkp_kzg_open opens it
        if (len - 1 > r->srs->n) return fail(ZKP_E_SIZE, "SRS shorter than the quotient polynomial (kzg/src/scheme.rs:86)");
        ZCHK(ctx().tmp.ensure(32 * open_scratch_elems(len) + 64));
        Fr* d_q = nullptr;
        ZCHK(open_eval_div_dev(reinterpret_cast<Fr*>(ctx().tmp.p), d, len, z, st, &y, &d_q));
        if (len > 1) ZCHK(msm_partial(r->srs, d_q, (size_t)(len - 1), st, &w));
    }
    w.to_affine(out_xy, out_inf);
    y.store(out_eval);
    return ZKP_OK;
}

}  // namespace

// ---- nova/src/transcript.rs -----------------------------------------------------------------------------------------------------
struct zkp_nova_transcript {
    PlonkChallengeGenerator gen;  // feed (transcript.rs:69-78) and generate_challenges (:95-114) are the PLONK generator's
};

extern "C" {

int zkp_nova_transcript_create(zkp_nova_transcript** out) try {
    if (!out) return fail(ZKP_E_ARG, "null argument");
    *out = new (std::nothrow) zkp_nova_transcript();
    return *out ? ZKP_OK : fail(ZKP_E_NOMEM, "out of host memory");
} ZKP_CATCH_INT
void zkp_nova_transcript_destroy(zkp_nova_transcript* t) { delete t; }

int zkp_nova_transcript_feed(zkp_nova_transcript* t, const uint64_t xy[12], uint8_t is_inf) try {
    if (!t || (!is_inf && !xy)) return fail(ZKP_E_ARG, "null argument");
    transcript_feed_g1(t->gen, xy, is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

// feed_scalar_num, transcript.rs:80-88: serialize_uncompressed(Fr) = the canonical integer, 32 little-endian bytes
int zkp_nova_transcript_feed_scalar(zkp_nova_transcript* t, const uint64_t s[4]) try {
    if (!t || !s) return fail(ZKP_E_ARG, "null argument");
    const HFr c = HFr::load(s).from_mont();
    uint8_t bytes[32];
    for (int i = 0; i < 32; i++) bytes[i] = static_cast<uint8_t>(c.l[i / 8] >> (8 * (i % 8)));
    t->gen.absorb(bytes, 32);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_nova_transcript_challenges(zkp_nova_transcript* t, size_t n, uint64_t* out) try {
    if (!t || (n && !out)) return fail(ZKP_E_ARG, "null argument");
    if (!t->gen.generate(n, out)) return fail(ZKP_E_ARG, "I'm hungry! Feed me something first");
    return ZKP_OK;
} ZKP_CATCH_INT

// ---- R1CS handle -----------------------------------------------------------------------------------------------------------------
void zkp_nova_r1cs_destroy(zkp_nova_r1cs* r) {
    if (!r) return;
    CtxScope s(r->slot);
    if (s.rc == ZKP_OK) (void)hipDeviceSynchronize();
    delete r;  // (also when the slot is gone: its buffers are released rather than leaked, hipFree finds their device itself)
}

int zkp_nova_r1cs_create(const zkp_bases* srs, size_t rows, size_t num_vars, size_t num_io, const zkp_csr* a, const zkp_csr* b,
                         const zkp_csr* c, zkp_nova_r1cs** out) try {
    if (!out) return fail(ZKP_E_ARG, "null argument");
    *out = nullptr;
    if (rows == 0 || num_vars == 0) return fail(ZKP_E_ARG, "an R1CS needs at least one row and one witness variable");
    const uint64_t ncols = (uint64_t)num_vars + num_io + 1;
    if (rows >= (1ull << 32) || ncols > (1ull << 32)) return fail(ZKP_E_ARG, "rows and columns must fit 32-bit indices");
    const zkp_csr* mats[3] = {a, b, c};
    static const char* const names[3] = {"A", "B", "C"};
    for (int k = 0; k < 3; k++) ZCHK(nova_check_csr(mats[k], rows, ncols, names[k]));  // (host only: checkable without a device)
    if (!srs) return fail(ZKP_E_ARG, "null argument (srs)");
    if (!srs->shards.empty()) return fail(ZKP_E_ARG, kShardedDev);
    // the row split (nova.hpp: NOVA_LONG_ROW); each list in row order, so that neighbouring lanes write neighbouring T entries
    std::vector<uint32_t> short_rows, long_rows;
    for (size_t i = 0; i < rows; i++) {
        uint64_t len = 0;
        for (int k = 0; k < 3; k++) len += mats[k]->row_ptr[i + 1] - mats[k]->row_ptr[i];
        (len > NOVA_LONG_ROW ? long_rows : short_rows).push_back((uint32_t)i);
    }
    auto align = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t off[3][3], total = 0;
    for (int k = 0; k < 3; k++) {
        const size_t nnz = mats[k]->row_ptr[rows];
        off[k][0] = total; total = align(total + 8 * (rows + 1));
        off[k][1] = total; total = align(total + 4 * nnz);
        off[k][2] = total; total = align(total + 32 * nnz);
    }
    const size_t off_short = total; total = align(total + 4 * short_rows.size());
    const size_t off_long = total; total = align(total + 4 * long_rows.size());
    const size_t off_x = total; total = align(total + 32 * (2 * num_io + 1));
    const size_t off_t = total; total = align(total + 32 * rows);
    const size_t off_cnt = total; total += 8;
    CTX_ENTER(srs->slot);
    WsOrder ord(nullptr);
    std::unique_ptr<zkp_nova_r1cs> r(new zkp_nova_r1cs());  // handed out only complete; freed on the slot's device otherwise
    r->srs = srs;
    r->slot = srs->slot;
    r->rows = (uint32_t)rows;
    r->nv = (uint32_t)num_vars;
    r->nio = (uint32_t)num_io;
    ZCHK(r->mem.ensure(total));
    char* base = static_cast<char*>(r->mem.p);
    for (int k = 0; k < 3; k++) {
        const size_t nnz = mats[k]->row_ptr[rows];
        HIPCHK(hipMemcpy(base + off[k][0], mats[k]->row_ptr, 8 * (rows + 1), hipMemcpyHostToDevice));
        if (nnz) {
            HIPCHK(hipMemcpy(base + off[k][1], mats[k]->cols, 4 * nnz, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(base + off[k][2], mats[k]->vals, 32 * nnz, hipMemcpyHostToDevice));
        }
        r->m[k] = NovaCsr{reinterpret_cast<const uint64_t*>(base + off[k][0]), reinterpret_cast<const uint32_t*>(base + off[k][1]),
                          reinterpret_cast<const Fr*>(base + off[k][2])};
    }
    if (!short_rows.empty()) HIPCHK(hipMemcpy(base + off_short, short_rows.data(), 4 * short_rows.size(), hipMemcpyHostToDevice));
    if (!long_rows.empty()) HIPCHK(hipMemcpy(base + off_long, long_rows.data(), 4 * long_rows.size(), hipMemcpyHostToDevice));
    r->short_rows = reinterpret_cast<const uint32_t*>(base + off_short);
    r->long_rows = reinterpret_cast<const uint32_t*>(base + off_long);
    r->n_short = (uint32_t)short_rows.size();
    r->n_long = (uint32_t)long_rows.size();
    r->d_x = reinterpret_cast<Fr*>(base + off_x);
    r->d_t = reinterpret_cast<Fr*>(base + off_t);
    r->d_count = reinterpret_cast<unsigned long long*>(base + off_cnt);
    *out = r.release();
    return ZKP_OK;
} ZKP_CATCH_INT

// ---- kernels one by one ----------------------------------------------------------------------------------------------------------
int zkp_nova_cross_term_dev(zkp_nova_r1cs* r, const void* d_w1, const uint64_t* x1, const uint64_t u1[4], const void* d_w2,
                            const uint64_t* x2, const uint64_t u2[4], void* d_t, void* stream) try {
    if (!r || !d_w1 || !d_w2 || !u1 || !u2 || !d_t || (r->nio && (!x1 || !x2))) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(r->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return nova_cross_locked(r, d_w1, x1, u1, d_w2, x2, u2, reinterpret_cast<Fr*>(d_t), st);
} ZKP_CATCH_INT

int zkp_nova_fold_witness_dev(zkp_nova_r1cs* r, const uint64_t rr[4], const void* d_e1, const void* d_w1, const void* d_e2,
                              const void* d_w2, const void* d_t, void* d_e_out, void* d_w_out, void* stream) try {
    if (!r || !rr || !d_e1 || !d_w1 || !d_e2 || !d_w2 || !d_t || !d_e_out || !d_w_out) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(r->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return nova_fold_locked(r, HFr::load(rr), d_e1, d_w1, d_e2, d_w2, d_t, d_e_out, d_w_out, st);
} ZKP_CATCH_INT

int zkp_nova_relaxed_residual_dev(zkp_nova_r1cs* r, const void* d_w, const uint64_t* x, const uint64_t u[4], const void* d_e,
                                  void* stream, uint64_t* bad_rows) try {
    if (!r || !d_w || !u || !d_e || !bad_rows || (r->nio && !x)) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(r->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    ZCHK(nova_put_x(r, 0, x, st));
    const NovaZ z = nova_zv(r, 0, d_w, u);
    const Fr* e = reinterpret_cast<const Fr*>(d_e);
    HIPCHK(hipMemsetAsync(r->d_count, 0, 8, st));
    if (r->n_short)
        hipLaunchKernelGGL(nova_residual_short_kernel, dim3((r->n_short + NOVA_THREADS - 1) / NOVA_THREADS), dim3(NOVA_THREADS), 0, st,
                           nova_rows(r, false), z, e, r->d_count);
    if (r->n_long)
        hipLaunchKernelGGL(nova_residual_long_kernel, dim3(r->n_long), dim3(NOVA_WAVE), 0, st, nova_rows(r, true), z, e, r->d_count);
    HIPCHK(hipGetLastError());
    unsigned long long h = 0;
    HIPCHK(hipMemcpyAsync(&h, r->d_count, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *bad_rows = h;
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"

// ---- NIFS::prover / prove --------------------------------------------------------------------------------------------------------
namespace {

HXyzz nova_pt(const uint64_t xy[12], uint8_t inf) { return HXyzz::from_affine(xy, inf != 0); }
HXyzz nova_mul(const HXyzz& p, const HFr& k) { return p.mul(k.from_mont().l); }

int nova_prover_locked(zkp_nova_r1cs* r, const void* e1, const void* w1, const void* e2, const void* w2, const zkp_nova_instance* fi1,
                       const zkp_nova_instance* fi2, zkp_nova_transcript* t, void* e_out, void* w_out, hipStream_t st,
                       zkp_nova_instance* out, uint64_t com_t_xy[12], uint8_t* com_t_inf, uint64_t r_out[4]) {
    // T and com_T (nifs_prover.rs:31-32)
    ZCHK(nova_cross_locked(r, w1, fi1->x, fi1->u, w2, fi2->x, fi2->u, r->d_t, st));
    HXyzz ct;
    ZCHK(nova_commit_locked(r, r->d_t, r->rows, st, &ct));
    uint64_t ct_xy[12];
    uint8_t ct_inf = 0;
    ct.to_affine(ct_xy, &ct_inf);
    // r = Transcript(u1, u2, com_T) (nifs_prover.rs:34-37)
    ZCHK(zkp_nova_transcript_feed_scalar(t, fi1->u));
    ZCHK(zkp_nova_transcript_feed_scalar(t, fi2->u));
    ZCHK(zkp_nova_transcript_feed(t, ct_xy, ct_inf));
    uint64_t rl[4];
    ZCHK(zkp_nova_transcript_challenges(t, 1, rl));
    const HFr rr = HFr::load(rl);
    // fold_witness on the device, fold_instance on the host (nifs_prover.rs:39-40; nifs/mod.rs:64-106)
    ZCHK(nova_fold_locked(r, rr, e1, w1, e2, w2, r->d_t, e_out, w_out, st));
    const HXyzz ce = nova_pt(fi1->com_e_xy, fi1->com_e_is_inf).add(nova_mul(ct, rr)).add(nova_mul(nova_pt(fi2->com_e_xy, fi2->com_e_is_inf), rr * rr));
    const HXyzz cw = nova_pt(fi1->com_w_xy, fi1->com_w_is_inf).add(nova_mul(nova_pt(fi2->com_w_xy, fi2->com_w_is_inf), rr));
    const HFr u = HFr::load(fi1->u) + HFr::load(fi2->u) * rr;
    for (uint32_t i = 0; i < r->nio; i++) (HFr::load(fi1->x + 4 * i) + HFr::load(fi2->x + 4 * i) * rr).store(out->x + 4 * i);
    ce.to_affine(out->com_e_xy, &out->com_e_is_inf);
    cw.to_affine(out->com_w_xy, &out->com_w_is_inf);
    u.store(out->u);
    std::memcpy(com_t_xy, ct_xy, 96);
    *com_t_inf = ct_inf;
    std::memcpy(r_out, rl, 32);
    return ZKP_OK;
}

int nova_prove_locked(zkp_nova_r1cs* r, const uint64_t rr[4], const void* d_e, const void* d_w, const zkp_nova_instance* fi,
                      zkp_nova_transcript* t, hipStream_t st, zkp_nova_proof* out) {
    // opening point = Transcript(com_E, com_W) (nifs_prover.rs:57-60)
    ZCHK(zkp_nova_transcript_feed(t, fi->com_e_xy, fi->com_e_is_inf));
    ZCHK(zkp_nova_transcript_feed(t, fi->com_w_xy, fi->com_w_is_inf));
    uint64_t z[4];
    ZCHK(zkp_nova_transcript_challenges(t, 1, z));
    const HFr zz = HFr::load(z);
    // open_vector(E), open_vector(W) (nifs_prover.rs:62-63)
    ZCHK(nova_open_locked(r, reinterpret_cast<const Fr*>(d_e), r->rows, zz, st, out->open_e_xy, &out->open_e_is_inf, out->eval_e));
    ZCHK(nova_open_locked(r, reinterpret_cast<const Fr*>(d_w), r->nv, zz, st, out->open_w_xy, &out->open_w_is_inf, out->eval_w));
    std::memcpy(out->r, rr, 32);
    std::memcpy(out->opening_point, z, 32);
    return ZKP_OK;
}

bool nova_instance_ok(const zkp_nova_r1cs* r, const zkp_nova_instance* fi) { return fi && (r->nio == 0 || fi->x); }

}  // namespace

extern "C" {

int zkp_nova_nifs_prover_dev(zkp_nova_r1cs* r, const void* d_e1, const void* d_w1, const void* d_e2, const void* d_w2,
                             const zkp_nova_instance* fi1, const zkp_nova_instance* fi2, zkp_nova_transcript* t, void* d_e_out,
                             void* d_w_out, void* stream, zkp_nova_instance* out, uint64_t com_t_xy[12], uint8_t* com_t_is_inf,
                             uint64_t r_out[4]) try {
    if (!r || !d_e1 || !d_w1 || !d_e2 || !d_w2 || !nova_instance_ok(r, fi1) || !nova_instance_ok(r, fi2) || !t || !d_e_out ||
        !d_w_out || !nova_instance_ok(r, out) || !com_t_xy || !com_t_is_inf || !r_out)
        return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(r->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return nova_prover_locked(r, d_e1, d_w1, d_e2, d_w2, fi1, fi2, t, d_e_out, d_w_out, st, out, com_t_xy, com_t_is_inf, r_out);
} ZKP_CATCH_INT

int zkp_nova_nifs_prover(zkp_nova_r1cs* r, const uint64_t* e1, const uint64_t* w1, const uint64_t* e2, const uint64_t* w2,
                         const zkp_nova_instance* fi1, const zkp_nova_instance* fi2, zkp_nova_transcript* t, uint64_t* e_out,
                         uint64_t* w_out, zkp_nova_instance* out, uint64_t com_t_xy[12], uint8_t* com_t_is_inf, uint64_t r_out[4]) try {
    if (!r || !e1 || !w1 || !e2 || !w2 || !nova_instance_ok(r, fi1) || !nova_instance_ok(r, fi2) || !t || !e_out || !w_out ||
        !nova_instance_ok(r, out) || !com_t_xy || !com_t_is_inf || !r_out)
        return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(r->slot);
    hipStream_t st = nullptr;
    WsOrder ord(st);
    const size_t eb = 32 * (size_t)r->rows, wb = 32 * (size_t)r->nv;
    ZCHK(r->stage.ensure(2 * (eb + wb)));
    char* d = static_cast<char*>(r->stage.p);
    char *de1 = d, *dw1 = d + eb, *de2 = dw1 + wb, *dw2 = de2 + eb;
    HIPCHK(hipMemcpyAsync(de1, e1, eb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dw1, w1, wb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(de2, e2, eb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(dw2, w2, wb, hipMemcpyHostToDevice, st));
    ZCHK(nova_prover_locked(r, de1, dw1, de2, dw2, fi1, fi2, t, de1, dw1, st, out, com_t_xy, com_t_is_inf, r_out));
    HIPCHK(hipMemcpyAsync(e_out, de1, eb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(w_out, dw1, wb, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_nova_nifs_prove_dev(zkp_nova_r1cs* r, const uint64_t rr[4], const void* d_e, const void* d_w, const zkp_nova_instance* fi,
                            zkp_nova_transcript* t, void* stream, zkp_nova_proof* out) try {
    if (!r || !rr || !d_e || !d_w || !fi || !t || !out) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(r->slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return nova_prove_locked(r, rr, d_e, d_w, fi, t, st, out);
} ZKP_CATCH_INT

int zkp_nova_nifs_prove(zkp_nova_r1cs* r, const uint64_t rr[4], const uint64_t* e, const uint64_t* w, const zkp_nova_instance* fi,
                        zkp_nova_transcript* t, zkp_nova_proof* out) try {
    if (!r || !rr || !e || !w || !fi || !t || !out) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(r->slot);
    hipStream_t st = nullptr;
    WsOrder ord(st);
    const size_t eb = 32 * (size_t)r->rows, wb = 32 * (size_t)r->nv;
    ZCHK(r->stage.ensure(eb + wb));
    char* d = static_cast<char*>(r->stage.p);
    HIPCHK(hipMemcpyAsync(d, e, eb, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d + eb, w, wb, hipMemcpyHostToDevice, st));
    return nova_prove_locked(r, rr, d, d + eb, fi, t, st, out);
} ZKP_CATCH_INT

// NIFS::verify, nifs_verifier.rs:22-91
int zkp_nova_nifs_verify(const uint64_t g2s_xy[24], const zkp_nova_proof* proof, const zkp_nova_instance* fi1,
                         const zkp_nova_instance* fi2, const zkp_nova_instance* fi3, const uint64_t com_t_xy[12], uint8_t com_t_is_inf,
                         zkp_nova_transcript* t, int* accepted) try {
    if (!g2s_xy || !proof || !fi1 || !fi2 || !fi3 || (!com_t_is_inf && !com_t_xy) || !t || !accepted)
        return fail(ZKP_E_ARG, "null argument");
    *accepted = 0;
    uint64_t ch[4];
    // verify_challenge, :44-66
    ZCHK(zkp_nova_transcript_feed_scalar(t, fi1->u));
    ZCHK(zkp_nova_transcript_feed_scalar(t, fi2->u));
    ZCHK(zkp_nova_transcript_feed(t, com_t_xy, com_t_is_inf));
    ZCHK(zkp_nova_transcript_challenges(t, 1, ch));
    if (std::memcmp(ch, proof->r, 32) != 0) {
        *accepted = -1;  // "Verify: Error in computing random r"
        return ZKP_OK;
    }
    // verify_opening, :69-91
    ZCHK(zkp_nova_transcript_feed(t, fi3->com_e_xy, fi3->com_e_is_inf));
    ZCHK(zkp_nova_transcript_feed(t, fi3->com_w_xy, fi3->com_w_is_inf));
    ZCHK(zkp_nova_transcript_challenges(t, 1, ch));
    if (std::memcmp(ch, proof->opening_point, 32) != 0) {
        *accepted = -2;  // "Verify: Error in computing random opening point"
        return ZKP_OK;
    }
    int ok = 0;
    ZCHK(zkp_kzg_verify(g2s_xy, fi3->com_w_xy, fi3->com_w_is_inf, proof->open_w_xy, proof->open_w_is_inf, proof->eval_w, ch, &ok));
    if (!ok) {
        *accepted = 0;  // "Verify: Folding wrong at W"
        return ZKP_OK;
    }
    ZCHK(zkp_kzg_verify(g2s_xy, fi3->com_e_xy, fi3->com_e_is_inf, proof->open_e_xy, proof->open_e_is_inf, proof->eval_e, ch, &ok));
    *accepted = ok ? 1 : -3;  // "Verify: Folding wrong at E"
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
