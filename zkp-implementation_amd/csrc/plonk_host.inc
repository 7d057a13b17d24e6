// plonk_host.inc -- host driver of the PLONK prover rounds (included at the end of api.hip).
//
// Mirrors plonk/src/prover.rs::generate_proof (61-293) round by round.  The reference draws the blinders from
// StdRng::from_entropy() and the challenges from its SHA-256 ChallengeGenerator; both stay on the caller's side of the
// boundary (they are inputs here), so a Rust shim keeps its transcript and calls one entry per round.
// Polynomials stay resident in HBM between rounds.

// The scratch the evaluation, division and scan helpers work in, by value: a prover's own buffers (zkp_plonk_prover::scratch(), made
// per call from the owners) or scratch borrowed by open_eval_div_dev
struct PlonkScratch {
    Fr* ev;                       // 2 len elements per division
    Fr* scan;
    uint64_t scan_cap;
    Fr* partial;
    unsigned partial_cap;
    uint64_t* h_pin;              // nullable (borrowed scratch): wait_stream then waits on the stream
    unsigned long long* poll_seq;
};

struct zkp_plonk_prover {
    const zkp_bases* srs = nullptr;
    unsigned log_n = 0, log_D = 0;
    uint64_t n = 0, D = 0, cap = 0;  // cap = n + 8 coefficients per working polynomial
    HFr k1, k2;
    // device polynomials (Fr coefficients)
    int device = 0;                // of the SRS's slot: where the resources below live
    TypedBuf<Fr> circ;    // 12 x n: q_m q_l q_r q_o q_c pi f_a f_b f_c s1 s2 s3
    TypedBuf<Fr> work;    // 8 x cap: ax bx cx z r wz wzw txc
    TypedBuf<Fr> t;       // D
    TypedBuf<Fr> ev;      // 15 x D
    // The 4n-coset evaluations of a(X), b(X), c(X), z(X) (slots 0..3 of the quotient's inputs) live in a buffer of their own and are
    // computed EARLY, on a second stream: those of a, b, c underneath round 1's commitments (they need no challenge), that of z
    // underneath round 2's -- a 2^16-term MSM is a chain of latencies that leaves most of the machine idle, so the transforms ride
    // along for free and round 3 starts at the quotient kernel (round 5: 0.1 ms per proof).  Every entry waits for the side stream's
    // work before it returns, so nothing of it outlives the call.
    TypedBuf<Fr> ev_w;    // 4 x D
    Stream side;
    Event ev_fork, ev_abc, ev_z;
    TypedBuf<Fr> scan;    // scan scratch (plonk.hpp, scan_scratch_elems)
    uint64_t scan_cap = 0;
    TypedBuf<Fr> partial;
    unsigned partial_cap = 0;
    TypedBuf<unsigned long long> d_len;
    TypedBuf<Fr> dom_evals;     // the 12 circuit polynomials evaluated on the domain (12 n, circuit order): circuit constants, computed by the first round 2
                                // (a prover made from gates starts with them: they are the columns its polynomials were interpolated from)
    uint64_t gates = 0;         // real gates of zkp_plonk_prover_create_from_gates; 0: made from coefficient vectors, no witness rebinding
    // "No remainder expected" (prover.rs:404,431,441), decided exactly on the domain instead of by long division:
    int gate_rows_bad = -1;     // rows of the witness that violate their gate equation (-1: not checked yet; a circuit constant)
    bool perm_closes = false;   // this proof's beta, gamma: prod_i num_i == prod_i den_i, i.e. the accumulator returns to 1 (:431)
    TypedBuf<uint64_t, PinnedBuf> h_pin;  // pinned host scratch (32 * partial_cap bytes) for the small read-backs: a D2H into pageable
                                          // memory costs ~20 us per call; one more line behind it holds the flag of wait_stream
    unsigned long long poll_seq = 0;
    uint64_t t_len = 0, chunk = 0, r_len = 0, wz_len = 0, wzw_len = 0;
    int stage = 0;
    HFr beta, gamma, alpha, zeta, bar[6], pi_e;
    // commit_para (kzg/src/scheme.rs:78-82): 4-bit window table of g1_points[0] (affine entries), built on first use by zkp_plonk_prove
    std::vector<HXyzz> para_table;
    // round 3: the coset evaluations of the 11 polynomials that do not depend on the proof (q_*, pi, s_sigma_*, L1, X) are
    // computed once per prover and stay in slots 4..14 of ev[] (rounds 2 and 5 only use the first three slots as scratch)
    bool fixed_evals_ready = false;
    // per-prover constants (host inversions are ~15 us each): 1 / Z_H on the D / n cosets of the quotient domain, 1 / n
    bool consts_ready = false;
    HFr zh_inv[8], n_inv;
    PlonkScratch scratch() { return {ev, scan, scan_cap, partial, partial_cap, h_pin, &poll_seq}; }
    Fr* poly(int i) const { return work + (uint64_t)i * cap; }
    Fr* circuit(int i) const { return circ + (uint64_t)i * n; }
};

namespace {

enum { P_AX = 0, P_BX, P_CX, P_Z, P_R, P_WZ, P_WZW, P_TXC };
enum { C_QM = 0, C_QL, C_QR, C_QO, C_QC, C_PI, C_FA, C_FB, C_FC, C_S1, C_S2, C_S3 };

Fr fr_dev(const HFr& x) { Fr r; std::memcpy(r.l, x.l, 32); return r; }

__global__ void fr_add_at_kernel(Fr* d, uint64_t idx, Fr v) { d[idx] = d[idx] + v; }

// d[idx] += v, enqueued on the stream (no host round trip)
int poke_add(Fr* d, uint64_t idx, const HFr& v, hipStream_t st) {
    hipLaunchKernelGGL(fr_add_at_kernel, dim3(1), dim3(1), 0, st, d, idx, fr_dev(v));
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

// dst_w = src_w (n coefficients, zero-padded to cap) + blind_w(X) * (X^n - 1) for up to three polynomials in one launch
// (mul_by_vanishing_poly, prover.rs:83-89,109); c[w][i] = coefficient i of blind_w
int blind_polys(zkp_plonk_prover* p, int count, Fr* const* dst, const Fr* const* src, const HFr (*c)[3], int len, hipStream_t st) {
    BlindParams bp;
    std::memset(&bp, 0, sizeof bp);
    for (int w = 0; w < count; w++) {
        bp.dst[w] = dst[w];
        bp.src[w] = src[w];
        for (int i = 0; i < len; i++) bp.c[w][i] = fr_dev(c[w][i]);
    }
    bp.len = (uint32_t)len;
    bp.n = p->n;
    bp.cap = p->cap;
    hipLaunchKernelGGL(plonk_blind_kernel, dim3((unsigned)((p->cap + PK_THREADS - 1) / PK_THREADS), (unsigned)count), dim3(PK_THREADS), 0, st, bp);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

int commit_dev(const zkp_plonk_prover* p, const Fr* coeffs, uint64_t len, hipStream_t st, uint64_t out_xy[12], uint8_t* out_inf) {
    if (len > p->srs->n) return fail(ZKP_E_SIZE, "SRS shorter than the polynomial (kzg/src/scheme.rs:86)");
    HXyzz r;
    ZCHK(msm_partial(p->srs, coeffs, (size_t)len, st, &r));
    r.to_affine(out_xy, out_inf);
    return ZKP_OK;
}

// `count` commitments of equal length in one pass through the MSM kernels
int commit_batch_dev(const zkp_plonk_prover* p, const Fr* const* coeffs, size_t count, uint64_t len, hipStream_t st,
                     uint64_t* out_xy, uint8_t* out_inf) {
    if (len > p->srs->n) return fail(ZKP_E_SIZE, "SRS shorter than the polynomial (kzg/src/scheme.rs:86)");
    HXyzz r[8];
    if (count > 8) return fail(ZKP_E_ARG, "internal: batch too large");
    ZCHK(msm_partial_batch(p->srs, coeffs, count, (size_t)len, st, r));
    batch_to_affine(r, count, out_xy, out_inf);  // one field inversion (a Fermat inverse is ~23 us of host time) for the batch
    return ZKP_OK;
}

// up to SCAN_MAX_BATCH independent scans with one operator in one set of three launches.  force_chunk: 0 = the elements per thread of
// scan_chunk_for (every caller but the self-test hooks at the end of this file), else that many (1..SCAN_MAX_CHUNK)
template <class Op>
int run_scan_batch(const PlonkScratch& s, const ScanJob* jobs, int count, hipStream_t st, uint32_t force_chunk = 0) {
    if (count < 1 || count > SCAN_MAX_BATCH) return fail(ZKP_E_ARG, "internal: scan batch");
    if (force_chunk > (uint32_t)SCAN_MAX_CHUNK) return fail(ZKP_E_ARG, "internal: scan chunk");
    ScanParams sp;
    std::memset(&sp, 0, sizeof sp);
    uint64_t nmax = 0;
    for (int j = 0; j < count; j++) {
        sp.job[j] = jobs[j];
        nmax = std::max<uint64_t>(nmax, jobs[j].n);
    }
    if (nmax == 0) return ZKP_OK;
    sp.chunk = force_chunk ? force_chunk : scan_chunk_for(nmax);
    const uint64_t blocks = scan_blocks_for(nmax, sp.chunk);
    if (blocks > (1u << 20) || SCAN_MAX_BATCH * blocks * 257 > s.scan_cap) return fail(ZKP_E_ARG, "internal: scan scratch too small");
    sp.blocks = (uint32_t)blocks;
    sp.tpre = s.scan;
    sp.btot = s.scan + SCAN_MAX_BATCH * blocks * 256;
    const dim3 grid((unsigned)blocks, (unsigned)count);
    hipLaunchKernelGGL((scan_block_kernel<Op>), grid, dim3(256), 0, st, sp);
    hipLaunchKernelGGL((scan_mid_kernel<Op>), dim3(1, (unsigned)count), dim3(256), 0, st, sp);
    hipLaunchKernelGGL((scan_apply_kernel<Op>), grid, dim3(256), 0, st, sp);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

// out[i] = c_i(z_i) for several (polynomial, point) pairs: all kernels are enqueued first, then ONE copy + sync
struct EvalReq { const Fr* c; uint64_t len; HFr z; HFr* out; };
// Wait for everything enqueued on `st`.  A proof has four small read-backs on its critical path (the accumulator's three totals, the
// quotient's length, two sets of evaluations) and the runtime's stream wait costs 30-60 us of wake-up latency each time: a one-thread
// kernel writes a sequence number into pinned memory behind the read-back and the host polls it (as the MSM does with its result
// flags: poll_or_sync, dev_res.hpp); without a pinned buffer (zkp_kzg_open's borrowed scratch), the stream wait.
int wait_stream(const PlonkScratch& s, hipStream_t st) {
    if (!s.h_pin || knob_flag(KNOB_PLONK_NO_POLL)) {
        HIPCHK(hipStreamSynchronize(st));
        return ZKP_OK;
    }
    unsigned long long* flag = reinterpret_cast<unsigned long long*>(s.h_pin + 4 * (size_t)s.partial_cap);
    const unsigned long long seq = ++*s.poll_seq;
    hipLaunchKernelGGL(stream_signal_kernel, dim3(1), dim3(1), 0, st, flag, seq);
    HIPCHK(hipGetLastError());
    return poll_or_sync(true, st, [=] { return __atomic_load_n(flag, __ATOMIC_ACQUIRE) == seq; });
}

int eval_many_dev(const PlonkScratch& s, const std::vector<EvalReq>& reqs, hipStream_t st) {
    if (reqs.size() > EVAL_MAX_REQ) return fail(ZKP_E_ARG, "internal: too many evaluation requests");
    EvalParams ep;
    std::memset(&ep, 0, sizeof ep);
    std::vector<unsigned> blocks(reqs.size());
    std::vector<HFr> zblock(reqs.size());
    unsigned total = 0, max_blocks = 0;
    for (size_t i = 0; i < reqs.size(); i++) {
        const uint64_t threads = (reqs[i].len + EVAL_CHUNK - 1) / EVAL_CHUNK;
        blocks[i] = (unsigned)((threads + PK_THREADS - 1) / PK_THREADS);
        ep.c[i] = reqs[i].c;
        ep.len[i] = reqs[i].len;
        ep.part_off[i] = total;
        ep.z[i] = fr_dev(reqs[i].z);
        HFr zk = reqs[i].z.pow_u64(EVAL_CHUNK);
        for (int k = 0; k < 8; k++) {
            ep.zp[i][k] = fr_dev(zk);
            zk = zk * zk;
        }
        zblock[i] = zk;  // z^(256 EVAL_CHUNK): one block further
        total += blocks[i];
        max_blocks = std::max(max_blocks, blocks[i]);
    }
    if (total > s.partial_cap) return fail(ZKP_E_ARG, "internal: evaluation scratch too small");
    if (max_blocks)
        hipLaunchKernelGGL(fr_poly_eval_kernel, dim3(max_blocks, (unsigned)reqs.size()), dim3(PK_THREADS), 0, st, ep, s.partial);
    HIPCHK(hipGetLastError());
    std::vector<uint64_t> pageable;
    uint64_t* h = s.h_pin;  // total <= partial_cap
    if (!h) {  // zkp_kzg_open's borrowed scratch has no pinned buffer
        pageable.resize(4 * (size_t)std::max(total, 1u));
        h = pageable.data();
    }
    if (total) HIPCHK(hipMemcpyAsync(h, s.partial, 32 * (size_t)total, hipMemcpyDeviceToHost, st));
    ZCHK(wait_stream(s, st));
    for (size_t i = 0; i < reqs.size(); i++) {
        HFr acc = HFr::zero();
        for (unsigned b = blocks[i]; b-- > 0;) acc = acc * zblock[i] + HFr::load(&h[4 * (size_t)(ep.part_off[i] + b)]);
        *reqs[i].out = acc;
    }
    return ZKP_OK;
}
int eval_dev(const PlonkScratch& s, const Fr* c, uint64_t len, const HFr& z, hipStream_t st, HFr* out) {
    return eval_many_dev(s, {EvalReq{c, len, z, out}}, st);
}

// *d_len = highest index of c[0..n) with a non-zero element, plus one (0: none); n >= 1.  Enqueued on `st`.
int trim_len_enqueue(const Fr* c, uint64_t n, unsigned long long* d_len, hipStream_t st) {
    HIPCHK(hipMemsetAsync(d_len, 0, 8, st));
    hipLaunchKernelGGL(fr_trim_len_kernel, dim3((unsigned)((n + PK_THREADS - 1) / PK_THREADS)), dim3(PK_THREADS), 0, st, c, n, d_len);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}
int trim_len_dev(zkp_plonk_prover* p, const Fr* c, uint64_t n, hipStream_t st, uint64_t* len) {
    ZCHK(trim_len_enqueue(c, n, p->d_len, st));
    HIPCHK(hipMemcpyAsync(p->h_pin, p->d_len, 8, hipMemcpyDeviceToHost, st));
    ZCHK(wait_stream(p->scratch(), st));
    *len = p->h_pin[0];
    return ZKP_OK;
}

ScalePowParams scale_pow_params(const HFr& base, uint64_t e0, uint32_t chunk) {
    ScalePowParams sp;
    sp.base = fr_dev(base);
    sp.c0 = fr_dev(base.pow_u64(e0));
    HFr b = base.pow_u64(chunk);
    for (int k = 0; k < 30; k++) {
        sp.bp[k] = fr_dev(b);
        b = b * b;
    }
    return sp;
}
// elements per thread of fr_scale_pow_kernel over at most n elements (about 2^16 threads) and the grid of `jobs` jobs
constexpr uint32_t SCALE_MAX_CHUNK = 8;
uint32_t scale_chunk_for(uint64_t n) { return (uint32_t)std::min<uint64_t>(SCALE_MAX_CHUNK, std::max<uint64_t>(1, n >> 16)); }
dim3 scale_pow_grid(uint64_t nmax, uint32_t chunk, int jobs) {
    return dim3((unsigned)(((nmax + chunk - 1) / chunk + PK_THREADS - 1) / PK_THREADS), (unsigned)jobs);
}

// q = (c(X) - c(z)) / (X - z): len - 1 coefficients into `out` (may not alias c), one or two divisions per set of launches (the two
// opening quotients of round 5 are independent); uses ev[] as scratch (2 len elements per division).  force_chunk: 0 = the elements
// per thread of scale_chunk_for and scan_chunk_for, else that many in both steps (1..SCALE_MAX_CHUNK; the self-test hooks only)
struct DivReq { const Fr* c; uint64_t len; HFr z; Fr* out; };
int div_linear_batch_dev(const PlonkScratch& s, const DivReq* reqs, int count, hipStream_t st, uint32_t force_chunk = 0) {
    if (force_chunk > SCALE_MAX_CHUNK) return fail(ZKP_E_ARG, "internal: scale chunk");
    DivReq rq[2];
    int m = 0;
    for (int i = 0; i < count; i++) {
        if (reqs[i].len <= 1) continue;
        if (reqs[i].z.is_zero()) {  // q_j = c_{j+1}
            HIPCHK(hipMemcpyAsync(reqs[i].out, reqs[i].c + 1, 32 * (reqs[i].len - 1), hipMemcpyDeviceToDevice, st));
            continue;
        }
        if (m == 2) return fail(ZKP_E_ARG, "internal: more than two divisions");
        rq[m++] = reqs[i];
    }
    if (!m) return ZKP_OK;
    uint64_t nmax = 0;
    for (int i = 0; i < m; i++) nmax = std::max(nmax, rq[i].len);
    const uint32_t chunk = force_chunk ? force_chunk : scale_chunk_for(nmax);
    HFr zinv[2];
    if (m == 2) {  // both inverses from one inversion
        const HFr pi = (rq[0].z * rq[1].z).inverse();
        zinv[0] = pi * rq[1].z;
        zinv[1] = pi * rq[0].z;
    } else {
        zinv[0] = rq[0].z.inverse();
    }
    ScalePowBatch fwd, back;
    std::memset(&fwd, 0, sizeof fwd);
    std::memset(&back, 0, sizeof back);
    ScanJob sj[2];
    Fr* scratch = s.ev;
    for (int i = 0; i < m; i++) {
        Fr* d = scratch;
        Fr* sfx = scratch + rq[i].len;
        scratch += 2 * rq[i].len;
        fwd.job[i] = ScalePowJob{rq[i].c, d, rq[i].len};
        fwd.sp[i] = scale_pow_params(rq[i].z, 0, chunk);
        sj[i] = ScanJob{d, sfx, rq[i].len, 1u, 1u};  // sfx[j] = sum_{i > j} d[i]
        back.job[i] = ScalePowJob{sfx, rq[i].out, rq[i].len - 1};
        back.sp[i] = scale_pow_params(zinv[i], 1, chunk);
    }
    fwd.chunk = back.chunk = chunk;
    const dim3 grid = scale_pow_grid(nmax, chunk, m);
    hipLaunchKernelGGL(fr_scale_pow_kernel, grid, dim3(PK_THREADS), 0, st, fwd);
    ZCHK(run_scan_batch<OpAdd>(s, sj, m, st, force_chunk));
    hipLaunchKernelGGL(fr_scale_pow_kernel, grid, dim3(PK_THREADS), 0, st, back);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}
int div_linear_dev(const PlonkScratch& s, const Fr* c, uint64_t len, const HFr& z, Fr* out, hipStream_t st) {
    const DivReq r{c, len, z, out};
    return div_linear_batch_dev(s, &r, 1, st);
}

struct LcTerm { const Fr* p; uint64_t len; HFr s; };
int lincomb_dev(const std::vector<LcTerm>& terms, Fr* out, uint64_t n_out, hipStream_t st) {
    LincombParams L;
    std::memset(&L, 0, sizeof L);
    if (terms.size() > LINCOMB_MAX) return fail(ZKP_E_ARG, "too many terms");
    L.terms = (int)terms.size();
    L.n_out = n_out;
    for (size_t k = 0; k < terms.size(); k++) {
        L.p[k] = terms[k].p;
        L.len[k] = terms[k].len;
        L.s[k] = fr_dev(terms[k].s);
    }
    hipLaunchKernelGGL(fr_lincomb_kernel, dim3((unsigned)((n_out + PK_THREADS - 1) / PK_THREADS)), dim3(PK_THREADS), 0, st, L, out);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

__global__ void fr_fill_kernel(Fr* p, uint64_t n, Fr v) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

const char* const kShardedSrsMsg = "SRS is sharded over several devices: a 2^16-gate proof does not shard (SURVEY 8e: replicas only) -- "
                                   "create the SRS on one slot (zkp_set_device) and run one prover per device";

// A prover of 2^log_n rows over `srs` with every buffer, stream and event it will need and zeroed polynomials; the caller is inside
// the SRS's slot (CTX_ENTER) and fills `circ`.  (Every HIP failure here reports the bare HIP error text.)
int prover_alloc(const zkp_bases* srs, unsigned log_n, const HFr& k1, const HFr& k2, std::unique_ptr<zkp_plonk_prover>& p) {
    const uint64_t n = 1ull << log_n;
    if (srs->n < n + 3) return fail(ZKP_E_SIZE, "SRS must hold circuit_size + 3 points (kzg/src/srs.rs:51)");
    p.reset(new (std::nothrow) zkp_plonk_prover());
    if (!p) return fail(ZKP_E_NOMEM, "host allocation failed");
    p->srs = srs;
    p->device = ctx().device;
    p->log_n = log_n;
    p->n = n;
    p->log_D = log_n + 2;
    while ((1ull << p->log_D) < 3 * n + 7) p->log_D++;  // t has 3n + 6 coefficients (prover.rs:149)
    p->D = 1ull << p->log_D;
    p->cap = n + 8;
    p->k1 = k1;
    p->k2 = k2;
    HIPCHK_BARE(p->circ.grow(32 * 12 * n));
    HIPCHK_BARE(p->work.grow(32 * 8 * p->cap));
    HIPCHK_BARE(p->t.grow(32 * std::max<uint64_t>(p->D, 2 * p->cap)));
    HIPCHK_BARE(p->ev.grow(32 * 15 * p->D));
    HIPCHK_BARE(p->ev_w.grow(32 * 4 * p->D));
    HIPCHK_BARE(p->side.make(hipStreamNonBlocking));
    for (Event* ev : {&p->ev_fork, &p->ev_abc, &p->ev_z}) HIPCHK_BARE(ev->make(hipEventDisableTiming));
    p->scan_cap = scan_scratch_elems(p->D);
    HIPCHK_BARE(p->scan.grow(32 * p->scan_cap));
    p->partial_cap = (unsigned)(8 * (p->D / (EVAL_CHUNK * PK_THREADS) + 2));
    HIPCHK_BARE(p->partial.grow(32 * (size_t)p->partial_cap));
    HIPCHK_BARE(p->d_len.grow(8));
    HIPCHK_BARE(p->h_pin.grow(32 * (size_t)p->partial_cap + 128, hipHostMallocPortable | hipHostMallocMapped));
    p->h_pin[4 * (size_t)p->partial_cap] = 0;
    HIPCHK_BARE(hipMemset(p->circ, 0, 32 * 12 * n));
    HIPCHK_BARE(hipMemset(p->work, 0, 32 * 8 * p->cap));
    return ZKP_OK;
}

}  // namespace

extern "C" {

int zkp_plonk_prover_create(const zkp_bases* srs, unsigned log_n, const uint64_t* const polys[12], const size_t lens[12],
                            const uint64_t k1[4], const uint64_t k2[4], zkp_plonk_prover** out) try {
    if (!srs || !polys || !lens || !k1 || !k2 || !out) return fail(ZKP_E_ARG, "null argument");
    if (log_n > 24) return fail(ZKP_E_ARG, "log_n > 24");
    if (!srs->shards.empty()) return fail(ZKP_E_ARG, kShardedSrsMsg);
    CTX_ENTER(srs->slot);
    WsOrder ord(nullptr);
    std::unique_ptr<zkp_plonk_prover> p;
    ZCHK(prover_alloc(srs, log_n, HFr::load(k1), HFr::load(k2), p));
    const uint64_t n = p->n;
    for (int i = 0; i < 12; i++) {
        if (lens[i] > n) return fail(ZKP_E_ARG, "circuit polynomial longer than n");
        if (lens[i]) HIPCHK_BARE(hipMemcpy(p->circuit(i), polys[i], 32 * lens[i], hipMemcpyHostToDevice));
    }
    *out = p.release();
    return ZKP_OK;
} ZKP_CATCH_INT

void zkp_plonk_prover_destroy(zkp_plonk_prover* p) {
    if (!p) return;
    if (p->side) (void)hipStreamSynchronize(p->side);
    DeviceRestore restore;
    (void)hipSetDevice(p->device);
    delete p;
}

// 1 / Z_H(g w_D^j) = 1 / (g^n w_{D/n}^j - 1), j < D / n (one shared inversion), and 1 / n: they depend on the sizes only
static void prover_constants(zkp_plonk_prover* p) {
    if (p->consts_ready) return;
    const HFr g = HFr::from_u64(7);
    const uint32_t shift = (uint32_t)(p->D / p->n);
    HFr gn = g.pow_u64(p->n), ws = fr_root_of_unity(p->log_D - p->log_n), cur = HFr::one();
    HFr zh[8], prefix[8], run = HFr::one();
    for (uint32_t j = 0; j < 8 && j < shift; j++) {
        zh[j] = gn * cur - HFr::one();
        prefix[j] = run;
        run = run * zh[j];
        cur = cur * ws;
    }
    HFr inv = run.inverse();
    for (uint32_t j = 8; j-- > 0;) {
        if (j >= shift) { p->zh_inv[j] = HFr::zero(); continue; }
        p->zh_inv[j] = inv * prefix[j];
        inv = inv * zh[j];
    }
    HFr ninv = HFr::one(), half = HFr::from_u64(2).inverse();
    for (unsigned i = 0; i < p->log_n; i++) ninv = ninv * half;
    p->n_inv = ninv;
    p->consts_ready = true;
}

// coset evaluations (4n or 8n domain, coset generator 7) of `count` witness polynomials into slots first .. first + count - 1 of ev_w,
// on the side stream, ordered after what `st` holds now; `done` is recorded behind them
int witness_coset_async(zkp_plonk_prover* p, int first, int count, const Fr* const* src, const uint64_t* lens, hipStream_t st, hipEvent_t done) {
    const HFr g = HFr::from_u64(7);
    const uint64_t D = p->D;
    HIPCHK(hipEventRecord(p->ev_fork, st));
    HIPCHK(hipStreamWaitEvent(p->side, p->ev_fork, 0));
    HIPCHK(hipMemsetAsync(p->ev_w + (uint64_t)first * D, 0, 32 * (uint64_t)count * D, p->side));
    for (int i = 0; i < count; i++)
        HIPCHK(hipMemcpyAsync(p->ev_w + (uint64_t)(first + i) * D, src[i], 32 * lens[i], hipMemcpyDeviceToDevice, p->side));
    ZCHK(run_ntt<Fr>(p->ev_w + (uint64_t)first * D, p->log_D, (size_t)count, 0, g.l, p->side));
    HIPCHK(hipEventRecord(done, p->side));
    return ZKP_OK;
}

// Round 1, prover.rs:68-92
int zkp_plonk_round1(zkp_plonk_prover* p, const uint64_t* blinders /* b1..b6, 6 x 4 limbs */, uint64_t* out_xy /* 3 x 12 */,
                     uint8_t* out_inf /* 3 */) try {
    if (!p || !blinders || !out_xy || !out_inf) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(p->srs->slot);
    hipStream_t st = nullptr;
    WsOrder ord(st);
    const uint64_t n = p->n;
    {   // pre_w = [b_{2w+2}, b_{2w+1}] (prover.rs:79-81): constant term b2, linear term b1
        Fr* dst[3] = {p->poly(P_AX), p->poly(P_BX), p->poly(P_CX)};
        const Fr* src[3] = {p->circuit(C_FA), p->circuit(C_FB), p->circuit(C_FC)};
        HFr pre[3][3];
        for (int w = 0; w < 3; w++) {
            pre[w][0] = HFr::load(blinders + 4 * (2 * w + 1));
            pre[w][1] = HFr::load(blinders + 4 * (2 * w));
        }
        ZCHK(blind_polys(p, 3, dst, src, pre, 2, st));
    }
    const Fr* polys3[3] = {p->poly(P_AX), p->poly(P_BX), p->poly(P_CX)};
    {   // round 3's transforms of a, b, c: under the commitments below
        const uint64_t lens[3] = {n + 2, n + 2, n + 2};
        ZCHK(witness_coset_async(p, 0, 3, polys3, lens, st, p->ev_abc));
    }
    const int rc = commit_batch_dev(p, polys3, 3, n + 2, st, out_xy, out_inf);  // commit_round1, prover.rs:571-581
    HIPCHK(hipEventSynchronize(p->ev_abc));  // (long done: the MSM synchronised the launch stream after ~1 ms)
    ZCHK(rc);
    p->stage = 1;
    return ZKP_OK;
} ZKP_CATCH_INT

// Round 2, prover.rs:98-123 (compute_acc 302-377)
int zkp_plonk_round2(zkp_plonk_prover* p, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t* blinders /* b7 b8 b9 */,
                     uint64_t out_xy[12], uint8_t* out_inf) try {
    if (!p || !beta || !gamma || !blinders || !out_xy || !out_inf) return fail(ZKP_E_ARG, "null argument");
    if (p->stage < 1) return fail(ZKP_E_ARG, "round 1 has not run");
    CTX_ENTER(p->srs->slot);
    hipStream_t st = nullptr;
    WsOrder ord(st);
    const uint64_t n = p->n;
    p->beta = HFr::load(beta);
    p->gamma = HFr::load(gamma);
    // evaluations of f_a f_b f_c s1 s2 s3 on the domain (the reference re-evaluates by Horner at every root).  They depend on
    // the circuit only, not on blinders or challenges: six transforms once per prover, not per proof
    if (!p->dom_evals) {  // published in the prover only once the transforms are enqueued: a failure on the way must not leave
        TypedBuf<Fr> de_new;   // a non-null, unfilled cache behind for the next proof
        ZCHK(de_new.ensure(32 * 12 * n));
        int rc = ZKP_OK;
        if (hipMemcpyAsync(de_new, p->circ, 32 * 12 * n, hipMemcpyDeviceToDevice, st) != hipSuccess)
            rc = fail(ZKP_E_DEVICE, "copy of the circuit polynomials failed");
        if (rc == ZKP_OK) rc = run_ntt<Fr>(de_new, p->log_n, 12, 0, nullptr, st);
        if (rc == ZKP_OK) {
            // the witness either satisfies its gates or it does not, whatever the blinders and challenges: checked once per prover
            // (the read-back rides on this round's existing synchronisation)
            if (hipMemsetAsync(p->d_len, 0, 8, st) != hipSuccess) rc = fail(ZKP_E_DEVICE, "memset failed");
            hipLaunchKernelGGL(plonk_gate_check_kernel, dim3((unsigned)((n + PK_THREADS - 1) / PK_THREADS)), dim3(PK_THREADS), 0, st,
                               de_new, n, p->d_len);
            if (rc == ZKP_OK && hipGetLastError() != hipSuccess) rc = fail(ZKP_E_DEVICE, "gate check launch failed");
            if (rc == ZKP_OK && hipMemcpyAsync(p->h_pin + 16, p->d_len, 8, hipMemcpyDeviceToHost, st) != hipSuccess)
                rc = fail(ZKP_E_DEVICE, "read-back failed");
        }
        // once per prover: resolved here, before anything else can fail or reuse the pinned word -- a state "read-back in flight"
        // that an early return further down left behind used to switch the gate check of round 3 off (ADVICE r4)
        if (rc == ZKP_OK && hipStreamSynchronize(st) != hipSuccess) rc = fail(ZKP_E_DEVICE, "gate check: synchronisation failed");
        if (rc != ZKP_OK) {
            (void)hipStreamSynchronize(st);  // before de_new is freed
            return rc;
        }
        p->gate_rows_bad = (int)std::min<uint64_t>(p->h_pin[16], 1u << 30);
        p->dom_evals = std::move(de_new);
    }
    const Fr* de = p->dom_evals + 6 * n;  // f_a f_b f_c s1 s2 s3
    AccParams ap;
    ap.a = de; ap.b = de + n; ap.c = de + 2 * n; ap.s1 = de + 3 * n; ap.s2 = de + 4 * n; ap.s3 = de + 5 * n;
    ap.beta = fr_dev(p->beta); ap.gamma = fr_dev(p->gamma); ap.k1 = fr_dev(p->k1); ap.k2 = fr_dev(p->k2);
    {
        HFr wk = fr_root_of_unity(p->log_n);
        for (int k = 0; k < 32; k++) {
            ap.wp[k] = fr_dev(wk);
            wk = wk.sqr();
        }
    }
    ap.n = n;
    Fr* num = p->ev + 6 * n;
    Fr* den = p->ev + 7 * n;
    Fr* nprefix = p->ev + 8 * n;
    Fr* dsuffix = p->ev + 9 * n;
    Fr* acc = p->ev + 10 * n;
    const unsigned nblocks = (unsigned)((n + PK_THREADS - 1) / PK_THREADS);
    hipLaunchKernelGGL(plonk_acc_numden_kernel, dim3(nblocks), dim3(PK_THREADS), 0, st, ap, num, den);
    HIPCHK(hipGetLastError());
    {   // prod_{j<i} num_j (acc_e[0] = 1) and prod_{j>=i} den_j in one set of launches
        const ScanJob sj[2] = {{num, nprefix, n, 0u, 1u}, {den, dsuffix, n, 1u, 0u}};
        ZCHK(run_scan_batch<OpMul>(p->scratch(), sj, 2, st));
    }
    uint64_t* total = p->h_pin;
    // three field elements go home in ONE launch that writes the pinned scratch directly (three device-to-host copies are three
    // blit launches of ~6 us each)
    hipLaunchKernelGGL(fr_gather3_kernel, dim3(1), dim3(64), 0, st, dsuffix, nprefix + (n - 1), num + (n - 1), total);
    HIPCHK(hipGetLastError());
    ZCHK(wait_stream(p->scratch(), st));
    // line2 - line3 of the quotient vanishes on the domain by construction of the accumulator everywhere but at the wrap-around
    // row, where it needs prod num_i == prod den_i (the copy constraints hold): the "No remainder" of prover.rs:431
    p->perm_closes = HFr::load(total + 4) * HFr::load(total + 8) == HFr::load(total);
    if (HFr::load(total) == HFr::zero())
        return fail(ZKP_E_ARG, "a permutation denominator is zero for these beta, gamma (rows 0 .. n-2: the reference divides by zero, "
                               "prover.rs:316,367; row n-1: the single-inversion accumulator of this prover cannot be formed)");
    const HFr inv_total = HFr::load(total).inverse();  // the one inversion of compute_acc (the reference divides n times)
    hipLaunchKernelGGL(plonk_acc_combine_kernel, dim3(nblocks), dim3(PK_THREADS), 0, st, nprefix, dsuffix, fr_dev(inv_total), n, acc);
    HIPCHK(hipGetLastError());
    ZCHK(run_ntt<Fr>(acc, p->log_n, 1, 1, nullptr, st));           // interpolate (prover.rs:374)
    Fr* z = p->poly(P_Z);
    {   // pre4 = [b9, b8, b7] (prover.rs:108)
        Fr* dst[1] = {z};
        const Fr* src[1] = {acc};
        const HFr pre[1][3] = {{HFr::load(blinders + 8), HFr::load(blinders + 4), HFr::load(blinders)}};
        ZCHK(blind_polys(p, 1, dst, src, pre, 3, st));
    }
    {   // round 3's transform of z: under the commitment below
        const Fr* zsrc[1] = {z};
        const uint64_t lens[1] = {n + 3};
        ZCHK(witness_coset_async(p, 3, 1, zsrc, lens, st, p->ev_z));
    }
    const int rc = commit_dev(p, z, n + 3, st, out_xy, out_inf);
    HIPCHK(hipEventSynchronize(p->ev_z));
    ZCHK(rc);
    p->stage = 2;
    return ZKP_OK;
} ZKP_CATCH_INT

// Round 3, prover.rs:136-150 (compute_quotient_polynomial 381-444, SlicePoly slice_polynomial.rs:22-53)
int zkp_plonk_round3(zkp_plonk_prover* p, const uint64_t alpha[4], uint64_t* out_xy /* 3 x 12 */, uint8_t* out_inf /* 3 */,
                     size_t* out_degree) try {
    if (!p || !alpha || !out_xy || !out_inf || !out_degree) return fail(ZKP_E_ARG, "null argument");
    if (p->stage < 2) return fail(ZKP_E_ARG, "round 2 has not run");
    CTX_ENTER(p->srs->slot);
    hipStream_t st = nullptr;
    WsOrder ord(st);
    const uint64_t n = p->n, D = p->D;
    p->alpha = HFr::load(alpha);
    const HFr g = HFr::from_u64(7);  // coset generator: the field's multiplicative generator (not in any 2-power subgroup)
    // slots 0..3 (a, b, c, z) were transformed into ev_w underneath the commitments of rounds 1 and 2 (witness_coset_async); the
    // eleven slots that depend on the circuit only are computed by the first proof of a prover and stay in ev[4..14]
    const int first_fixed = 4;
    if (!p->fixed_evals_ready) {
        HIPCHK(hipMemsetAsync(p->ev + (uint64_t)first_fixed * D, 0, 32 * (uint64_t)(15 - first_fixed) * D, st));
        const Fr* src[9] = {p->circuit(C_QM), p->circuit(C_QL), p->circuit(C_QR), p->circuit(C_QO), p->circuit(C_QC), p->circuit(C_PI),
                            p->circuit(C_S1), p->circuit(C_S2), p->circuit(C_S3)};
        for (int i = 0; i < 9; i++)
            HIPCHK(hipMemcpyAsync(p->ev + (uint64_t)(first_fixed + i) * D, src[i], 32 * n, hipMemcpyDeviceToDevice, st));
        // L1 = interpolate([1, 0, ..., 0]) has every coefficient equal to 1/n (l1_poly, prover.rs:459-464)
        prover_constants(p);
        const HFr ninv = p->n_inv;
        hipLaunchKernelGGL(fr_fill_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, p->ev + 13 * D, n, fr_dev(ninv));
        uint64_t one[4];
        HFr::one().store(one);
        HIPCHK(hipMemcpyAsync(p->ev + 14 * D + 1, one, 32, hipMemcpyHostToDevice, st));  // the polynomial X
        ZCHK(run_ntt<Fr>(p->ev + (uint64_t)first_fixed * D, p->log_D, (size_t)(15 - first_fixed), 0, g.l, st));
    }
    p->fixed_evals_ready = true;
    QuotParams qp;
    qp.ev = p->ev;
    qp.w = p->ev_w;
    qp.D = D;
    qp.shift = (uint32_t)(D / n);
    qp.beta = fr_dev(p->beta); qp.gamma = fr_dev(p->gamma); qp.alpha = fr_dev(p->alpha); qp.alpha2 = fr_dev(p->alpha.sqr());
    qp.k1 = fr_dev(p->k1); qp.k2 = fr_dev(p->k2);
    if (qp.shift > 8) return fail(ZKP_E_ARG, "unsupported domain ratio");
    prover_constants(p);
    for (uint32_t j = 0; j < 8; j++) qp.zh_inv[j] = fr_dev(p->zh_inv[j]);
    hipLaunchKernelGGL(plonk_quotient_kernel, dim3((unsigned)((D + PK_THREADS - 1) / PK_THREADS)), dim3(PK_THREADS), 0, st, qp, p->t);
    HIPCHK(hipGetLastError());
    ZCHK(run_ntt<Fr>(p->t, p->log_D, 1, 1, g.l, st));
    ZCHK(trim_len_dev(p, p->t, D, st, &p->t_len));
    // The reference divides the three numerator lines by Z_H and panics on a remainder.  Here the quotient comes from a coset
    // division, which "succeeds" whatever the numerator: a remainder rem(X) adds rem(X) / Z_H interpolated on the coset, a
    // polynomial in X^n times rem -- it only shows above 3n + 6 coefficients when deg rem >= 6 (a constant offset in q_c is
    // invisible).  So divisibility is decided where it is defined, on the domain: line 1 <=> every gate row holds
    // (plonk_gate_check_kernel, once per prover), lines 2-3 <=> the accumulator closes (round 2), line 4 <=> acc_0 = 1 (by
    // construction).  The length test stays as a guard for internal errors.
    if (p->gate_rows_bad < 0) return fail(ZKP_E_DEVICE, "the gate rows of the witness were never checked (round 2 did not complete)");
    if (p->gate_rows_bad > 0)
        return fail(ZKP_E_ARG, "No remainder expected: " + std::to_string(p->gate_rows_bad) +
                                   " gate row(s) of the witness do not satisfy q_m ab + q_l a + q_r b + q_o c + pi + q_c = 0 (prover.rs:404)");
    if (!p->perm_closes)
        return fail(ZKP_E_ARG, "No remainder expected: the copy constraints do not hold, the permutation accumulator does not return to 1 (prover.rs:431)");
    if (p->t_len > 3 * n + 6) return fail(ZKP_E_ARG, "No remainder expected: circuit not satisfied (prover.rs:404,431,441)");
    if (p->t_len == 0) return fail(ZKP_E_ARG, "zero quotient polynomial cannot be sliced (slice_polynomial.rs:30)");
    // SlicePoly::new: chunk = ceil(len / 3) consecutive coefficients per slice (slice_polynomial.rs:22-43)
    p->chunk = (p->t_len + 2) / 3;
    {   // the three slices are consecutive runs of `chunk` coefficients; beyond t_len the buffer holds exact zeros (the
        // transform size D exceeds 3n + 6), so all three commitments can use the same length
        const Fr* sl[3] = {p->t, p->t + p->chunk, p->t + 2 * p->chunk};
        if (3 * p->chunk > std::max<uint64_t>(p->D, 2 * p->cap)) return fail(ZKP_E_ARG, "internal: slice overruns the buffer");
        ZCHK(commit_batch_dev(p, sl, 3, p->chunk, st, out_xy, out_inf));
    }
    *out_degree = (size_t)(p->chunk - 1);
    p->stage = 3;
    return ZKP_OK;
} ZKP_CATCH_INT

// Round 4, prover.rs:156-178: bar_a bar_b bar_c bar_s_sigma_1 bar_s_sigma_2 bar_z_w
int zkp_plonk_round4(zkp_plonk_prover* p, const uint64_t zeta[4], uint64_t* out_bars /* 6 x 4 */) try {
    if (!p || !zeta || !out_bars) return fail(ZKP_E_ARG, "null argument");
    if (p->stage < 3) return fail(ZKP_E_ARG, "round 3 has not run");
    CTX_ENTER(p->srs->slot);
    hipStream_t st = nullptr;
    WsOrder ord(st);
    const uint64_t n = p->n;
    p->zeta = HFr::load(zeta);
    const HFr w = fr_root_of_unity(p->log_n);
    ZCHK(eval_many_dev(p->scratch(), {{p->poly(P_AX), n + 2, p->zeta, &p->bar[0]}, {p->poly(P_BX), n + 2, p->zeta, &p->bar[1]},
                           {p->poly(P_CX), n + 2, p->zeta, &p->bar[2]}, {p->circuit(C_S1), n, p->zeta, &p->bar[3]},
                           {p->circuit(C_S2), n, p->zeta, &p->bar[4]}, {p->poly(P_Z), n + 3, p->zeta * w, &p->bar[5]},
                           {p->circuit(C_PI), n, p->zeta, &p->pi_e}}, st));
    // tx_compact = sum_i zeta^((degree+1) i) slice_i (slice_polynomial.rs:56-70)
    std::vector<LcTerm> terms;
    HFr zc = p->zeta.pow_u64(p->chunk), cur = HFr::one();
    for (int i = 0; i < 3; i++) {
        const uint64_t off = (uint64_t)i * p->chunk;
        const uint64_t len = off < p->t_len ? std::min<uint64_t>(p->chunk, p->t_len - off) : 0;
        terms.push_back(LcTerm{p->t + off, len, cur});
        cur = cur * zc;
    }
    ZCHK(lincomb_dev(terms, p->poly(P_TXC), p->chunk, st));
    for (int i = 0; i < 6; i++) p->bar[i].store(out_bars + 4 * i);
    p->stage = 4;
    return ZKP_OK;
} ZKP_CATCH_INT

// Round 5, prover.rs:183-268 (compute_linearisation_polynomial 469-568)
int zkp_plonk_round5(zkp_plonk_prover* p, const uint64_t v_limbs[4], uint64_t* out_xy /* 2 x 12 */, uint8_t* out_inf /* 2 */) try {
    if (!p || !v_limbs || !out_xy || !out_inf) return fail(ZKP_E_ARG, "null argument");
    if (p->stage < 4) return fail(ZKP_E_ARG, "round 4 has not run");
    CTX_ENTER(p->srs->slot);
    hipStream_t st = nullptr;
    WsOrder ord(st);
    const uint64_t n = p->n;
    const HFr v = HFr::load(v_limbs);
    const HFr &beta = p->beta, &gamma = p->gamma, &alpha = p->alpha, &zeta = p->zeta;
    const HFr &ba = p->bar[0], &bb = p->bar[1], &bc = p->bar[2], &bs1 = p->bar[3], &bs2 = p->bar[4], &bzw = p->bar[5];
    const HFr w = fr_root_of_unity(p->log_n);
    // scalars of lines 2-5 (prover.rs:502-563)
    const HFr c2 = (ba + beta * zeta + gamma) * (bb + beta * p->k1 * zeta + gamma) * (bc + beta * p->k2 * zeta + gamma) * alpha;
    const HFr c3 = (ba + beta * bs1 + gamma) * (bb + beta * bs2 + gamma) * bzw * alpha;
    const HFr zn = zeta.pow_u64(n);
    const HFr zh = zn - HFr::one();                       // domain.evaluate_vanishing_polynomial(zeta)
    prover_constants(p);
    const HFr ninv = p->n_inv;
    HFr l1e;                                              // l1_poly(domain).evaluate(zeta) = (1/n) sum zeta^i
    if (zeta == HFr::one()) l1e = HFr::one();
    else l1e = ninv * zh * (zeta - HFr::one()).inverse();
    const HFr c4 = l1e * alpha.sqr();
    std::vector<LcTerm> terms = {
        {p->circuit(C_QM), n, ba * bb}, {p->circuit(C_QL), n, ba}, {p->circuit(C_QR), n, bb}, {p->circuit(C_QO), n, bc},
        {p->circuit(C_QC), n, HFr::one()}, {p->poly(P_Z), n + 3, c2 + c4}, {p->circuit(C_S3), n, (beta * c3).neg()},
        {p->poly(P_TXC), p->chunk, zh.neg()}};
    p->r_len = std::max<uint64_t>(n + 3, p->chunk);
    if (p->r_len > p->cap) return fail(ZKP_E_ARG, "internal: linearisation longer than the working capacity");
    Fr* r = p->poly(P_R);
    ZCHK(lincomb_dev(terms, r, p->r_len, st));
    // constant term: + pi_e (line1) - (bar_c + gamma) c3 (line3) - c4 (line4's "- 1")
    ZCHK(poke_add(r, 0, p->pi_e - (bc + gamma) * c3 - c4, st));
    HFr bar_r;
    ZCHK(eval_dev(p->scratch(), r, p->r_len, zeta, st, &bar_r));
    // w_ev_x (prover.rs:214-229)
    const HFr v2 = v * v, v3 = v2 * v, v4 = v3 * v, v5 = v4 * v;
    std::vector<LcTerm> wt = {{r, p->r_len, HFr::one()}, {p->poly(P_AX), n + 2, v}, {p->poly(P_BX), n + 2, v2},
                              {p->poly(P_CX), n + 2, v3}, {p->circuit(C_S1), n, v4}, {p->circuit(C_S2), n, v5}};
    Fr* num = p->t;  // t(X) itself is no longer needed after round 4's tx_compact; reuse as scratch
    ZCHK(lincomb_dev(wt, num, p->r_len, st));
    ZCHK(poke_add(num, 0, (bar_r + v * ba + v2 * bb + v3 * bc + v4 * bs1 + v5 * bs2).neg(), st));
    p->wz_len = p->r_len - 1;
    // w_ev_wx = (z - bar_z_w) / (X - zeta w) (prover.rs:247-265)
    Fr* num2 = p->t + p->cap;
    HIPCHK(hipMemcpyAsync(num2, p->poly(P_Z), 32 * (n + 3), hipMemcpyDeviceToDevice, st));
    ZCHK(poke_add(num2, 0, bzw.neg(), st));
    {
        const DivReq dv[2] = {{num, p->r_len, zeta, p->poly(P_WZ)}, {num2, n + 3, zeta * w, p->poly(P_WZW)}};
        ZCHK(div_linear_batch_dev(p->scratch(), dv, 2, st));
    }
    p->wzw_len = n + 2;
    if (p->wz_len == p->wzw_len) {
        const Fr* ws[2] = {p->poly(P_WZ), p->poly(P_WZW)};
        ZCHK(commit_batch_dev(p, ws, 2, p->wz_len, st, out_xy, out_inf));
    } else {
        ZCHK(commit_dev(p, p->poly(P_WZ), p->wz_len, st, out_xy, out_inf));
        ZCHK(commit_dev(p, p->poly(P_WZW), p->wzw_len, st, out_xy + 12, out_inf + 1));
    }
    p->stage = 5;
    return ZKP_OK;
} ZKP_CATCH_INT

// Copy one of the prover's polynomials to the host (parity tests): 0 ax 1 bx 2 cx 3 z 4 r 5 w_zeta 6 w_zeta_omega
// 7 tx_compact 8 t.  `out` receives min(cap_elems, length) coefficients; *len the untrimmed working length.
int zkp_plonk_get_poly(zkp_plonk_prover* p, int which, uint64_t* out, size_t cap_elems, size_t* len) try {
    if (!p || !len) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(p->srs->slot);
    WsOrder ord(nullptr);
    const Fr* src = nullptr;
    uint64_t l = 0;
    const uint64_t n = p->n;
    switch (which) {
        case 0: case 1: case 2: src = p->poly(which); l = n + 2; break;
        case 3: src = p->poly(P_Z); l = n + 3; break;
        case 4: src = p->poly(P_R); l = p->r_len; break;
        case 5: src = p->poly(P_WZ); l = p->wz_len; break;
        case 6: src = p->poly(P_WZW); l = p->wzw_len; break;
        case 7: src = p->poly(P_TXC); l = p->chunk; break;
        case 8: src = p->t; l = p->stage >= 5 ? 0 : p->t_len; break;
        default: return fail(ZKP_E_ARG, "unknown polynomial id");
    }
    *len = (size_t)l;
    const size_t m = std::min<size_t>(cap_elems, (size_t)l);
    if (m && out) HIPCHK(hipMemcpy(out, src, 32 * m, hipMemcpyDeviceToHost));
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"

// Elements of scratch open_eval_div_dev needs for `len` coefficients: q (len) | scale + scan scratch (2 len) | scan totals | evaluation
// partials
uint64_t open_scratch_elems(uint64_t len) {
    return 3 * len + scan_scratch_elems(len) + len / (EVAL_CHUNK * PK_THREADS) + 2;
}

// y = p(z) and q = (p - y) / (X - z) for `len` >= 1 coefficients resident at d_c: q (len - 1 coefficients) is left at the start of
// `scratch` (open_scratch_elems(len) elements that do not overlap d_c); *q_out points to it.  Enqueued on `st`; y is read back.
int open_eval_div_dev(Fr* scratch, const Fr* d_c, uint64_t len, const HFr& z, hipStream_t st, HFr* y, Fr** q_out) {
    const uint64_t n_tot = scan_scratch_elems(len);
    Fr* d_q = scratch;
    Fr* ev = d_q + len;
    const PlonkScratch w{ev, ev + 2 * len, n_tot, ev + 2 * len + n_tot, (unsigned)(len / (EVAL_CHUNK * PK_THREADS) + 2), nullptr, nullptr};
    ZCHK(eval_dev(w, d_c, len, z, st, y));
    if (len > 1) ZCHK(div_linear_dev(w, d_c, len, z, d_q, st));
    *q_out = d_q;
    return ZKP_OK;
}

// KzgScheme::open (kzg/src/scheme.rs:108-120) with the polynomial work on the device: y = p(z) by chunked Horner,
// q = (p - y) / (X - z) by weighted suffix sums, W = MSM(q).
int kzg_open_device(const zkp_bases* srs, const uint64_t* coeffs, size_t len, const uint64_t z_limbs[4], uint64_t out_xy[12],
                    uint8_t* out_is_inf, uint64_t out_eval[4]) {
    len = trimmed_len(coeffs, len);  // DensePolynomial trims trailing zeros (open_vector, scheme.rs:134)
    if (len == 0) {                  // zero polynomial: y = 0, zero quotient -> identity
        std::memset(out_eval, 0, 32);
        std::memset(out_xy, 0, 96);
        *out_is_inf = 1;
        return ZKP_OK;
    }
    if (len - 1 > srs->n) return fail(ZKP_E_SIZE, "SRS shorter than the quotient polynomial (kzg/src/scheme.rs:86)");
    // an SRS sharded over several devices: evaluation and division run on the first chunk's device, the quotient goes back to
    // the host and through the sharded MSM (every device uploads the coefficients of its own chunk)
    const bool sharded = !srs->shards.empty();
    std::vector<uint64_t> h_q;
    HXyzz r = HXyzz::infinity();
    {
        CTX_ENTER(sharded ? srs->shards[0]->slot : srs->slot);
        hipStream_t st = nullptr;
        WsOrder ord(st);
        // scratch carved from the staging buffer: coeffs | open_eval_div_dev's scratch
        ZCHK(ctx().tmp.ensure(32 * (len + open_scratch_elems(len)) + 64));
        Fr* d_c = reinterpret_cast<Fr*>(ctx().tmp.p);
        HIPCHK(hipMemcpyAsync(d_c, coeffs, 32 * len, hipMemcpyHostToDevice, st));
        HFr y;
        Fr* d_q = nullptr;
        ZCHK(open_eval_div_dev(d_c + len, d_c, len, HFr::load(z_limbs), st, &y, &d_q));
        y.store(out_eval);
        if (len > 1) {
            if (sharded) {
                h_q.resize(4 * (len - 1));
                HIPCHK(hipMemcpyAsync(h_q.data(), d_q, 32 * (len - 1), hipMemcpyDeviceToHost, st));
                HIPCHK(hipStreamSynchronize(st));
            } else {
                ZCHK(msm_partial(srs, d_q, len - 1, st, &r));
            }
        }
    }
    if (sharded && len > 1) ZCHK(msm_host_scalars_any(srs, h_q.data(), len - 1, &r));
    r.to_affine(out_xy, out_is_inf);
    return ZKP_OK;
}

// ---- generate_proof in one call (plonk/src/prover.rs:61-293) with the reference's own transcript ---------------
namespace {

// d * 16^w * G0 for w < 64, d in 1..15 (G0 = g1_points[0], read back from the resident bases)
int build_para_table(zkp_plonk_prover* p) {
    uint32_t raw[32];
    {
        CTX_ENTER(p->srs->slot);
        WsOrder ord(nullptr);
        if (!p->srs->n) return fail(ZKP_E_SIZE, "empty SRS (unwrap() at kzg/src/scheme.rs:79)");
        HIPCHK(hipMemcpy(raw, p->srs->d_xy.p, 128, hipMemcpyDeviceToHost));
    }
    HXyzz base{fq_from_limbs28(raw), fq_from_limbs28(raw + 16), HFq::one(), HFq::one()};
    p->para_table.resize(64 * 15);
    for (int w = 0; w < 64; w++) {
        HXyzz cur = base;
        for (int d = 0; d < 15; d++) {
            p->para_table[w * 15 + d] = cur;
            cur = cur.add(base);
        }
        for (int k = 0; k < 4; k++) base = base.dbl();
    }
    // normalise the table to affine (one inversion for all 960 entries) so that commit_para adds with the mixed formula; multiples
    // d * 16^w * G0 with 0 < d * 16^w < r are never the identity
    const size_t cnt = p->para_table.size();
    std::vector<uint64_t> xy(12 * cnt);
    std::vector<uint8_t> inf(cnt);
    batch_to_affine(p->para_table.data(), cnt, xy.data(), inf.data());
    for (size_t i = 0; i < cnt; i++) p->para_table[i] = HXyzz::from_affine(&xy[12 * i], false);
    return ZKP_OK;
}

HXyzz commit_para_xyzz(const zkp_plonk_prover* p, const HFr& para) {
    const HFr k = para.from_mont();
    HXyzz acc = HXyzz::infinity();
    for (int w = 0; w < 64; w++) {
        const unsigned d = (unsigned)(k.l[w >> 4] >> (4 * (w & 15))) & 15u;
        if (d) acc = acc.madd(p->para_table[w * 15 + d - 1].x, p->para_table[w * 15 + d - 1].y);
    }
    return acc;
}

void commit_para(const zkp_plonk_prover* p, const HFr& para, uint64_t out_xy[12], uint8_t* out_inf) {
    commit_para_xyzz(p, para).to_affine(out_xy, out_inf);
}

}  // namespace

extern "C" int zkp_plonk_prove(zkp_plonk_prover* p, const uint64_t* blinders /* b1..b9, 9 x 4 limbs */, zkp_plonk_proof* out) try {
    if (!p || !blinders || !out) return fail(ZKP_E_ARG, "null argument");
    if (p->srs->d_inf.p) return fail(ZKP_E_ARG, "SRS with infinity points");
    if (p->para_table.empty()) ZCHK(build_para_table(p));
    std::memset(out, 0, sizeof *out);
    PlonkChallengeGenerator ch;
    auto feed = [&](int i) {
        uint64_t x[6] = {0}, y[6] = {0};
        if (!out->commit_is_inf[i]) {
            const HFq cx = HFq::load(out->commit_xy[i]).from_mont(), cy = HFq::load(out->commit_xy[i] + 6).from_mont();
            std::memcpy(x, cx.l, 48);
            std::memcpy(y, cy.l, 48);
        }
        ch.feed(x, y, out->commit_is_inf[i] != 0);
    };
    uint64_t c2[8], c1[4];
    // round 1 (prover.rs:68-92), round 2 (94-123)
    ZCHK(zkp_plonk_round1(p, blinders, out->commit_xy[0], out->commit_is_inf));
    feed(0); feed(1); feed(2);
    ch.generate(2, c2);  // beta, gamma
    ZCHK(zkp_plonk_round2(p, c2, c2 + 4, blinders + 24, out->commit_xy[3], out->commit_is_inf + 3));
    // round 3 (133-150)
    feed(3);
    ch.generate(1, c1);  // alpha
    size_t degree = 0;
    ZCHK(zkp_plonk_round3(p, c1, out->commit_xy[4], out->commit_is_inf + 4, &degree));
    out->degree = degree;
    // round 4 (155-178)
    feed(4); feed(5); feed(6);
    ch.generate(1, c1);  // evaluation challenge
    ZCHK(zkp_plonk_round4(p, c1, out->bars[0]));
    // round 5 (183-268): the six evaluations enter the transcript as commit_para(bar) = bar * g1_points[0]
    HXyzz para[6];
    uint64_t para_xy[6 * 12];
    uint8_t para_inf[6];
    {  // six independent fixed-base multiplications of ~25 us: spread over the resident host workers
        const std::function<void(size_t)> job = [&](size_t i) { para[i] = commit_para_xyzz(p, HFr::load(out->bars[i])); };
        host_pool().run(job, 6);
    }
    batch_to_affine(para, 6, para_xy, para_inf);
    for (int i = 0; i < 6; i++) {
        const uint64_t* xy = para_xy + 12 * i;
        const uint8_t inf = para_inf[i];
        uint64_t x[6] = {0}, y[6] = {0};
        if (!inf) {
            const HFq cx = HFq::load(xy).from_mont(), cy = HFq::load(xy + 6).from_mont();
            std::memcpy(x, cx.l, 48);
            std::memcpy(y, cy.l, 48);
        }
        ch.feed(x, y, inf != 0);
    }
    ch.generate(1, c1);  // v
    ZCHK(zkp_plonk_round5(p, c1, out->commit_xy[7], out->commit_is_inf + 7));
    feed(7); feed(8);
    ch.generate(1, out->u);
    return ZKP_OK;
} ZKP_CATCH_INT

// ---- self-test hooks of the polynomial helpers above (include/zkp_hip.h: zkp_selftest_poly_*_dev) ---------------
// Host code only: every hook checks its arguments, carves the helper's scratch from the slot's staging buffer (as kzg_open_device does)
// and calls the helper the prover calls, which launches the kernels the prover launches.  tests/test_gpu_poly_primitives.py.
namespace {

constexpr uint64_t POLY_SELFTEST_MAX = 1ull << 22;  // elements per vector: the scratch of two scans at one element per thread stays near 0.5 GB

// [a, a + na) and [b, b + nb) (32-byte elements) share a byte; the same start is accepted where `same_ok` (a kernel that reads
// element i and writes element i in one thread works in place)
bool fr_ranges_clash(const void* a, uint64_t na, const void* b, uint64_t nb, bool same_ok) {
    if (!na || !nb || !a || !b) return false;
    if (a == b) return !same_ok;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + 32 * nb && b0 < a0 + 32 * na;
}
int poly_selftest_scratch(uint64_t elems, Fr** out) {
    ZCHK(ctx().tmp.ensure(32 * elems + 64));
    *out = reinterpret_cast<Fr*>(ctx().tmp.p);
    return ZKP_OK;
}

}  // namespace

extern "C" {

int zkp_selftest_poly_scan_dev(int op, size_t count, const void* const* d_in, void* const* d_out, const size_t* n, const unsigned* flags,
                               unsigned chunk, void* stream) try {
    if (!d_in || !d_out || !n || !flags) return fail(ZKP_E_ARG, "null argument");
    if (op != 0 && op != 1) return fail(ZKP_E_ARG, "op must be 0 (add) or 1 (mul)");
    if (count < 1 || count > (size_t)SCAN_MAX_BATCH) return fail(ZKP_E_ARG, "a scan launch takes one or two jobs");
    if (chunk > (unsigned)SCAN_MAX_CHUNK) return fail(ZKP_E_ARG, "chunk must be 0 (the production rule) or 1..16 elements per thread");
    ScanJob jobs[SCAN_MAX_BATCH];
    uint64_t nmax = 0;
    for (size_t j = 0; j < count; j++) {
        if (n[j] && (!d_in[j] || !d_out[j])) return fail(ZKP_E_ARG, "null argument");
        if (flags[j] > 3) return fail(ZKP_E_ARG, "flags: bit 0 = suffix scan, bit 1 = exclusive");
        if (n[j] > POLY_SELFTEST_MAX) return fail(ZKP_E_SIZE, "a polynomial self-test takes at most 2^22 elements per vector");
        jobs[j] = ScanJob{reinterpret_cast<const Fr*>(d_in[j]), reinterpret_cast<Fr*>(d_out[j]), n[j], flags[j] & 1u, (flags[j] >> 1) & 1u};
        nmax = std::max<uint64_t>(nmax, n[j]);
    }
    for (size_t j = 0; j < count; j++)
        for (size_t k = 0; k < count; k++)
            if (fr_ranges_clash(d_out[j], n[j], d_in[k], n[k], j == k) || (k != j && fr_ranges_clash(d_out[j], n[j], d_out[k], n[k], false)))
                return fail(ZKP_E_ARG, "a scan's output overlaps another vector of the launch (in place is d_out == d_in of the same job)");
    CTX_ENTER(-1);
    if (!nmax) return ZKP_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    // the rule's own bound where the rule picks the chunk, what the forced chunk needs otherwise
    const uint64_t cap = chunk ? SCAN_MAX_BATCH * scan_blocks_for(nmax, chunk) * 257 : scan_scratch_elems(nmax);
    Fr* scratch = nullptr;
    ZCHK(poly_selftest_scratch(cap, &scratch));
    const PlonkScratch w{nullptr, scratch, cap, nullptr, 0, nullptr, nullptr};
    return op ? run_scan_batch<OpMul>(w, jobs, (int)count, st, chunk) : run_scan_batch<OpAdd>(w, jobs, (int)count, st, chunk);
} ZKP_CATCH_INT

int zkp_selftest_poly_scale_pow_dev(const void* d_in, size_t n, const uint64_t base[4], uint64_t e0, unsigned chunk, void* d_out,
                                    void* stream) try {
    if (!base || (n && (!d_in || !d_out))) return fail(ZKP_E_ARG, "null argument");
    if (chunk > SCALE_MAX_CHUNK) return fail(ZKP_E_ARG, "chunk must be 0 (the production rule) or 1..8 elements per thread");
    if (n > POLY_SELFTEST_MAX) return fail(ZKP_E_SIZE, "a polynomial self-test takes at most 2^22 elements per vector");
    if (fr_ranges_clash(d_out, n, d_in, n, true)) return fail(ZKP_E_ARG, "d_out overlaps d_in (in place is d_out == d_in)");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    ScalePowBatch b;
    std::memset(&b, 0, sizeof b);
    b.chunk = chunk ? chunk : scale_chunk_for(n);
    b.job[0] = ScalePowJob{reinterpret_cast<const Fr*>(d_in), reinterpret_cast<Fr*>(d_out), n};
    b.sp[0] = scale_pow_params(HFr::load(base), e0, b.chunk);
    hipLaunchKernelGGL(fr_scale_pow_kernel, scale_pow_grid(n, b.chunk, 1), dim3(PK_THREADS), 0, st, b);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_selftest_poly_div_linear_dev(size_t count, const void* const* d_c, const size_t* len, const uint64_t* z, void* const* d_out,
                                     unsigned chunk, void* stream) try {
    if (!d_c || !len || !z || !d_out) return fail(ZKP_E_ARG, "null argument");
    if (count < 1 || count > 2) return fail(ZKP_E_ARG, "a division launch takes one or two requests");
    if (chunk > SCALE_MAX_CHUNK) return fail(ZKP_E_ARG, "chunk must be 0 (the production rule) or 1..8 elements per thread");
    DivReq rq[2];
    uint64_t ev_elems = 0, nmax = 0;
    for (size_t i = 0; i < count; i++) {
        if (len[i] > 1 && (!d_c[i] || !d_out[i])) return fail(ZKP_E_ARG, "null argument");
        if (len[i] > POLY_SELFTEST_MAX) return fail(ZKP_E_SIZE, "a polynomial self-test takes at most 2^22 elements per vector");
        rq[i] = DivReq{reinterpret_cast<const Fr*>(d_c[i]), len[i], HFr::load(z + 4 * i), reinterpret_cast<Fr*>(d_out[i])};
        ev_elems += 2 * (uint64_t)len[i];
        nmax = std::max<uint64_t>(nmax, len[i]);
    }
    for (size_t i = 0; i < count; i++)
        for (size_t k = 0; k < count; k++)
            if (len[i] > 1 && (fr_ranges_clash(d_out[i], len[i] - 1, d_c[k], len[k], false) ||
                               (k != i && len[k] > 1 && fr_ranges_clash(d_out[i], len[i] - 1, d_out[k], len[k] - 1, false))))
                return fail(ZKP_E_ARG, "a quotient may not overlap a dividend or the other quotient");
    CTX_ENTER(-1);
    if (nmax <= 1) return ZKP_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    const uint64_t cap = chunk ? SCAN_MAX_BATCH * scan_blocks_for(nmax, chunk) * 257 : scan_scratch_elems(nmax);
    Fr* scratch = nullptr;
    ZCHK(poly_selftest_scratch(ev_elems + cap, &scratch));
    const PlonkScratch w{scratch, scratch + ev_elems, cap, nullptr, 0, nullptr, nullptr};
    return div_linear_batch_dev(w, rq, (int)count, st, chunk);
} ZKP_CATCH_INT

int zkp_selftest_poly_eval_dev(size_t count, const void* const* d_c, const size_t* len, const uint64_t* z, uint64_t* out, void* stream) try {
    if (count && (!d_c || !len || !z || !out)) return fail(ZKP_E_ARG, "null argument");
    if (count > (size_t)EVAL_MAX_REQ) return fail(ZKP_E_ARG, "an evaluation launch takes at most 8 requests");
    std::vector<EvalReq> reqs(count);
    std::vector<HFr> y(count);
    uint64_t partials = 0;
    for (size_t i = 0; i < count; i++) {
        if (len[i] && !d_c[i]) return fail(ZKP_E_ARG, "null argument");
        if (len[i] > POLY_SELFTEST_MAX) return fail(ZKP_E_SIZE, "a polynomial self-test takes at most 2^22 elements per vector");
        reqs[i] = EvalReq{reinterpret_cast<const Fr*>(d_c[i]), len[i], HFr::load(z + 4 * i), &y[i]};
        partials += (len[i] + EVAL_CHUNK * PK_THREADS - 1) / (EVAL_CHUNK * PK_THREADS);
    }
    CTX_ENTER(-1);
    if (!count) return ZKP_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    Fr* scratch = nullptr;
    ZCHK(poly_selftest_scratch(partials + 1, &scratch));
    const PlonkScratch w{nullptr, nullptr, 0, scratch, (unsigned)partials, nullptr, nullptr};
    ZCHK(eval_many_dev(w, reqs, st));
    for (size_t i = 0; i < count; i++) y[i].store(out + 4 * i);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_selftest_poly_lincomb_dev(size_t terms, const void* const* d_p, const size_t* len, const uint64_t* s, size_t n_out, void* d_out,
                                  void* stream) try {
    if ((terms && (!d_p || !len || !s)) || (n_out && !d_out)) return fail(ZKP_E_ARG, "null argument");
    if (terms > (size_t)LINCOMB_MAX) return fail(ZKP_E_ARG, "a linear combination takes at most 12 terms");
    if (n_out > POLY_SELFTEST_MAX) return fail(ZKP_E_SIZE, "a polynomial self-test takes at most 2^22 elements per vector");
    std::vector<LcTerm> t(terms);
    for (size_t k = 0; k < terms; k++) {
        if (len[k] && !d_p[k]) return fail(ZKP_E_ARG, "null argument");
        if (len[k] > POLY_SELFTEST_MAX) return fail(ZKP_E_SIZE, "a polynomial self-test takes at most 2^22 elements per vector");
        if (fr_ranges_clash(d_out, n_out, d_p[k], len[k], true)) return fail(ZKP_E_ARG, "d_out overlaps a term (in place is d_out == d_p[k])");
        t[k] = LcTerm{reinterpret_cast<const Fr*>(d_p[k]), len[k], HFr::load(s + 4 * k)};
    }
    CTX_ENTER(-1);
    if (!n_out) return ZKP_OK;
    return lincomb_dev(t, reinterpret_cast<Fr*>(d_out), n_out, reinterpret_cast<hipStream_t>(stream));
} ZKP_CATCH_INT

int zkp_selftest_poly_trim_len_dev(const void* d_c, size_t n, size_t* out_len, void* stream) try {
    if (!out_len || (n && !d_c)) return fail(ZKP_E_ARG, "null argument");
    if (n > POLY_SELFTEST_MAX) return fail(ZKP_E_SIZE, "a polynomial self-test takes at most 2^22 elements per vector");
    CTX_ENTER(-1);
    *out_len = 0;
    if (!n) return ZKP_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    Fr* scratch = nullptr;
    ZCHK(poly_selftest_scratch(1, &scratch));
    unsigned long long* d_len = reinterpret_cast<unsigned long long*>(scratch);
    ZCHK(trim_len_enqueue(reinterpret_cast<const Fr*>(d_c), n, d_len, st));
    unsigned long long h = 0;
    HIPCHK(hipMemcpyAsync(&h, d_len, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *out_len = (size_t)h;
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
