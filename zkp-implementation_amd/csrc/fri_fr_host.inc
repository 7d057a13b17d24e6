// fri_fr_host.inc -- host side of the FRI commitment path over BLS12-381 Fr (included after fri_host.inc, whose helpers it
// shares: merkle_depth / merkle_node_count, fri_zero_as_0, FriTranscript).  Same structure as the Goldilocks driver: one
// arena, every layer enqueued back to back with the transcript on the device, one D2H of the small outputs, the host replay of
// the last transcript step, and the gather.  The verifier runs on the host.
//
// Flat proof layout (uint64 words; field elements are 4-word memory form = Montgomery residues):
//   [0] domain_size  [1] layers = log2(domain_size)  [2] number_of_queries
//   [3 .. 7) coset (F::GENERATOR = 7)   then layers_root[layers] (4 words each), then const_val (4 words)
//   then for every query, for every layer l (domain d_l = domain_size >> l, depth_l = log2 d_l):
//       index (1 word), evaluation, sym_evaluation, auth path (depth_l sibling hashes, leaf level first), sym auth path

namespace {

constexpr size_t FR_W = 4;  // words per element

// the Fr side of the shared FRI shape (FriGlTraits in fri_host.inc): 4-word elements, 77-digit Display, digest mod r
struct FriFrTraits {
    static constexpr size_t W = FR_W;
    typedef HFr H;
    typedef std::array<uint64_t, 4> C;
    static C canon(const uint64_t* mont) {
        const HFr c = HFr::load(mont).from_mont();
        C out;
        std::memcpy(out.data(), c.l, 32);
        return out;
    }
    static std::string display_mont(const uint64_t* mont, bool z0) { return fr_display(canon(mont).data(), z0); }
    // hasher.rs on the host: SHA-256 of the concatenated Display strings, F::from_le_bytes_mod_order; canonical out
    static C hash(const C* in, size_t n, bool z0) {
        Sha256 h;
        for (size_t i = 0; i < n; i++) {
            const std::string s = fr_display(in[i].data(), z0);
            h.update(s.data(), s.size());
        }
        const auto dg = h.finish();
        C out;
        for (int k = 0; k < 4; k++) {
            out[k] = 0;
            for (int b = 7; b >= 0; b--) out[k] = out[k] << 8 | dg[8 * k + b];
        }
        const uint64_t* m = FrTag::ctx().p;
        for (int s = 0; s < 2; s++)  // < 2^256 < 3 r
            if (Mont<4>::ge(out.data(), m)) Mont<4>::sub(out.data(), out.data(), m);
        return out;
    }
    static H root(unsigned log_n) { return fr_root_of_unity(log_n); }
    static int challenges(const uint64_t* roots, size_t L, const uint64_t* cst, size_t nq, uint64_t* r, uint64_t* q) {
        return zkp_fri_challenges_fr(roots, L, cst, nq, r, q);
    }
};

// layers with at most 2^fri_fr_tail_log() points (default 512) run in fri_fr_tail_kernel.  ZKP_FRI_FR_TAIL_LOG (0 .. FR_TAIL_LOG) overrides the
// default for measurements: 0 sends every layer through the large-layer launches.
unsigned fri_fr_tail_log() {
    const char* e = getenv("ZKP_FRI_FR_TAIL_LOG");
    if (!e || !*e) return FR_TAIL_DEFAULT_LOG;
    const long v = strtol(e, nullptr, 10);
    return v < 0 ? 0u : v > FR_TAIL_LOG ? (unsigned)FR_TAIL_LOG : (unsigned)v;
}

size_t fri_fr_proof_words(size_t domain_size, size_t nq) { return fri_proof_words_t<FriFrTraits>(domain_size, nq); }

// MerkleTree::new over Fr for n leaves in device memory; nodes = every level, concatenated
int merkle_tree_fr_dev(const Fr* d_leaves, size_t n, Fr* d_nodes, hipStream_t st) {
    if (n == 0) return ZKP_OK;
    const size_t depth = merkle_depth(n);
    std::vector<size_t> off(depth + 2), len(depth + 1);
    off[0] = 0;
    len[0] = n;
    for (size_t l = 0; l <= depth; l++) {
        off[l + 1] = off[l] + len[l];
        if (l < depth) len[l + 1] = (len[l] + 1) / 2;
    }
    ProfScope ps("fri_merkle", st);
    size_t done = 0;  // levels written so far
    while (done < depth + 1) {
        FrMerkleLaunch p;
        std::memset(&p, 0, sizeof p);
        const bool first = done == 0;
        p.leaf_mode = first ? 1 : 0;
        p.zero_as_0 = fri_zero_as_0() ? 1 : 0;
        p.in = first ? d_leaves : d_nodes + off[done - 1];
        p.n_in = first ? n : len[done - 1];
        p.levels = (int)std::min<size_t>((first ? 1 : 0) + 8, depth + 1 - done);
        for (int k = 0; k < p.levels; k++) p.out[k] = d_nodes + off[done + k];
        hipLaunchKernelGGL(fri_fr_merkle_levels_kernel, dim3((unsigned)((p.n_in + FR_MERKLE_BLOCK - 1) / FR_MERKLE_BLOCK)),
                           dim3(FR_MERKLE_BLOCK), 0, st, p);
        HIPCHK(hipGetLastError());
        done += p.levels;
    }
    return ZKP_OK;
}

}  // namespace

extern "C" {

int zkp_fri_layer_eval_fr(const uint64_t* coeffs, size_t d, const uint64_t coset[4], unsigned log_D, uint64_t* out) try {
    if ((d && !coeffs) || !out || !coset) return fail(ZKP_E_ARG, "null argument");
    if (log_D > 32) return fail(ZKP_E_ARG, "log_D > 32");
    const size_t D = (size_t)1 << log_D;
    if (d > D) return fail(ZKP_E_ARG, "more coefficients than domain points");
    CTX_ENTER(-1);
    WsOrder ord(nullptr);
    ZCHK(ctx().tmp.ensure(32 * D));
    HIPCHK(hipMemsetAsync(ctx().tmp.p, 0, 32 * D, nullptr));
    if (d) HIPCHK(hipMemcpyAsync(ctx().tmp.p, coeffs, 32 * d, hipMemcpyHostToDevice, nullptr));
    ZCHK(run_ntt<Fr>(reinterpret_cast<Fr*>(ctx().tmp.p), log_D, 1, 0, coset, nullptr));
    HIPCHK(hipMemcpyAsync(out, ctx().tmp.p, 32 * D, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_fri_fold_fr(const uint64_t* coeffs, size_t d, const uint64_t r[4], uint64_t* out) try {
    if (!r || (d && (!coeffs || !out))) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(-1);
    if (!d) return ZKP_OK;
    WsOrder ord(nullptr);
    const size_t m = (d + 1) / 2;
    ZCHK(ctx().tmp.ensure(32 * (d + m + 1)));
    Fr* dc = reinterpret_cast<Fr*>(ctx().tmp.p);
    HIPCHK(hipMemcpyAsync(dc, coeffs, 32 * d, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(dc + d + m, r, 32, hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(fri_fr_fold_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, dc, (uint64_t)d, dc + d + m,
                       dc + d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dc + d, 32 * m, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_fri_merkle_tree_fr_dev(const void* d_leaves, size_t n, void* d_nodes, void* stream) try {
    if (n && (!d_leaves || !d_nodes)) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(-1);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    return merkle_tree_fr_dev(reinterpret_cast<const Fr*>(d_leaves), n, reinterpret_cast<Fr*>(d_nodes),
                              reinterpret_cast<hipStream_t>(stream));
} ZKP_CATCH_INT

int zkp_fri_merkle_tree_fr(const uint64_t* leaves, size_t n, uint64_t* nodes_out) try {
    if (n && (!leaves || !nodes_out)) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    WsOrder ord(nullptr);
    const size_t total = merkle_node_count(n);
    ZCHK(ctx().tmp.ensure(32 * (n + total)));
    Fr* d = reinterpret_cast<Fr*>(ctx().tmp.p);
    HIPCHK(hipMemcpyAsync(d, leaves, 32 * n, hipMemcpyHostToDevice, nullptr));
    ZCHK(merkle_tree_fr_dev(d, n, d + n, nullptr));
    HIPCHK(hipMemcpyAsync(nodes_out, d + n, 32 * total, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_fri_challenges_fr(const uint64_t* roots, size_t layers, const uint64_t const_val[4], size_t num_queries, uint64_t* r_out,
                          uint64_t* q_out) try {
    if ((layers && (!roots || !r_out)) || (num_queries && !q_out) || !const_val) return fail(ZKP_E_ARG, "null argument");
    const bool z0 = fri_zero_as_0();
    FriTranscript t(z0);
    StdRng rng(0);
    for (size_t l = 0; l < layers; l++) {  // verifier.rs:13-21
        t.digest_display(FriFrTraits::display_mont(roots + FR_W * l, z0));
        t.rng(&rng);
        const auto v = sample_bls_fr(rng);
        std::memcpy(r_out + FR_W * l, v.data(), 32);
    }
    t.digest_display(FriFrTraits::display_mont(const_val, z0));
    t.rng(&rng);
    for (size_t i = 0; i < num_queries; i++) {  // transcript.rs:132-137: into_bigint().as_ref()[0]
        const auto v = sample_bls_fr(rng);
        q_out[i] = FriFrTraits::canon(v.data())[0];
    }
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_fri_prove_fr(const uint64_t* coeffs, size_t d, size_t blowup, size_t num_queries, uint64_t** out_proof,
                     size_t* out_words) try {
    if (!out_proof || !out_words || (d && !coeffs)) return fail(ZKP_E_ARG, "null argument");
    *out_proof = nullptr;
    *out_words = 0;
    auto is_zero = [&](size_t i) { return (coeffs[FR_W * i] | coeffs[FR_W * i + 1] | coeffs[FR_W * i + 2] | coeffs[FR_W * i + 3]) == 0; };
    while (d && is_zero(d - 1)) d--;  // DensePolynomial::from_coefficients_vec trims trailing zeros
    if (d == 0) return fail(ZKP_E_ARG, "zero polynomial (assert_eq!(poly.len(), 1), fri/src/prover.rs:72)");
    if (blowup == 0) return fail(ZKP_E_ARG, "blowup_factor is zero");
    if (d > ((size_t)1 << 32) / blowup) return fail(ZKP_E_SIZE, "domain above 2^32 (Fr two-adicity)");
    size_t D = 1;
    while (D < d * blowup) D <<= 1;  // prover.rs:146
    const size_t L = merkle_depth(D);
    const bool z0 = fri_zero_as_0();
    CTX_ENTER(-1);
    hipStream_t st = nullptr;
    WsOrder ord(st);

    // one arena (in elements): coefficient ping-pong (2 d), per layer its evaluations and Merkle nodes, the query records, then
    // the small outputs read back after the folding phase: transcript state (2 elements) | challenges[L] | roots[L] | const
    std::vector<size_t> ev_off(L + 1), nd_off(L + 1);
    size_t elems = 2 * d;
    for (size_t l = 0; l < L; l++) {
        ev_off[l] = elems;
        elems += D >> l;
        nd_off[l] = elems;
        elems += merkle_node_count(D >> l);
    }
    const size_t rec_words = fri_fr_proof_words(D, num_queries) - (3 + FR_W * (L + 2));
    const size_t out_off = elems;
    elems += (rec_words + FR_W - 1) / FR_W;
    const size_t small_off = elems;
    const size_t r_off = small_off + 2, root_off = r_off + L, cst_off = root_off + L;
    elems = cst_off + 1;
    const size_t small_elems = elems - small_off;
    static_assert(sizeof(FriTranscriptState) <= 2 * sizeof(Fr), "transcript state fits two elements");
    ZCHK(ctx().fri_arena.ensure(sizeof(Fr) * elems));
    Fr* base = reinterpret_cast<Fr*>(ctx().fri_arena.p);
    Fr* poly[2] = {base, base + d};
    HIPCHK(hipMemcpyAsync(poly[0], coeffs, 32 * d, hipMemcpyHostToDevice, st));

    std::vector<uint64_t> proof(3 + FR_W * (L + 2));
    proof[0] = D;
    proof[1] = L;
    proof[2] = num_queries;
    HFr coset = HFr::from_u64(7);  // F::GENERATOR of ark-bls12-381 Fr, prover.rs:147
    std::memcpy(&proof[3], coset.l, 32);
    FriTranscript t(z0);
    StdRng rng(0);
    FriTranscriptState hstate;
    {
        const auto& dg = t.data();
        for (int i = 0; i < 8; i++)
            hstate.data[i] = (uint32_t)dg[4 * i] << 24 | (uint32_t)dg[4 * i + 1] << 16 | (uint32_t)dg[4 * i + 2] << 8 | dg[4 * i + 3];
        hstate.index = t.index();
    }
    FriTranscriptState* dstate = reinterpret_cast<FriTranscriptState*>(base + small_off);
    ZCHK(ctx().fri_small.ensure(sizeof(Fr) * small_elems, hipHostMallocDefault));
    Fr* h_small = static_cast<Fr*>(ctx().fri_small.p);
    HIPCHK(hipMemcpyAsync(dstate, &hstate, sizeof hstate, hipMemcpyHostToDevice, st));
    auto to_dev = [](const HFr& x) {
        Fr c;
        std::memcpy(c.l, x.l, 32);  // memory form = the device's Montgomery form
        return c;
    };
    auto prep = [&](const Fr* src, uint64_t src_len, const Fr* r_ptr, const HFr& cs, uint64_t next_dom, Fr* next_poly, Fr* next_ev) {
        const uint64_t per_block = (uint64_t)FR_PREP_THREADS * FR_PREP_CHUNK;
        ProfScope ps("fri_fold", st);
        hipLaunchKernelGGL(fri_fr_fold_prep_kernel, dim3((unsigned)((next_dom + per_block - 1) / per_block)), dim3(FR_PREP_THREADS), 0,
                           st, src, src_len, r_ptr, to_dev(cs), to_dev(cs.pow_u64(FR_PREP_THREADS)), next_dom, next_poly, next_ev);
    };
    const size_t tail_max = (size_t)1 << fri_fr_tail_log();
    size_t len = d, dom = D;
    int cur = 0;
    size_t l = 0;
    if (L && dom > tail_max) prep(poly[cur], len, nullptr, coset, dom, nullptr, base + ev_off[0]);  // layer 0 input
    for (; l < L && dom > tail_max; l++) {  // folding_phase, prover.rs:56-70: the large layers, nothing waits for the GPU
        Fr* ev = base + ev_off[l];
        Fr* nodes = base + nd_off[l];
        ZCHK(run_ntt<Fr>(ev, (unsigned)merkle_depth(dom), 1, 0, nullptr, st));  // FriLayer::from_poly on the scaled input
        ZCHK(merkle_tree_fr_dev(ev, dom, nodes, st));
        {
            ProfScope ps("fri_transcript", st);
            hipLaunchKernelGGL(fri_fr_transcript_kernel, dim3(1), dim3(1), 0, st, dstate, nodes + merkle_node_count(dom) - 1,
                               base + r_off + l, base + root_off + l, z0 ? 1 : 0);
        }
        const size_t nl = (len + 1) / 2;
        const HFr next_coset = coset * coset;
        if (l + 1 < L && (dom >> 1) > tail_max) {  // fold + scaled, padded input of the next large layer
            prep(poly[cur], len, base + r_off + l, next_coset, dom >> 1, poly[cur ^ 1], base + ev_off[l + 1]);
        } else {  // plain fold: the tail kernel's coefficients, or (no tail) the final constant next to the small outputs
            hipLaunchKernelGGL(fri_fr_fold_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st, poly[cur], (uint64_t)len,
                               base + r_off + l, l + 1 < L ? poly[cur ^ 1] : base + cst_off);
        }
        HIPCHK(hipGetLastError());
        cur ^= 1;
        len = nl;
        coset = next_coset;
        dom >>= 1;
    }
    if (l < L) {  // the remaining layers (domain <= tail_max): one launch, transcript included (fri_fr_tail_kernel)
        FriFrTailParams tp;
        std::memset(&tp, 0, sizeof tp);
        tp.poly = poly[cur];
        tp.len = (uint32_t)len;
        tp.log_size = (uint32_t)(L - l);
        tp.coset = to_dev(coset);
        tp.coset_stride = to_dev(coset.pow_u64(FR_TAIL_THREADS));
        tp.omega = to_dev(fr_root_of_unity(tp.log_size));
        tp.state = dstate;
        tp.zero_as_0 = z0 ? 1 : 0;
        for (size_t j = 0; l + j < L; j++) {
            tp.evals[j] = base + ev_off[l + j];
            tp.nodes[j] = base + nd_off[l + j];
        }
        tp.roots = base + root_off + l;
        tp.r_out = base + r_off + l;
        tp.cst_out = base + cst_off;
        ZCHK(allow_big_lds(fri_fr_tail_kernel));
        ProfScope ps("fri_tail", st);
        hipLaunchKernelGGL(fri_fr_tail_kernel, dim3(1), dim3(FR_TAIL_THREADS), FR_TAIL_LDS, st, tp);
        HIPCHK(hipGetLastError());
    }
    if (!L) HIPCHK(hipMemcpyAsync(base + cst_off, poly[0], 32, hipMemcpyDeviceToDevice, st));
    HIPCHK(hipMemcpyAsync(h_small, base + small_off, sizeof(Fr) * small_elems, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(&hstate, h_small, sizeof hstate);
    for (size_t k = 0; k < L; k++) std::memcpy(&proof[3 + FR_W * (1 + k)], h_small + (root_off - small_off) + k, 32);
    uint64_t cst[4];
    std::memcpy(cst, h_small + (cst_off - small_off), 32);
    if (L) {  // continue the host transcript where the device left it (the last challenge was already drawn there)
        std::array<uint8_t, 32> dg2;
        for (int i = 0; i < 8; i++) {
            const uint32_t w = hstate.data[i];
            dg2[4 * i] = (uint8_t)(w >> 24); dg2[4 * i + 1] = (uint8_t)(w >> 16); dg2[4 * i + 2] = (uint8_t)(w >> 8); dg2[4 * i + 3] = (uint8_t)w;
        }
        t.resume(dg2, hstate.index, true);
    }
    if ((cst[0] | cst[1] | cst[2] | cst[3]) == 0)
        return fail(ZKP_E_ARG, "folded polynomial is zero (assert_eq!(poly.len(), 1), fri/src/prover.rs:72)");
    std::memcpy(&proof[3 + FR_W * (L + 1)], cst, 32);
    t.digest_display(FriFrTraits::display_mont(cst, z0));
    t.rng(&rng);

    if (L && num_queries) {  // query_phase, prover.rs:84-134
        std::vector<uint64_t> challenges(num_queries), rec_off(num_queries * L);
        for (size_t q = 0; q < num_queries; q++) {
            const auto v = sample_bls_fr(rng);
            challenges[q] = FriFrTraits::canon(v.data())[0] % D;
        }
        size_t o = 0;
        for (size_t q = 0; q < num_queries; q++)
            for (size_t l = 0; l < L; l++) {
                rec_off[q * L + l] = o;
                o += 1 + FR_W * (2 + 2 * (L - l));
            }
        std::vector<FriFrLayerRef> refs(L);
        for (size_t l = 0; l < L; l++) refs[l] = FriFrLayerRef{base + ev_off[l], base + nd_off[l], (uint64_t)(D >> l)};
        const size_t meta_bytes = sizeof(FriFrLayerRef) * L + 8 * num_queries + 8 * num_queries * L;
        ZCHK(ctx().fri_meta.ensure(meta_bytes));
        char* m = reinterpret_cast<char*>(ctx().fri_meta.p);
        std::vector<char> meta(meta_bytes);  // one upload, not three
        std::memcpy(meta.data(), refs.data(), sizeof(FriFrLayerRef) * L);
        std::memcpy(meta.data() + sizeof(FriFrLayerRef) * L, challenges.data(), 8 * num_queries);
        std::memcpy(meta.data() + sizeof(FriFrLayerRef) * L + 8 * num_queries, rec_off.data(), 8 * num_queries * L);
        HIPCHK(hipMemcpyAsync(m, meta.data(), meta.size(), hipMemcpyHostToDevice, st));
        uint64_t* d_out = reinterpret_cast<uint64_t*>(base + out_off);
        ProfScope ps("fri_gather", st);
        hipLaunchKernelGGL(fri_fr_gather_kernel, dim3((unsigned)num_queries, (unsigned)L), dim3(64), 0, st,
                           reinterpret_cast<const FriFrLayerRef*>(m), (uint32_t)L,
                           reinterpret_cast<const uint64_t*>(m + sizeof(FriFrLayerRef) * L),
                           reinterpret_cast<const uint64_t*>(m + sizeof(FriFrLayerRef) * L + 8 * num_queries), d_out);
        HIPCHK(hipGetLastError());
        const size_t head = proof.size();
        proof.resize(head + rec_words);
        HIPCHK(hipMemcpyAsync(proof.data() + head, d_out, 8 * rec_words, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    uint64_t* out = static_cast<uint64_t*>(std::malloc(8 * proof.size()));
    if (!out) return fail(ZKP_E_NOMEM, "out of host memory");
    std::memcpy(out, proof.data(), 8 * proof.size());
    *out_proof = out;
    *out_words = proof.size();
    return ZKP_OK;
} ZKP_CATCH_INT

// fri/src/verifier.rs:10-127 over Fr (fri_verify_t in fri_host.inc).  ZKP_OK = accepted; ZKP_E_ARG with the reference's error
// string otherwise.
int zkp_fri_verify_fr(const uint64_t* proof, size_t words) try {
    return fri_verify_t<FriFrTraits>(proof, words);
} ZKP_CATCH_INT

}  // extern "C"
