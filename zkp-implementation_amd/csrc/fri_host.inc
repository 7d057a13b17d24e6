// fri_host.inc -- host side of the FRI commitment path (included at the end of api.hip): Merkle trees on the GPU,
// the folding/query phases of fri/src/prover.rs:49-168 driven by the host transcript, and the verifier of
// fri/src/verifier.rs:10-127 (host only: two hashes per layer and query).
//
// Flat proof layout (uint64 words; field elements in memory form = Montgomery residues):
//   [0] domain_size  [1] layers = log2(domain_size)  [2] number_of_queries  [3] coset (F::GENERATOR = 7)
//   [4 .. 4+layers)  layers_root        [4+layers]  const_val
//   then for every query, for every layer l (domain d_l = domain_size >> l, depth_l = log2 d_l):
//       index, evaluation, sym_evaluation, auth path (depth_l sibling hashes, leaf level first), sym auth path (depth_l)
//   (a proof over a domain of size 1 has no layers and no query records, prover.rs:90-92)

namespace {

bool fri_zero_as_0() {
    const char* e = getenv("ZKP_FRI_ZERO_AS_0");
    return e && e[0] == '1';
}

size_t merkle_depth(size_t n) {
    size_t d = 0;
    while (((size_t)1 << d) < n) d++;
    return d;
}
size_t merkle_node_count(size_t n) {
    size_t total = n, len = n;
    for (size_t l = 0, d = merkle_depth(n); l < d; l++) {
        len = (len + 1) / 2;
        total += len;
    }
    return total;
}

// MerkleTree::new (merkle_tree.rs:42-63) for n leaves in device memory; nodes = every level, concatenated
int merkle_tree_dev(const uint64_t* d_leaves, size_t n, uint64_t* d_nodes, hipStream_t st) {
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
    bool first = true;
    while (done < depth + 1) {
        MerkleLaunch p;
        std::memset(&p, 0, sizeof p);
        p.leaf_mode = first ? 1 : 0;
        p.zero_as_0 = fri_zero_as_0() ? 1 : 0;
        p.in = first ? d_leaves : d_nodes + off[done - 1];
        p.n_in = first ? n : len[done - 1];
        p.ipl_log = p.n_in >= (1u << 18) ? 2 : 0;
        const size_t cap = (first ? 1 : 0) + p.ipl_log + 8;
        p.levels = (int)std::min(cap, depth + 1 - done);
        for (int k = 0; k < p.levels; k++) p.out[k] = d_nodes + off[done + k];
        const uint64_t span = (uint64_t)MERKLE_BLOCK << p.ipl_log;
        hipLaunchKernelGGL(merkle_levels_kernel, dim3((unsigned)((p.n_in + span - 1) / span)), dim3(MERKLE_BLOCK), 0, st, p);
        HIPCHK(hipGetLastError());
        done += p.levels;
        first = false;
    }
    return ZKP_OK;
}

uint64_t gl_canon(uint64_t mont) { return HGl::load(&mont).from_mont().l[0]; }
uint64_t gl_mont(uint64_t canon) { return HGl::from_u64(canon).l[0]; }

// hasher.rs on the host (verifier only): canonical in, canonical out
uint64_t host_hash_slice(const uint64_t* canon, size_t n, bool z0) {
    Sha256 h;
    for (size_t i = 0; i < n; i++) {
        const std::string s = goldilocks_display(canon[i], z0);
        h.update(s.data(), s.size());
    }
    const auto dg = h.finish();
    unsigned __int128 acc = 0;
    for (int i = 31; i >= 0; i--) acc = (acc * 256 + dg[i]) % Gl::MOD;
    return (uint64_t)acc;
}

// The field-specific parts of the FRI proof shape and verifier (fri/src is generic over F: PrimeField): W words per element,
// the host field type, canonical values, hash / hash_slice, roots of unity and the transcript replay.  Goldilocks here, Fr in
// fri_fr_host.inc (FriFrTraits).
struct FriGlTraits {
    static constexpr size_t W = 1;
    typedef HGl H;
    typedef std::array<uint64_t, 1> C;
    static C canon(const uint64_t* mont) { return C{gl_canon(*mont)}; }
    static C hash(const C* in, size_t n, bool z0) {
        uint64_t v[2] = {in[0][0], n > 1 ? in[1][0] : 0};
        return C{host_hash_slice(v, n, z0)};
    }
    static H root(unsigned log_n) { return gl_root_of_unity(log_n); }
    static int challenges(const uint64_t* roots, size_t L, const uint64_t* cst, size_t nq, uint64_t* r, uint64_t* q) {
        return zkp_fri_challenges(roots, L, *cst, nq, r, q);
    }
};

// Flat proof length: [0] D [1] L [2] nq, W-word coset, roots[L], const_val, then per query and layer l
// index + evaluation + sym_evaluation + 2 depth_l path nodes
template <class T>
size_t fri_proof_words_t(size_t domain_size, size_t nq) {
    const size_t L = merkle_depth(domain_size);
    return 3 + T::W * (L + 2) + nq * (L * (1 + 2 * T::W) + T::W * L * (L + 1));
}
size_t fri_proof_words(size_t domain_size, size_t nq) { return fri_proof_words_t<FriGlTraits>(domain_size, nq); }

// fri/src/verifier.rs:10-127 on the flat proof of either field.  ZKP_OK = accepted; ZKP_E_ARG with the reference's error
// string otherwise.
template <class T>
int fri_verify_t(const uint64_t* proof, size_t words) {
    typedef typename T::H H;
    typedef typename T::C C;
    constexpr size_t W = T::W;
    if (!proof || words < 3 + 2 * W) return fail(ZKP_E_ARG, "malformed proof");
    const size_t D = proof[0], L = proof[1], nq = proof[2];
    if (D == 0 || (D & (D - 1)) || merkle_depth(D) != L || L > 32 || words != fri_proof_words_t<T>(D, nq))
        return fail(ZKP_E_ARG, "malformed proof");
    const bool z0 = fri_zero_as_0();
    const uint64_t* roots = proof + 3 + W;
    const uint64_t* cst_p = roots + W * L;
    std::vector<uint64_t> r(W * L), qs(nq);
    ZCHK(T::challenges(roots, L, cst_p, nq, r.data(), qs.data()));
    const H cst = H::load(cst_p);
    const H two_inv = H::from_u64(2).inverse();
    const uint64_t* p = cst_p + W;
    for (size_t q = 0; q < nq && L; q++) {
        const size_t ch = qs[q] % D;
        H coset = H::load(proof + 3);
        size_t ds = D;
        for (size_t l = 0; l < L; l++, ds /= 2) {  // verify_query, verifier.rs:49-121
            const size_t idx = ch % ds, sym = (idx + ds / 2) % ds, depth = L - l;
            const uint64_t* rec = p;
            p += 1 + W * (2 + 2 * depth);
            if (rec[0] != idx) return fail(ZKP_E_ARG, "wrong index!");
            const C want_root = T::canon(roots + W * l);
            for (int pass = 0; pass < 2; pass++) {  // verify_merkle_proof, merkle_tree.rs:119-135
                size_t c = pass ? sym : idx;
                C pair[2];
                pair[0] = T::canon(rec + 1 + W * pass);
                C h = T::hash(pair, 1, z0);
                const uint64_t* path = rec + 1 + W * (2 + pass * depth);
                for (size_t i = 0; i < depth; i++) {
                    pair[c & 1] = h;
                    pair[1 - (c & 1)] = T::canon(path + W * i);
                    h = T::hash(pair, 2, z0);
                    c /= 2;
                }
                if (h != want_root) return fail(ZKP_E_ARG, "verify Merkle path failed!");
            }
            // q_fold = (r + w) e / (2 w) - (r - w) s / (2 w),  w = omega_ds^idx * coset (verifier.rs:96-101)
            const H w = T::root((unsigned)depth).pow_u64(idx) * coset;
            const H rl = H::load(&r[W * l]), e = H::load(rec + 1), s = H::load(rec + 1 + W);
            const H i2w = two_inv * w.inverse();
            const H qf = (rl + w) * e * i2w - (rl - w) * s * i2w;
            const H expect = l + 1 < L ? H::load(p + 1) : cst;  // next layer's evaluation of this query, or const_val
            if (!(qf == expect)) return fail(ZKP_E_ARG, "folding wrong!");
            coset = coset * coset;
        }
    }
    return ZKP_OK;
}

}  // namespace

extern "C" {

size_t zkp_fri_merkle_node_count(size_t n) { return merkle_node_count(n); }

int zkp_fri_merkle_tree_dev(const void* d_leaves, size_t n, void* d_nodes, void* stream) try {
    if (n && (!d_leaves || !d_nodes)) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(-1);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    return merkle_tree_dev(reinterpret_cast<const uint64_t*>(d_leaves), n, reinterpret_cast<uint64_t*>(d_nodes),
                           reinterpret_cast<hipStream_t>(stream));
} ZKP_CATCH_INT

int zkp_fri_merkle_tree(const uint64_t* leaves, size_t n, uint64_t* nodes_out) try {
    if (n && (!leaves || !nodes_out)) return fail(ZKP_E_ARG, "null argument");
    if (!n) return ZKP_OK;
    CTX_ENTER(-1);
    WsOrder ord(nullptr);
    const size_t total = merkle_node_count(n);
    ZCHK(ctx().tmp.ensure(8 * (n + total)));
    uint64_t* d = reinterpret_cast<uint64_t*>(ctx().tmp.p);
    HIPCHK(hipMemcpyAsync(d, leaves, 8 * n, hipMemcpyHostToDevice, nullptr));
    ZCHK(merkle_tree_dev(d, n, d + n, nullptr));
    HIPCHK(hipMemcpyAsync(nodes_out, d + n, 8 * total, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_fri_challenges(const uint64_t* roots, size_t layers, uint64_t const_val, size_t num_queries, uint64_t* r_out,
                       uint64_t* q_out) try {
    if ((layers && (!roots || !r_out)) || (num_queries && !q_out)) return fail(ZKP_E_ARG, "null argument");
    FriTranscript t(fri_zero_as_0());
    StdRng rng(0);
    for (size_t l = 0; l < layers; l++) {  // verifier.rs:13-21
        t.digest(gl_canon(roots[l]));
        t.rng(&rng);
        r_out[l] = sample_goldilocks(rng);
    }
    t.digest(gl_canon(const_val));
    t.rng(&rng);
    for (size_t i = 0; i < num_queries; i++) q_out[i] = gl_canon(sample_goldilocks(rng));  // transcript.rs:132-137
    return ZKP_OK;
} ZKP_CATCH_INT

void zkp_free(void* p) { std::free(p); }

int zkp_fri_prove(const uint64_t* coeffs, size_t d, size_t blowup, size_t num_queries, uint64_t** out_proof, size_t* out_words) try {
    if (!out_proof || !out_words || (d && !coeffs)) return fail(ZKP_E_ARG, "null argument");
    *out_proof = nullptr;
    *out_words = 0;
    while (d && coeffs[d - 1] == 0) d--;  // DensePolynomial::from_coefficients_vec trims trailing zeros
    if (d == 0) return fail(ZKP_E_ARG, "zero polynomial (assert_eq!(poly.len(), 1), fri/src/prover.rs:72)");
    if (blowup == 0) return fail(ZKP_E_ARG, "blowup_factor is zero");
    if (d > ((size_t)1 << 32) / blowup) return fail(ZKP_E_SIZE, "domain above 2^32 (Goldilocks two-adicity)");
    size_t D = 1;
    while (D < d * blowup) D <<= 1;  // prover.rs:146
    const size_t L = merkle_depth(D);
    const bool z0 = fri_zero_as_0();
    CTX_ENTER(-1);
    hipStream_t st = nullptr;
    WsOrder ord(st);

    // one arena: coefficient ping-pong (2 d), then per layer its evaluations and Merkle nodes
    std::vector<size_t> ev_off(L + 1), nd_off(L + 1);
    size_t words = 2 * d;
    for (size_t l = 0; l < L; l++) {
        ev_off[l] = words;
        words += D >> l;
        nd_off[l] = words;
        words += merkle_node_count(D >> l);
    }
    const size_t rec_words = fri_proof_words(D, num_queries) - (4 + L + 1);
    const size_t out_off = words;
    words += rec_words;
    const size_t tail_off = words;  // roots, constant and remaining length written by fri_tail_kernel
    words += FRI_TAIL_LOG + 8;
    const size_t state_off = words;  // FriTranscriptState (5 words, 8 reserved) + one challenge and one root per large layer
    words += 8 + 2 * (L + 1);
    const size_t small_words = words - tail_off;  // everything the host reads back after the folding phase, contiguous
    ZCHK(ctx().fri_arena.ensure(8 * std::max<size_t>(words, 1)));
    uint64_t* base = reinterpret_cast<uint64_t*>(ctx().fri_arena.p);
    uint64_t* poly[2] = {base, base + d};
    HIPCHK(hipMemcpyAsync(poly[0], coeffs, 8 * d, hipMemcpyHostToDevice, st));

    std::vector<uint64_t> proof(4 + L + 1);
    proof[0] = D;
    proof[1] = L;
    proof[2] = num_queries;
    proof[3] = gl_mont(7);  // F::GENERATOR (fri/src/fields/goldilocks.rs:6), prover.rs:147
    FriTranscript t(z0);
    StdRng rng(0);
    HGl coset = HGl::from_u64(7);
    size_t len = d, dom = D;
    int cur = 0;
    // transcript state and per-layer challenges live on the device: nothing below waits for the GPU until every layer is
    // enqueued (the host only replays the transcript afterwards to continue with the query phase)
    FriTranscriptState hstate;
    {
        const auto& dg = t.data();
        for (int i = 0; i < 8; i++)
            hstate.data[i] = (uint32_t)dg[4 * i] << 24 | (uint32_t)dg[4 * i + 1] << 16 | (uint32_t)dg[4 * i + 2] << 8 | dg[4 * i + 3];
        hstate.index = t.index();
    }
    FriTranscriptState* dstate = reinterpret_cast<FriTranscriptState*>(base + state_off);
    uint64_t* d_r = base + state_off + 8;  // one challenge per large layer
    uint64_t* d_roots = d_r + L + 1;       // and its Merkle root (written by fri_transcript_kernel)
    ZCHK(ctx().fri_small.ensure(8 * small_words, hipHostMallocDefault));  // pinned: a D2H into pageable memory costs ~20 us per call
    uint64_t* h_small = static_cast<uint64_t*>(ctx().fri_small.p);
    HIPCHK(hipMemcpyAsync(dstate, &hstate, sizeof hstate, hipMemcpyHostToDevice, st));
    size_t l = 0;
    auto prep = [&](const uint64_t* src, uint64_t src_len, const uint64_t* r_ptr, const HGl& cs, uint64_t next_dom, uint64_t* next_poly,
                    uint64_t* next_ev) {
        const uint64_t threads = (next_dom + FRI_PREP_CHUNK - 1) / FRI_PREP_CHUNK;
        hipLaunchKernelGGL(fri_fold_prep_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, src, src_len, r_ptr,
                           cs.from_mont().l[0], next_dom, next_poly, next_ev);
    };
    if (L && dom > (size_t)FRI_TAIL_MAX) prep(poly[cur], len, nullptr, coset, dom, nullptr, base + ev_off[0]);  // layer 0 input
    for (; l < L && dom > (size_t)FRI_TAIL_MAX; l++) {  // folding_phase, prover.rs:56-70: the large layers, one at a time
        uint64_t* ev = base + ev_off[l];
        uint64_t* nodes = base + nd_off[l];
        ZCHK(run_ntt<Gl>(reinterpret_cast<Gl*>(ev), (unsigned)merkle_depth(dom), 1, 0, nullptr, st));  // FriLayer::from_poly
        ZCHK(merkle_tree_dev(ev, dom, nodes, st));
        hipLaunchKernelGGL(fri_transcript_kernel, dim3(1), dim3(1), 0, st, dstate, nodes + merkle_node_count(dom) - 1, d_r + l,
                           d_roots + l, z0 ? 1 : 0);
        const size_t nl = (len + 1) / 2;
        const HGl next_coset = coset * coset;
        const size_t next_dom = dom >> 1;
        if (l + 1 < L && next_dom > (size_t)FRI_TAIL_MAX) {  // fold + scaled, padded input of the next large layer
            prep(poly[cur], len, d_r + l, next_coset, next_dom, poly[cur ^ 1], base + ev_off[l + 1]);
        } else {  // the next layer (if any) belongs to the tail kernel, which wants the plain folded coefficients
            hipLaunchKernelGGL(fri_fold_dev_kernel, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st, poly[cur], (uint64_t)len,
                               d_r + l, poly[cur ^ 1]);
        }
        HIPCHK(hipGetLastError());
        cur ^= 1;
        len = nl;
        coset = next_coset;
        dom = next_dom;
    }
    const size_t big = l;
    uint64_t cst = 0;
    const uint64_t* tail_out = h_small;  // host copy of the tail kernel's outputs (valid after the synchronise below)
    if (l < L) {  // the remaining layers (domain <= 2048): one launch, transcript included (fri_tail_kernel)
        FriTailParams tp;
        std::memset(&tp, 0, sizeof tp);
        tp.poly = poly[cur];
        tp.len = (uint32_t)len;
        tp.log_size = (uint32_t)(L - l);
        tp.coset = coset.from_mont().l[0];
        tp.omega = gl_root_of_unity(tp.log_size).from_mont().l[0];
        tp.state = dstate;
        tp.zero_as_0 = z0 ? 1 : 0;
        for (size_t j = 0; l + j < L; j++) {
            tp.evals[j] = base + ev_off[l + j];
            tp.nodes[j] = base + nd_off[l + j];
        }
        tp.out = base + tail_off;
        hipLaunchKernelGGL(fri_tail_kernel, dim3(1), dim3(FRI_TAIL_THREADS), FRI_TAIL_LDS, st, tp);
        HIPCHK(hipGetLastError());
    } else {  // every layer was a large one (not reachable with FRI_TAIL_MAX >= 2) or there are no layers (domain of size 1)
        HIPCHK(hipMemcpyAsync(&cst, poly[cur], 8, hipMemcpyDeviceToHost, st));
    }
    // tail outputs | transcript state | challenges | roots of the large layers: one copy into pinned memory
    HIPCHK(hipMemcpyAsync(h_small, base + tail_off, 8 * small_words, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(&hstate, h_small + (state_off - tail_off), sizeof hstate);
    for (size_t k = 0; k < big; k++) proof[4 + k] = h_small[(state_off - tail_off) + 8 + (L + 1) + k];
    if (l < L) {
        const size_t ts = L - l;
        for (size_t j = 0; j < ts; j++) proof[4 + l + j] = tail_out[j];
        cst = tail_out[ts];
        len = (size_t)tail_out[ts + 1];
    }
    if (L) {  // continue the host transcript where the device left it (the last challenge was already drawn there)
        std::array<uint8_t, 32> dg2;
        for (int i = 0; i < 8; i++) {
            const uint32_t w = hstate.data[i];
            dg2[4 * i] = (uint8_t)(w >> 24); dg2[4 * i + 1] = (uint8_t)(w >> 16); dg2[4 * i + 2] = (uint8_t)(w >> 8); dg2[4 * i + 3] = (uint8_t)w;
        }
        t.resume(dg2, hstate.index, true);
    }
    if (len != 1 || cst == 0) return fail(ZKP_E_ARG, "folded polynomial is zero (assert_eq!(poly.len(), 1), fri/src/prover.rs:72)");
    proof[4 + L] = cst;
    t.digest(gl_canon(cst));
    t.rng(&rng);

    if (L && num_queries) {  // query_phase, prover.rs:84-134
        std::vector<uint64_t> challenges(num_queries), rec_off(num_queries * L);
        for (size_t q = 0; q < num_queries; q++) challenges[q] = gl_canon(sample_goldilocks(rng)) % D;
        size_t o = 0;
        for (size_t q = 0; q < num_queries; q++)
            for (size_t l = 0; l < L; l++) {
                rec_off[q * L + l] = o;
                o += 3 + 2 * (L - l);
            }
        std::vector<FriLayerRef> refs(L);
        for (size_t l = 0; l < L; l++) refs[l] = FriLayerRef{base + ev_off[l], base + nd_off[l], (uint64_t)(D >> l)};
        ZCHK(ctx().fri_meta.ensure(sizeof(FriLayerRef) * L + 8 * num_queries + 8 * num_queries * L));
        char* m = reinterpret_cast<char*>(ctx().fri_meta.p);
        std::vector<char> meta(sizeof(FriLayerRef) * L + 8 * num_queries + 8 * num_queries * L);  // one upload, not three
        std::memcpy(meta.data(), refs.data(), sizeof(FriLayerRef) * L);
        std::memcpy(meta.data() + sizeof(FriLayerRef) * L, challenges.data(), 8 * num_queries);
        std::memcpy(meta.data() + sizeof(FriLayerRef) * L + 8 * num_queries, rec_off.data(), 8 * num_queries * L);
        HIPCHK(hipMemcpyAsync(m, meta.data(), meta.size(), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(fri_gather_kernel, dim3((unsigned)num_queries, (unsigned)L), dim3(64), 0, st,
                           reinterpret_cast<const FriLayerRef*>(m), (uint32_t)L,
                           reinterpret_cast<const uint64_t*>(m + sizeof(FriLayerRef) * L),
                           reinterpret_cast<const uint64_t*>(m + sizeof(FriLayerRef) * L + 8 * num_queries), base + out_off);
        HIPCHK(hipGetLastError());
        proof.resize(4 + L + 1 + rec_words);
        HIPCHK(hipMemcpyAsync(proof.data() + 4 + L + 1, base + out_off, 8 * rec_words, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
    }
    uint64_t* out = static_cast<uint64_t*>(std::malloc(8 * proof.size()));
    if (!out) return fail(ZKP_E_NOMEM, "out of host memory");
    std::memcpy(out, proof.data(), 8 * proof.size());
    *out_proof = out;
    *out_words = proof.size();
    return ZKP_OK;
} ZKP_CATCH_INT

// fri/src/verifier.rs:10-127.  ZKP_OK = accepted; ZKP_E_ARG with the reference's error string otherwise.
int zkp_fri_verify(const uint64_t* proof, size_t words) try {
    return fri_verify_t<FriGlTraits>(proof, words);
} ZKP_CATCH_INT

// ---- plonk/src/challenge.rs ------------------------------------------------------------------------
struct zkp_plonk_transcript {
    PlonkChallengeGenerator gen;
};

int zkp_plonk_transcript_create(zkp_plonk_transcript** out) try {
    if (!out) return fail(ZKP_E_ARG, "null argument");
    *out = new (std::nothrow) zkp_plonk_transcript();
    return *out ? ZKP_OK : fail(ZKP_E_NOMEM, "out of host memory");
} ZKP_CATCH_INT
void zkp_plonk_transcript_destroy(zkp_plonk_transcript* t) { delete t; }

int zkp_plonk_transcript_feed(zkp_plonk_transcript* t, const uint64_t xy[12], uint8_t is_inf) try {
    if (!t || (!is_inf && !xy)) return fail(ZKP_E_ARG, "null argument");
    uint64_t x[6] = {0}, y[6] = {0};
    if (!is_inf) {
        const HFq cx = HFq::load(xy).from_mont(), cy = HFq::load(xy + 6).from_mont();
        std::memcpy(x, cx.l, 48);
        std::memcpy(y, cy.l, 48);
    }
    t->gen.feed(x, y, is_inf != 0);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_plonk_transcript_challenges(zkp_plonk_transcript* t, size_t n, uint64_t* out) try {
    if (!t || (n && !out)) return fail(ZKP_E_ARG, "null argument");
    if (!t->gen.generate(n, out)) return fail(ZKP_E_ARG, "I'm hungry! Feed me something first");
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
