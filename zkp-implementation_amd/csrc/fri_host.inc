// fri_host.inc -- host side of the FRI commitment path (included at the end of api.hip), ONE implementation over a traits
// type per field (fri/src is generic over F: PrimeField): Merkle trees on the GPU, the folding / query phases of
// fri/src/prover.rs:49-168 with the transcript on the device, the challenges replay, and the verifier of
// fri/src/verifier.rs:10-127 (host only: two hashes per layer and query).
//
// Flat proof layout (uint64 words; a field element is W words in memory form = Montgomery residue; W = 1 Goldilocks, 4 Fr):
//   [0] domain_size  [1] layers = log2(domain_size)  [2] number_of_queries  then coset (F::GENERATOR = 7),
//   layers_root[layers], const_val;
//   then for every query, for every layer l (domain d_l = domain_size >> l, depth_l = log2 d_l):
//       index (1 word), evaluation, sym_evaluation, auth path (depth_l sibling hashes, leaf level first), sym auth path (depth_l)
//   (a proof over a domain of size 1 has no layers and no query records, prover.rs:90-92)

namespace {

bool fri_zero_as_0() { return knob_flag(KNOB_FRI_ZERO_AS_0); }

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

// What the shared code below needs to know about a field.  Proof shape and verifier: W words per element, the host field
// type H, canonical values C, hash / hash_slice, roots of unity.  Prover: the device side F (fri.hpp / fri_fr.hpp) with its
// element E, Display and UniformRand of a memory-form element, the tail threshold, the Merkle launch geometry, and which of
// the driver's phases are recorded.  A scalar (coset, root of unity, stride, challenge) goes to a kernel as
// HostField<E>::dev(x): the canonical value for Goldilocks, the Montgomery residue for Fr.
struct FriGlTraits {
    static constexpr size_t W = 1;
    typedef HGl H;
    typedef std::array<uint64_t, 1> C;
    typedef FriGl F;
    typedef Gl E;
    static constexpr const char* TWO_ADICITY = "domain above 2^32 (Goldilocks two-adicity)";
    static C canon(const uint64_t* mont) { return C{HGl::load(mont).from_mont().l[0]}; }
    static std::string display(const uint64_t* mont, bool z0) { return goldilocks_display(canon(mont)[0], z0); }
    static void sample(StdRng& rng, uint64_t* mont) { *mont = sample_goldilocks(rng); }
    // hasher.rs on the host (verifier only): canonical in, canonical out
    static C hash(const C* in, size_t n, bool z0) {
        Sha256 h;
        for (size_t i = 0; i < n; i++) {
            const std::string s = goldilocks_display(in[i][0], z0);
            h.update(s.data(), s.size());
        }
        const auto dg = h.finish();
        unsigned __int128 acc = 0;
        for (int i = 31; i >= 0; i--) acc = (acc * 256 + dg[i]) % Gl::MOD;
        return C{(uint64_t)acc};
    }
    static H root(unsigned log_n) { return gl_root_of_unity(log_n); }
    static unsigned tail_log() { return FriGl::TAIL_LOG; }
    // bench.py times the Goldilocks proof with profiling ON and every recorded scope costs two ~5 us markers inside that call
    // (ProfScope): only fri_merkle and the NTT passes are recorded for this field, none of the driver's own phases
    static const char* phase(const char*) { return nullptr; }
    // merkle_levels_kernel on `left` remaining levels: 4 inputs per lane for large levels (throughput), 1 for small ones
    // (shortest chain), up to 8 more levels through LDS; returns the levels written
    static size_t merkle_launch(const E* in, size_t n_in, bool leaf_mode, size_t left, E* const* out, bool z0, hipStream_t st) {
        MerkleLaunch p;
        std::memset(&p, 0, sizeof p);
        p.in = reinterpret_cast<const uint64_t*>(in);
        p.n_in = n_in;
        p.leaf_mode = leaf_mode ? 1 : 0;
        p.zero_as_0 = z0 ? 1 : 0;
        p.ipl_log = n_in >= (1u << 18) ? 2 : 0;
        p.levels = (int)std::min<size_t>((leaf_mode ? 1 : 0) + p.ipl_log + 8, left);
        for (int k = 0; k < p.levels; k++) p.out[k] = reinterpret_cast<uint64_t*>(out[k]);
        const uint64_t span = (uint64_t)MERKLE_BLOCK << p.ipl_log;
        hipLaunchKernelGGL(merkle_levels_kernel, dim3((unsigned)((n_in + span - 1) / span)), dim3(MERKLE_BLOCK), 0, st, p);
        return (size_t)p.levels;
    }
};

// 4-word elements, 77-digit Display, digest mod r
struct FriFrTraits {
    static constexpr size_t W = 4;
    typedef HFr H;
    typedef std::array<uint64_t, 4> C;
    typedef FriFr F;
    typedef Fr E;
    static constexpr const char* TWO_ADICITY = "domain above 2^32 (Fr two-adicity)";
    static C canon(const uint64_t* mont) {
        const HFr c = HFr::load(mont).from_mont();
        C out;
        std::memcpy(out.data(), c.l, 32);
        return out;
    }
    static std::string display(const uint64_t* mont, bool z0) { return fr_display(canon(mont).data(), z0); }
    static void sample(StdRng& rng, uint64_t* mont) { std::memcpy(mont, sample_bls_fr(rng).data(), 32); }
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
    // layers with at most 2^tail_log() points (default 2^9: DESIGN 4.5 has 2^20 proofs at 2^8 / 2^9 / 2^10 within 1 %) run in the
    // tail kernel.  ZKP_FRI_FR_TAIL_LOG (0 .. FriFr::TAIL_LOG) overrides the default for measurements: 0 sends every layer through
    // the large-layer launches.
    static unsigned tail_log() {
        static_assert(kKnobs[KNOB_FRI_FR_TAIL_LOG].hi == FriFr::TAIL_LOG, "knobs.hpp: the tail kernel's capacity");
        return (unsigned)knob_int(KNOB_FRI_FR_TAIL_LOG);
    }
    static const char* phase(const char* name) { return name; }
    // fri_fr_merkle_levels_kernel: one input per lane, up to 8 more levels through LDS
    static size_t merkle_launch(const E* in, size_t n_in, bool leaf_mode, size_t left, E* const* out, bool z0, hipStream_t st) {
        FrMerkleLaunch p;
        std::memset(&p, 0, sizeof p);
        p.in = in;
        p.n_in = n_in;
        p.leaf_mode = leaf_mode ? 1 : 0;
        p.zero_as_0 = z0 ? 1 : 0;
        p.levels = (int)std::min<size_t>((leaf_mode ? 1 : 0) + 8, left);
        for (int k = 0; k < p.levels; k++) p.out[k] = out[k];
        hipLaunchKernelGGL(fri_fr_merkle_levels_kernel, dim3((unsigned)((n_in + FR_MERKLE_BLOCK - 1) / FR_MERKLE_BLOCK)),
                           dim3(FR_MERKLE_BLOCK), 0, st, p);
        return (size_t)p.levels;
    }
};

// MerkleTree::new (merkle_tree.rs:42-63) for n leaves in device memory; nodes = every level, concatenated
template <class T>
int merkle_tree_dev_t(const typename T::E* d_leaves, size_t n, typename T::E* d_nodes, hipStream_t st) {
    if (n == 0) return ZKP_OK;
    const size_t depth = merkle_depth(n);
    std::vector<typename T::E*> level(depth + 1);
    std::vector<size_t> len(depth + 1);
    level[0] = d_nodes;
    len[0] = n;
    for (size_t l = 0; l < depth; l++) {
        level[l + 1] = level[l] + len[l];
        len[l + 1] = (len[l] + 1) / 2;
    }
    const bool z0 = fri_zero_as_0();
    ProfScope ps("fri_merkle", st);
    for (size_t done = 0; done <= depth;) {  // done = levels written so far; a launch reads the leaves or the level below
        const bool first = done == 0;
        done += T::merkle_launch(first ? d_leaves : level[done - 1], first ? n : len[done - 1], first, depth + 1 - done, &level[done],
                                 z0, st);
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

// The challenges a verifier derives from a proof's roots and constant (verifier.rs:13-21, transcript.rs:132-137): r_out = one
// folding challenge per layer (memory form), q_out = the query challenges (into_bigint().as_ref()[0], not yet reduced)
template <class T>
int fri_challenges_t(const uint64_t* roots, size_t layers, const uint64_t* const_val, size_t num_queries, uint64_t* r_out,
                     uint64_t* q_out) {
    if ((layers && (!roots || !r_out)) || (num_queries && !q_out) || !const_val) return fail(ZKP_E_ARG, "null argument");
    const bool z0 = fri_zero_as_0();
    FriTranscript t(z0);
    StdRng rng(0);
    for (size_t l = 0; l < layers; l++) {
        t.digest_display(T::display(roots + T::W * l, z0));
        t.rng(&rng);
        T::sample(rng, r_out + T::W * l);
    }
    t.digest_display(T::display(const_val, z0));
    t.rng(&rng);
    for (size_t i = 0; i < num_queries; i++) {
        uint64_t v[T::W];
        T::sample(rng, v);
        q_out[i] = T::canon(v)[0];
    }
    return ZKP_OK;
}

// Flat proof length: [0] D [1] L [2] nq, W-word coset, roots[L], const_val, then per query and layer l
// index + evaluation + sym_evaluation + 2 depth_l path nodes
template <class T>
size_t fri_proof_words_t(size_t domain_size, size_t nq) {
    const size_t L = merkle_depth(domain_size);
    return 3 + T::W * (L + 2) + nq * (L * (1 + 2 * T::W) + T::W * L * (L + 1));
}

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
    ZCHK(fri_challenges_t<T>(roots, L, cst_p, nq, r.data(), qs.data()));
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

// FriLayer::from_poly on the host's coefficients: the coset NTT of the zero-padded polynomial over 2^log_D points
template <class T>
int fri_layer_eval_t(const uint64_t* coeffs, size_t d, const uint64_t* coset, unsigned log_D, uint64_t* out) {
    typedef typename T::E E;
    if ((d && !coeffs) || !out || !coset) return fail(ZKP_E_ARG, "null argument");
    if (log_D > 32) return fail(ZKP_E_ARG, "log_D > 32");
    const size_t D = (size_t)1 << log_D;
    if (d > D) return fail(ZKP_E_ARG, "more coefficients than domain points");
    CTX_ENTER(-1);
    WsOrder ord(nullptr);
    ZCHK(ctx().tmp.ensure(sizeof(E) * D));
    HIPCHK(hipMemsetAsync(ctx().tmp.p, 0, sizeof(E) * D, nullptr));
    if (d) HIPCHK(hipMemcpyAsync(ctx().tmp.p, coeffs, sizeof(E) * d, hipMemcpyHostToDevice, nullptr));
    ZCHK(run_ntt<E>(reinterpret_cast<E*>(ctx().tmp.p), log_D, 1, 0, coset, nullptr));
    HIPCHK(hipMemcpyAsync(out, ctx().tmp.p, sizeof(E) * D, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return ZKP_OK;
}

// fold_polynomial (prover.rs:34-42) of d >= 1 host coefficients with the challenge r (memory form); the slot is entered
template <class T>
int fri_fold_t(const uint64_t* coeffs, size_t d, const uint64_t* r, uint64_t* out) {
    typedef typename T::E E;
    WsOrder ord(nullptr);
    const size_t m = (d + 1) / 2;
    ZCHK(ctx().tmp.ensure(sizeof(E) * (d + m + 1)));
    E* dc = reinterpret_cast<E*>(ctx().tmp.p);
    const E rs = HostField<E>::dev(T::H::load(r));
    HIPCHK(hipMemcpyAsync(dc, coeffs, sizeof(E) * d, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(dc + d + m, &rs, sizeof(E), hipMemcpyHostToDevice, nullptr));
    hipLaunchKernelGGL(fri_fold_kernel<typename T::F>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, nullptr, dc, (uint64_t)d,
                       dc + d + m, dc + d);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(out, dc + d, sizeof(E) * m, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return ZKP_OK;
}

// MerkleTree::new of n >= 1 host leaves; the slot is entered
template <class T>
int fri_merkle_tree_t(const uint64_t* leaves, size_t n, uint64_t* nodes_out) {
    typedef typename T::E E;
    WsOrder ord(nullptr);
    const size_t total = merkle_node_count(n);
    ZCHK(ctx().tmp.ensure(sizeof(E) * (n + total)));
    E* d = reinterpret_cast<E*>(ctx().tmp.p);
    HIPCHK(hipMemcpyAsync(d, leaves, sizeof(E) * n, hipMemcpyHostToDevice, nullptr));
    ZCHK(merkle_tree_dev_t<T>(d, n, d + n, nullptr));
    HIPCHK(hipMemcpyAsync(nodes_out, d + n, sizeof(E) * total, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return ZKP_OK;
}

template <class T>
int fri_merkle_tree_on_dev_t(const void* d_leaves, size_t n, void* d_nodes, void* stream) {
    typedef typename T::E E;
    if (n && (!d_leaves || !d_nodes)) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(-1);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    return merkle_tree_dev_t<T>(reinterpret_cast<const E*>(d_leaves), n, reinterpret_cast<E*>(d_nodes), reinterpret_cast<hipStream_t>(stream));
}

// generate_proof (prover.rs:137-168).  One arena, every layer enqueued back to back with the transcript on the device, one D2H
// of the small outputs, the host replay of the last transcript step, and the gather of the query records.
template <class T>
int fri_prove_t(const uint64_t* coeffs, size_t d, size_t blowup, size_t num_queries, uint64_t** out_proof, size_t* out_words) {
    typedef typename T::E E;
    typedef typename T::F F;
    typedef typename T::H H;
    constexpr size_t W = T::W;
    static_assert(sizeof(E) == 8 * W, "memory form of an element");
    if (!out_proof || !out_words || (d && !coeffs)) return fail(ZKP_E_ARG, "null argument");
    *out_proof = nullptr;
    *out_words = 0;
    auto is_zero = [](const uint64_t* x) {
        uint64_t any = 0;
        for (size_t k = 0; k < W; k++) any |= x[k];
        return any == 0;
    };
    while (d && is_zero(coeffs + W * (d - 1))) d--;  // DensePolynomial::from_coefficients_vec trims trailing zeros
    if (d == 0) return fail(ZKP_E_ARG, "zero polynomial (assert_eq!(poly.len(), 1), fri/src/prover.rs:72)");
    if (blowup == 0) return fail(ZKP_E_ARG, "blowup_factor is zero");
    if (d > ((size_t)1 << 32) / blowup) return fail(ZKP_E_SIZE, T::TWO_ADICITY);
    size_t D = 1;
    while (D < d * blowup) D <<= 1;  // prover.rs:146
    const size_t L = merkle_depth(D);
    const bool z0 = fri_zero_as_0();
    CTX_ENTER(-1);
    hipStream_t st = nullptr;
    WsOrder ord(st);

    // one arena (in elements): coefficient ping-pong (2 d), per layer its evaluations and Merkle nodes, the query records, then
    // the small outputs read back after the folding phase: transcript state | challenges[L] (scalars) | roots[L] | const
    std::vector<size_t> ev_off(L + 1), nd_off(L + 1);
    size_t elems = 2 * d;
    for (size_t l = 0; l < L; l++) {
        ev_off[l] = elems;
        elems += D >> l;
        nd_off[l] = elems;
        elems += merkle_node_count(D >> l);
    }
    const size_t head = 3 + W * (L + 2), rec_words = fri_proof_words_t<T>(D, num_queries) - head;
    const size_t out_off = elems;
    elems += (rec_words + W - 1) / W;
    const size_t small_off = elems;
    const size_t r_off = small_off + (sizeof(FriTranscriptState) + sizeof(E) - 1) / sizeof(E), root_off = r_off + L, cst_off = root_off + L;
    elems = cst_off + 1;
    const size_t small_elems = elems - small_off;
    ZCHK(ctx().fri_arena.ensure(sizeof(E) * elems));
    E* base = reinterpret_cast<E*>(ctx().fri_arena.p);
    E* poly[2] = {base, base + d};
    HIPCHK(hipMemcpyAsync(poly[0], coeffs, sizeof(E) * d, hipMemcpyHostToDevice, st));

    std::vector<uint64_t> proof(head);
    proof[0] = D;
    proof[1] = L;
    proof[2] = num_queries;
    H coset = H::from_u64(7);  // F::GENERATOR (fri/src/fields/goldilocks.rs:6, ark-bls12-381 Fr), prover.rs:147
    std::memcpy(&proof[3], coset.l, sizeof(E));
    FriTranscript t(z0);
    StdRng rng(0);
    // transcript state and per-layer challenges live on the device: nothing below waits for the GPU until every layer is
    // enqueued (the host only replays the transcript afterwards to continue with the query phase)
    FriTranscriptState hstate;
    {
        const auto& dg = t.data();
        for (int i = 0; i < 8; i++)
            hstate.data[i] = (uint32_t)dg[4 * i] << 24 | (uint32_t)dg[4 * i + 1] << 16 | (uint32_t)dg[4 * i + 2] << 8 | dg[4 * i + 3];
        hstate.index = t.index();
    }
    FriTranscriptState* dstate = reinterpret_cast<FriTranscriptState*>(base + small_off);
    ZCHK(ctx().fri_small.ensure(sizeof(E) * small_elems, hipHostMallocDefault));  // pinned: a D2H into pageable memory costs ~20 us per call
    E* h_small = static_cast<E*>(ctx().fri_small.p);
    HIPCHK(hipMemcpyAsync(dstate, &hstate, sizeof hstate, hipMemcpyHostToDevice, st));
    auto scalar = [](const H& x) { return HostField<E>::dev(x); };
    auto prep = [&](const E* src, uint64_t src_len, const E* r_ptr, const H& cs, uint64_t next_dom, E* next_poly, E* next_ev) {
        const uint64_t per_block = (uint64_t)F::PREP_THREADS * F::PREP_CHUNK;
        ProfScope ps(T::phase("fri_fold"), st);
        hipLaunchKernelGGL(fri_fold_prep_kernel<F>, dim3((unsigned)((next_dom + per_block - 1) / per_block)), dim3(F::PREP_THREADS), 0, st,
                           src, src_len, r_ptr, scalar(cs), scalar(cs.pow_u64(F::PREP_STEP)), next_dom, next_poly, next_ev);
    };
    const size_t tail_max = (size_t)1 << T::tail_log();
    size_t len = d, dom = D;
    int cur = 0;
    size_t l = 0;
    if (L && dom > tail_max) prep(poly[cur], len, nullptr, coset, dom, nullptr, base + ev_off[0]);  // layer 0 input
    for (; l < L && dom > tail_max; l++) {  // folding_phase, prover.rs:56-70: the large layers, one at a time
        E* ev = base + ev_off[l];
        E* nodes = base + nd_off[l];
        ZCHK(run_ntt<E>(ev, (unsigned)merkle_depth(dom), 1, 0, nullptr, st));  // FriLayer::from_poly on the scaled input
        ZCHK(merkle_tree_dev_t<T>(ev, dom, nodes, st));
        {
            ProfScope ps(T::phase("fri_transcript"), st);
            hipLaunchKernelGGL(fri_transcript_kernel<F>, dim3(1), dim3(1), 0, st, dstate, nodes + merkle_node_count(dom) - 1,
                               base + r_off + l, base + root_off + l, z0 ? 1 : 0);
        }
        const size_t nl = (len + 1) / 2;
        const H next_coset = coset * coset;
        if (l + 1 < L && (dom >> 1) > tail_max) {  // fold + scaled, padded input of the next large layer
            prep(poly[cur], len, base + r_off + l, next_coset, dom >> 1, poly[cur ^ 1], base + ev_off[l + 1]);
        } else {  // plain fold: the tail kernel's coefficients, or (no tail) the final constant next to the small outputs
            hipLaunchKernelGGL(fri_fold_kernel<F>, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, st, poly[cur], (uint64_t)len,
                               base + r_off + l, l + 1 < L ? poly[cur ^ 1] : base + cst_off);
        }
        HIPCHK(hipGetLastError());
        cur ^= 1;
        len = nl;
        coset = next_coset;
        dom >>= 1;
    }
    if (l < L) {  // the remaining layers (domain <= tail_max): one launch, transcript included
        FriTailParams<F> tp;
        std::memset(&tp, 0, sizeof tp);
        tp.poly = poly[cur];
        tp.len = (uint32_t)len;
        tp.log_size = (uint32_t)(L - l);
        tp.coset = scalar(coset);
        tp.coset_stride = scalar(coset.pow_u64(F::TAIL_THREADS));
        tp.omega = scalar(T::root(tp.log_size));
        tp.state = dstate;
        tp.zero_as_0 = z0 ? 1 : 0;
        for (size_t j = 0; l + j < L; j++) {
            tp.evals[j] = base + ev_off[l + j];
            tp.nodes[j] = base + nd_off[l + j];
        }
        tp.roots = base + root_off + l;
        tp.r_out = base + r_off + l;
        tp.cst_out = base + cst_off;
        ProfScope ps(T::phase("fri_tail"), st);
        hipLaunchKernelGGL(fri_tail_kernel<F>, dim3(1), dim3(F::TAIL_THREADS), fri_tail_lds<F>(), st, tp);
        HIPCHK(hipGetLastError());
    }
    if (!L) HIPCHK(hipMemcpyAsync(base + cst_off, poly[0], sizeof(E), hipMemcpyDeviceToDevice, st));  // domain of size 1
    HIPCHK(hipMemcpyAsync(h_small, base + small_off, sizeof(E) * small_elems, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    std::memcpy(&hstate, h_small, sizeof hstate);
    std::memcpy(&proof[3 + W], h_small + (root_off - small_off), sizeof(E) * L);
    uint64_t cst[W];
    std::memcpy(cst, h_small + (cst_off - small_off), sizeof(E));
    if (L) {  // continue the host transcript where the device left it (the last challenge was already drawn there)
        std::array<uint8_t, 32> dg2;
        for (int i = 0; i < 8; i++) {
            const uint32_t w = hstate.data[i];
            dg2[4 * i] = (uint8_t)(w >> 24); dg2[4 * i + 1] = (uint8_t)(w >> 16); dg2[4 * i + 2] = (uint8_t)(w >> 8); dg2[4 * i + 3] = (uint8_t)w;
        }
        t.resume(dg2, hstate.index, true);
    }
    if (is_zero(cst)) return fail(ZKP_E_ARG, "folded polynomial is zero (assert_eq!(poly.len(), 1), fri/src/prover.rs:72)");
    std::memcpy(&proof[3 + W * (L + 1)], cst, sizeof(E));
    t.digest_display(T::display(cst, z0));
    t.rng(&rng);

    if (L && num_queries) {  // query_phase, prover.rs:84-134
        typedef FriLayerRef<E> Ref;
        std::vector<uint64_t> challenges(num_queries), rec_off(num_queries * L);
        for (size_t q = 0; q < num_queries; q++) {
            uint64_t v[W];
            T::sample(rng, v);
            challenges[q] = T::canon(v)[0] % D;
        }
        size_t o = 0;
        for (size_t q = 0; q < num_queries; q++)
            for (size_t l = 0; l < L; l++) {
                rec_off[q * L + l] = o;
                o += 1 + W * (2 + 2 * (L - l));
            }
        std::vector<Ref> refs(L);
        for (size_t l = 0; l < L; l++) refs[l] = Ref{base + ev_off[l], base + nd_off[l], (uint64_t)(D >> l)};
        const size_t meta_bytes = sizeof(Ref) * L + 8 * num_queries + 8 * num_queries * L;
        ZCHK(ctx().fri_meta.ensure(meta_bytes));
        char* m = reinterpret_cast<char*>(ctx().fri_meta.p);
        std::vector<char> meta(meta_bytes);  // one upload, not three
        std::memcpy(meta.data(), refs.data(), sizeof(Ref) * L);
        std::memcpy(meta.data() + sizeof(Ref) * L, challenges.data(), 8 * num_queries);
        std::memcpy(meta.data() + sizeof(Ref) * L + 8 * num_queries, rec_off.data(), 8 * num_queries * L);
        HIPCHK(hipMemcpyAsync(m, meta.data(), meta.size(), hipMemcpyHostToDevice, st));
        uint64_t* d_out = reinterpret_cast<uint64_t*>(base + out_off);
        ProfScope ps(T::phase("fri_gather"), st);
        hipLaunchKernelGGL(fri_gather_kernel<E>, dim3((unsigned)num_queries, (unsigned)L), dim3(64), 0, st,
                           reinterpret_cast<const Ref*>(m), (uint32_t)L, reinterpret_cast<const uint64_t*>(m + sizeof(Ref) * L),
                           reinterpret_cast<const uint64_t*>(m + sizeof(Ref) * L + 8 * num_queries), d_out);
        HIPCHK(hipGetLastError());
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
}

}  // namespace

// The entries of the two families.  Two differences between them are part of the ABI's behaviour and live here, not in the
// templates: for empty input zkp_fri_fold and zkp_fri_merkle_tree answer ZKP_OK before the device is entered, their _fr
// counterparts after it (without a GPU: ZKP_E_DEVICE); and zkp_fri_fold takes its challenge by value.
extern "C" {

size_t zkp_fri_merkle_node_count(size_t n) { return merkle_node_count(n); }
void zkp_free(void* p) { std::free(p); }

int zkp_fri_layer_eval(const uint64_t* coeffs, size_t d, uint64_t coset, unsigned log_D, uint64_t* out) try {
    return fri_layer_eval_t<FriGlTraits>(coeffs, d, &coset, log_D, out);
} ZKP_CATCH_INT
int zkp_fri_layer_eval_fr(const uint64_t* coeffs, size_t d, const uint64_t coset[4], unsigned log_D, uint64_t* out) try {
    return fri_layer_eval_t<FriFrTraits>(coeffs, d, coset, log_D, out);
} ZKP_CATCH_INT

int zkp_fri_fold(const uint64_t* coeffs, size_t d, uint64_t r, uint64_t* out) try {
    if (d && (!coeffs || !out)) return fail(ZKP_E_ARG, "null argument");
    if (!d) return ZKP_OK;
    CTX_ENTER(-1);
    return fri_fold_t<FriGlTraits>(coeffs, d, &r, out);
} ZKP_CATCH_INT
int zkp_fri_fold_fr(const uint64_t* coeffs, size_t d, const uint64_t r[4], uint64_t* out) try {
    if (!r || (d && (!coeffs || !out))) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(-1);
    if (!d) return ZKP_OK;
    return fri_fold_t<FriFrTraits>(coeffs, d, r, out);
} ZKP_CATCH_INT

int zkp_fri_merkle_tree_dev(const void* d_leaves, size_t n, void* d_nodes, void* stream) try {
    return fri_merkle_tree_on_dev_t<FriGlTraits>(d_leaves, n, d_nodes, stream);
} ZKP_CATCH_INT
int zkp_fri_merkle_tree_fr_dev(const void* d_leaves, size_t n, void* d_nodes, void* stream) try {
    return fri_merkle_tree_on_dev_t<FriFrTraits>(d_leaves, n, d_nodes, stream);
} ZKP_CATCH_INT

int zkp_fri_merkle_tree(const uint64_t* leaves, size_t n, uint64_t* nodes_out) try {
    if (n && (!leaves || !nodes_out)) return fail(ZKP_E_ARG, "null argument");
    if (!n) return ZKP_OK;
    CTX_ENTER(-1);
    return fri_merkle_tree_t<FriGlTraits>(leaves, n, nodes_out);
} ZKP_CATCH_INT
int zkp_fri_merkle_tree_fr(const uint64_t* leaves, size_t n, uint64_t* nodes_out) try {
    if (n && (!leaves || !nodes_out)) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    return fri_merkle_tree_t<FriFrTraits>(leaves, n, nodes_out);
} ZKP_CATCH_INT

int zkp_fri_challenges(const uint64_t* roots, size_t layers, uint64_t const_val, size_t num_queries, uint64_t* r_out,
                       uint64_t* q_out) try {
    return fri_challenges_t<FriGlTraits>(roots, layers, &const_val, num_queries, r_out, q_out);
} ZKP_CATCH_INT
int zkp_fri_challenges_fr(const uint64_t* roots, size_t layers, const uint64_t const_val[4], size_t num_queries, uint64_t* r_out,
                          uint64_t* q_out) try {
    return fri_challenges_t<FriFrTraits>(roots, layers, const_val, num_queries, r_out, q_out);
} ZKP_CATCH_INT

int zkp_fri_prove(const uint64_t* coeffs, size_t d, size_t blowup, size_t num_queries, uint64_t** out_proof, size_t* out_words) try {
    return fri_prove_t<FriGlTraits>(coeffs, d, blowup, num_queries, out_proof, out_words);
} ZKP_CATCH_INT
int zkp_fri_prove_fr(const uint64_t* coeffs, size_t d, size_t blowup, size_t num_queries, uint64_t** out_proof,
                     size_t* out_words) try {
    return fri_prove_t<FriFrTraits>(coeffs, d, blowup, num_queries, out_proof, out_words);
} ZKP_CATCH_INT

// fri/src/verifier.rs:10-127.  ZKP_OK = accepted; ZKP_E_ARG with the reference's error string otherwise.
int zkp_fri_verify(const uint64_t* proof, size_t words) try {
    return fri_verify_t<FriGlTraits>(proof, words);
} ZKP_CATCH_INT
int zkp_fri_verify_fr(const uint64_t* proof, size_t words) try {
    return fri_verify_t<FriFrTraits>(proof, words);
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
    transcript_feed_g1(t->gen, xy, is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_plonk_transcript_challenges(zkp_plonk_transcript* t, size_t n, uint64_t* out) try {
    if (!t || (n && !out)) return fail(ZKP_E_ARG, "null argument");
    if (!t->gen.generate(n, out)) return fail(ZKP_E_ARG, "I'm hungry! Feed me something first");
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
