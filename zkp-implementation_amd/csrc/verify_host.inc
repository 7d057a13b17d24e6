// verify_host.inc -- the verifiers of the reference with real pairings (included at the end of api.hip, after
// plonk_host.inc): KzgScheme::verify / batch_verify (kzg/src/scheme.rs:143-160, 215-245) and plonk verify
// (plonk/src/verifier.rs:19-157).  Host code (pairing_host.hpp); only the eight circuit commitments and pi(zeta) of the
// PLONK verifier use the GPU (they are MSMs / an evaluation over the circuit polynomials).

namespace {

HXyzz g1_generator_host() {
    static const uint64_t gx[6] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL,
                                   0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL};
    static const uint64_t gy[6] = {0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL,
                                   0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    return HXyzz{HFq::load(gx).to_mont(), HFq::load(gy).to_mont(), HFq::one(), HFq::one()};
}
HXyzz g1_scale(const HXyzz& p, const HFr& k) { return p.mul(k.from_mont().l); }
HXyzz g1_load(const uint64_t xy[12], uint8_t inf) { return HXyzz::from_affine(xy, inf != 0); }

// The C ABI is the deserialisation boundary of the verifiers: in the reference every G1 value is a typed `G1Affine` that
// arkworks validated when it was built; here the caller hands over raw limbs.  A finite point is accepted only if both
// coordinates are canonical residues (< p), it satisfies y^2 = x^3 + 4 and it lies in the prime-order subgroup ([r]P = O;
// the curve's cofactor is not 1) -- otherwise the Miller loop would run on an invalid-curve / small-subgroup point.
int g1_validate(const uint64_t xy[12], uint8_t inf, const char* what) {
    if (inf) return ZKP_OK;
    const Mont<6>& m = HFq::M();
    if (Mont<6>::ge(xy, m.p) || Mont<6>::ge(xy + 6, m.p))
        return fail(ZKP_E_ARG, std::string(what) + ": G1 coordinate is not a canonical residue (limbs >= p)");
    const HFq x = HFq::load(xy), y = HFq::load(xy + 6);
    if (y.sqr() != x.sqr() * x + HFq::from_u64(4))
        return fail(ZKP_E_ARG, std::string(what) + ": G1 point is not on the curve y^2 = x^3 + 4");
    if (!HXyzz::from_affine(xy, false).mul(FrTag::ctx().p).is_inf())
        return fail(ZKP_E_ARG, std::string(what) + ": G1 point is not in the prime-order subgroup");
    return ZKP_OK;
}

// The same for G2 (the [s]_2 of an SRS, any caller-supplied G2 point): four canonical Fq limbs vectors, y^2 = x^3 + 4(1 + u), and
// [r]Q = O -- the twist's cofactor is ~2^381, so "on the curve" alone says nothing about the subgroup the pairing is defined on.
int g2_validate(const uint64_t xy[24], const char* what, G2Aff* out) {
    const Mont<6>& m = HFq::M();
    for (int c = 0; c < 4; c++)
        if (Mont<6>::ge(xy + 6 * c, m.p))
            return fail(ZKP_E_ARG, std::string(what) + ": G2 coordinate is not a canonical residue (limbs >= p)");
    const G2Aff q = G2Aff::load(xy, false);
    if (!q.on_curve()) return fail(ZKP_E_ARG, std::string(what) + ": G2 point is not on the curve");
    if (!q.mul(FrTag::ctx().p).inf) return fail(ZKP_E_ARG, std::string(what) + ": G2 point is not in the prime-order subgroup");
    *out = q;
    return ZKP_OK;
}

// FE(f) == 1, the question every check ends in.  By default through the tower the device kernels use (pairing_tower.hpp over HFq):
// E(f) = f^(3 (p^12 - 1) / r) by the x-chain, and E(f) == 1 iff FE(f) == 1 because gcd(3, r) = 1.  ZKP_PAIRING_FINAL_EXP=plain keeps
// the one (p^12 - 1) / r power (~19 ms on the host, what used to dominate a check); zkp_pairing always uses that one, its VALUE is pinned.
std::atomic<uint64_t> g_final_exp_runs[2];  // [0] the x-chain, [1] the plain power: what zkp_selftest_final_exp_counts reports
bool final_exp_is_one(const Fq12& f) {
    const bool plain = knob_is(KNOB_PAIRING_FINAL_EXP, "plain");
    g_final_exp_runs[plain ? 1 : 0].fetch_add(1, std::memory_order_relaxed);
    if (plain) return final_exponentiation(f) == Fq12::one();
    uint64_t w[72];
    f.store(w);
    return tower::f12_is_one(tower::final_exp(tower::f12_load(w)));
}

// e(p1, q1) == e(p2, q2)  <=>  FE(ml(p1, q1) * ml(-p2, q2)) == 1: two Miller loops share ONE final exponentiation
bool pairings_equal(const HXyzz& p1, const G2Aff& q1, const HXyzz& p2, const G2Aff& q2) {
    uint64_t a[12], b[12];
    uint8_t ai = 0, bi = 0;
    p1.to_affine(a, &ai);
    p2.negate().to_affine(b, &bi);
    const Fq12 f = miller_loop(ai ? HFq::zero() : HFq::load(a), ai ? HFq::zero() : HFq::load(a + 6), ai != 0, q1) *
                   miller_loop(bi ? HFq::zero() : HFq::load(b), bi ? HFq::zero() : HFq::load(b + 6), bi != 0, q2);
    return final_exp_is_one(f);
}

}  // namespace

extern "C" {

int zkp_selftest_final_exp_counts(uint64_t out[2]) try {
    if (!out) return fail(ZKP_E_ARG, "null argument");
    for (int i = 0; i < 2; i++) out[i] = g_final_exp_runs[i].load(std::memory_order_relaxed);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g2_generator(uint64_t out_xy[24]) try {
    if (!out_xy) return fail(ZKP_E_ARG, "null argument");
    uint8_t inf = 0;
    G2Aff::generator().store(out_xy, &inf);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g2_mul(const uint64_t q_xy[24], uint8_t q_is_inf, const uint64_t scalar[4], uint64_t out_xy[24], uint8_t* out_is_inf) try {
    if ((!q_is_inf && !q_xy) || !scalar || !out_xy || !out_is_inf) return fail(ZKP_E_ARG, "null argument");
    G2Aff q = G2Aff::infinity();
    if (!q_is_inf) ZCHK(g2_validate(q_xy, "G2 point", &q));
    q.mul(HFr::load(scalar).from_mont().l).store(out_xy, out_is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_pairing(const uint64_t p_xy[12], uint8_t p_is_inf, const uint64_t q_xy[24], uint8_t q_is_inf, uint64_t out_fq12[72]) try {
    if ((!p_is_inf && !p_xy) || (!q_is_inf && !q_xy) || !out_fq12) return fail(ZKP_E_ARG, "null argument");
    G2Aff q = G2Aff::infinity();
    if (!q_is_inf) ZCHK(g2_validate(q_xy, "G2 point", &q));
    if (!p_is_inf) ZCHK(g1_validate(p_xy, 0, "G1 point"));
    pairing(p_xy, p_is_inf != 0, q).store(out_fq12);
    return ZKP_OK;
} ZKP_CATCH_INT

// KzgScheme::verify, kzg/src/scheme.rs:143-160:  e(W, [s]_2 - z G_2) == e(C - y G_1, G_2)
int zkp_kzg_verify(const uint64_t g2s_xy[24], const uint64_t commit_xy[12], uint8_t commit_is_inf, const uint64_t w_xy[12],
                   uint8_t w_is_inf, const uint64_t y[4], const uint64_t z[4], int* accepted) try {
    if (!g2s_xy || (!commit_is_inf && !commit_xy) || (!w_is_inf && !w_xy) || !y || !z || !accepted)
        return fail(ZKP_E_ARG, "null argument");
    const G2Aff g2 = G2Aff::generator();
    G2Aff g2s = G2Aff::infinity();
    ZCHK(g2_validate(g2s_xy, "[s]_2", &g2s));
    ZCHK(g1_validate(commit_xy, commit_is_inf, "commitment"));
    ZCHK(g1_validate(w_xy, w_is_inf, "opening"));
    const G2Aff a = g2s.add(g2.mul(HFr::load(z).from_mont().l).neg());
    const HXyzz b = g1_load(commit_xy, commit_is_inf).add(g1_scale(g1_generator_host(), HFr::load(y)).negate());
    *accepted = pairings_equal(g1_load(w_xy, w_is_inf), a, b, g2) ? 1 : 0;
    return ZKP_OK;
} ZKP_CATCH_INT

// KzgScheme::batch_verify, kzg/src/scheme.rs:215-245; r_primes[i] replaces Fr::from(rng.gen::<u128>()) (the caller's rng)
int zkp_kzg_batch_verify(const uint64_t g2s_xy[24], size_t n, const uint64_t* commits_xy, const uint8_t* commits_is_inf,
                         const uint64_t* points, const uint64_t* openings_xy, const uint8_t* openings_is_inf,
                         const uint64_t* evals, const uint64_t* r_primes, int* accepted) try {
    if (!g2s_xy || !accepted || (n && (!commits_xy || !points || !openings_xy || !evals || !r_primes)))
        return fail(ZKP_E_ARG, "null argument");
    const G2Aff g2 = G2Aff::generator();
    G2Aff g2s = G2Aff::infinity();
    ZCHK(g2_validate(g2s_xy, "[s]_2", &g2s));
    const HXyzz g1 = g1_generator_host();
    HXyzz e1 = HXyzz::infinity(), e2 = HXyzz::infinity();
    for (size_t i = 0; i < n; i++) {
        ZCHK(g1_validate(commits_xy + 12 * i, commits_is_inf ? commits_is_inf[i] : 0, "commitment"));
        ZCHK(g1_validate(openings_xy + 12 * i, openings_is_inf ? openings_is_inf[i] : 0, "opening"));
    }
    for (size_t i = 0; i < n; i++) {
        const HXyzz cm = g1_load(commits_xy + 12 * i, commits_is_inf ? commits_is_inf[i] : 0);
        const HXyzz w = g1_load(openings_xy + 12 * i, openings_is_inf ? openings_is_inf[i] : 0);
        const HFr z = HFr::load(points + 4 * i), s = HFr::load(evals + 4 * i), rp = HFr::load(r_primes + 4 * i);
        const HXyzz cm_minus_s = cm.add(g1_scale(g1, s).negate());
        e1 = e1.add(g1_scale(cm_minus_s.add(g1_scale(w, z)), rp));  // scheme.rs:233-237
        e2 = e2.add(g1_scale(w, rp));                               // scheme.rs:240
    }
    *accepted = pairings_equal(e1, g2, e2, g2s) ? 1 : 0;            // scheme.rs:244
    return ZKP_OK;
} ZKP_CATCH_INT

// KzgScheme::aggregate_commitments, kzg/src/scheme.rs:187-202: sum_i challenge^i * C_i (a handful of points: host)
int zkp_kzg_aggregate_commitments(const uint64_t* commits_xy, const uint8_t* commits_is_inf, size_t n, const uint64_t challenge[4],
                                  uint64_t out_xy[12], uint8_t* out_is_inf) try {
    if (!challenge || !out_xy || !out_is_inf || (n && !commits_xy)) return fail(ZKP_E_ARG, "null argument");
    for (size_t i = 0; i < n; i++) ZCHK(g1_validate(commits_xy + 12 * i, commits_is_inf ? commits_is_inf[i] : 0, "commitment"));
    const HFr ch = HFr::load(challenge);
    HFr pw = HFr::one();
    HXyzz acc = HXyzz::infinity();
    for (size_t i = 0; i < n; i++) {
        acc = acc.add(g1_scale(g1_load(commits_xy + 12 * i, commits_is_inf ? commits_is_inf[i] : 0), pw));
        pw = pw * ch;
    }
    acc.to_affine(out_xy, out_is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

// verify, plonk/src/verifier.rs:19-157.  `p` carries the CompiledCircuit (device polynomials) and the G1 SRS; g2s = [s]_2.
// *accepted: 1 accepted, 0 "Pairing failed, rejected", -1 "Challenge verification failed" (u mismatch, verifier.rs:36-38).
int zkp_plonk_verify(zkp_plonk_prover* p, const uint64_t g2s_xy[24], const zkp_plonk_proof* proof, int* accepted) try {
    if (!p || !g2s_xy || !proof || !accepted) return fail(ZKP_E_ARG, "null argument");
    const G2Aff g2 = G2Aff::generator();
    G2Aff g2s = G2Aff::infinity();
    ZCHK(g2_validate(g2s_xy, "[s]_2", &g2s));
    static const char* const names[9] = {"a", "b", "c", "z", "t_lo", "t_mid", "t_hi", "w_ev_x", "w_ev_wx"};
    for (int i = 0; i < 9; i++) ZCHK(g1_validate(proof->commit_xy[i], proof->commit_is_inf[i], names[i]));
    if (p->para_table.empty()) ZCHK(build_para_table(p));
    const uint64_t n = p->n;
    // get_circuit_commitment (verifier.rs:160-186): q_m q_l q_r q_o q_c s1 s2 s3 in one pass through the MSM kernels
    uint64_t cc_xy[8 * 12];
    uint8_t cc_inf[8];
    HFr pi_e;
    {
        CTX_ENTER(p->srs->slot);
        WsOrder ord(nullptr);
        const Fr* polys8[8] = {p->circuit(C_QM), p->circuit(C_QL), p->circuit(C_QR), p->circuit(C_QO),
                               p->circuit(C_QC), p->circuit(C_S1), p->circuit(C_S2), p->circuit(C_S3)};
        ZCHK(commit_batch_dev(p, polys8, 8, n, nullptr, cc_xy, cc_inf));
    }
    // verify_challenges (verifier.rs:188-220)
    PlonkChallengeGenerator ch;
    auto feed_xy = [&](const uint64_t* xy, uint8_t inf) {
        uint64_t x[6] = {0}, y[6] = {0};
        if (!inf) {
            const HFq cx = HFq::load(xy).from_mont(), cy = HFq::load(xy + 6).from_mont();
            std::memcpy(x, cx.l, 48);
            std::memcpy(y, cy.l, 48);
        }
        ch.feed(x, y, inf != 0);
    };
    auto feed = [&](int i) { feed_xy(proof->commit_xy[i], proof->commit_is_inf[i]); };
    uint64_t c2[8], c1[4];
    feed(0); feed(1); feed(2);
    ch.generate(2, c2);
    const HFr beta = HFr::load(c2), gamma = HFr::load(c2 + 4);
    feed(3);
    ch.generate(1, c1);
    const HFr alpha = HFr::load(c1);
    feed(4); feed(5); feed(6);
    ch.generate(1, c1);
    const HFr zeta = HFr::load(c1);
    HFr bar[6];
    for (int i = 0; i < 6; i++) {
        bar[i] = HFr::load(proof->bars[i]);
        uint64_t xy[12];
        uint8_t inf = 0;
        commit_para(p, bar[i], xy, &inf);
        feed_xy(xy, inf);
    }
    ch.generate(1, c1);
    const HFr v = HFr::load(c1);
    feed(7); feed(8);
    ch.generate(1, c1);
    const HFr u = HFr::load(c1);
    if (!(u == HFr::load(proof->u))) {
        *accepted = -1;
        return ZKP_OK;
    }
    {
        CTX_ENTER(p->srs->slot);
        WsOrder ord(nullptr);
        ZCHK(eval_dev(p->scratch(), p->circuit(C_PI), n, zeta, nullptr, &pi_e));
    }
    const HFr one = HFr::one(), w = fr_root_of_unity(p->log_n);
    const HFr z_h_e = zeta.pow_u64(n) - one;                                  // verifier.rs:43
    const HFr l_1_e = z_h_e * (HFr::from_u64(n) * (zeta - one)).inverse();    // :44-45
    const HFr &ba = bar[0], &bb = bar[1], &bc = bar[2], &bs1 = bar[3], &bs2 = bar[4], &bzw = bar[5];
    const HFr r_0 = pi_e - l_1_e * alpha * alpha - alpha * (ba + bs1 * beta + gamma) * (bb + bs2 * beta + gamma) * (bc + gamma) * bzw;
    auto C = [&](int i) { return g1_load(cc_xy + 12 * i, cc_inf[i]); };        // 0 q_m 1 q_l 2 q_r 3 q_o 4 q_c 5 s1 6 s2 7 s3
    auto PC = [&](int i) { return g1_load(proof->commit_xy[i], proof->commit_is_inf[i]); };
    const HXyzz d1 = g1_scale(C(0), ba * bb).add(g1_scale(C(1), ba)).add(g1_scale(C(2), bb)).add(g1_scale(C(3), bc)).add(C(4));
    const HXyzz d2 = g1_scale(PC(3), (ba + beta * zeta + gamma) * (bb + beta * p->k1 * zeta + gamma) * (bc + beta * p->k2 * zeta + gamma) * alpha +
                                         l_1_e * alpha * alpha + u);
    const HXyzz d3 = g1_scale(C(7), (ba + beta * bs1 + gamma) * (bb + beta * bs2 + gamma) * alpha * beta * bzw);
    const HXyzz d4 = g1_scale(PC(4).add(g1_scale(PC(5), zeta.pow_u64(proof->degree + 1))).add(g1_scale(PC(6), zeta.pow_u64(proof->degree * 2 + 2))),
                              z_h_e);
    const HXyzz d = d1.add(d2).add(d3.negate()).add(d4.negate());
    const HFr v2 = v * v, v3 = v2 * v, v4 = v3 * v, v5 = v4 * v;
    const HXyzz f = d.add(g1_scale(PC(0), v)).add(g1_scale(PC(1), v2)).add(g1_scale(PC(2), v3)).add(g1_scale(C(5), v4)).add(g1_scale(C(6), v5));
    const HFr e_s = (HFr::zero() - r_0) + v * ba + v2 * bb + v3 * bc + v4 * bs1 + v5 * bs2 + u * bzw;
    uint64_t e_xy[12];
    uint8_t e_inf = 0;
    commit_para(p, e_s, e_xy, &e_inf);
    const HXyzz e = g1_load(e_xy, e_inf);
    const HXyzz left = PC(7).add(g1_scale(PC(8), u));                                                  // verifier.rs:131-134
    const HXyzz right = g1_scale(PC(7), zeta).add(g1_scale(PC(8), u * zeta * w)).add(f).add(e.negate());  // :138-149
    *accepted = pairings_equal(left, g2s, right, g2) ? 1 : 0;
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
