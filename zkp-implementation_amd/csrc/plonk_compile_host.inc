// plonk_compile_host.inc -- Circuit::compile (plonk/src/circuit.rs:166-245) on the device and witness rebinding (included after
// plonk_host.inc, whose prover it fills).
//
// The reference pads the gate list with dummy gates, collects nine assignment vectors and three permutation vectors and
// interpolates the twelve.  Here the gate table is uploaded once, one kernel writes the twelve evaluation columns
// (plonk_gate_cols_kernel), and one batched inverse transform leaves the coefficients in the prover's `circ`.  The columns are kept:
// they are the domain evaluations round 2 would otherwise recompute (dom_evals), and the gate equations are checked on them.
// A new witness for the same circuit rewrites the columns f_a f_b f_c (and pi) only: selectors, wiring, their coset evaluations and
// every allocation stay.

namespace {

// Rows of the witness in dom_evals that violate their gate equation -> gate_rows_bad; everything on `st` is done on return
int gate_check_now(zkp_plonk_prover* p, hipStream_t st) {
    const uint64_t n = p->n;
    HIPCHK(hipMemsetAsync(p->d_len, 0, 8, st));
    hipLaunchKernelGGL(plonk_gate_check_kernel, dim3((unsigned)((n + PK_THREADS - 1) / PK_THREADS)), dim3(PK_THREADS), 0, st,
                       p->dom_evals, n, p->d_len);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(p->h_pin + 16, p->d_len, 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    p->gate_rows_bad = (int)std::min<uint64_t>(p->h_pin[16], 1u << 30);
    return ZKP_OK;
}

int launch_gate_cols(const GateColsParams& gp, hipStream_t st) {
    hipLaunchKernelGGL(plonk_gate_cols_kernel, dim3((unsigned)((gp.n + PK_THREADS - 1) / PK_THREADS)), dim3(PK_THREADS), 0, st, gp);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

// The witness columns of dom_evals from g x 3 values (and g public inputs, nullable) resident on the device, their interpolation into
// `circ`, the public input's slot among the fixed coset evaluations, the gate check; the proof state goes back to "nothing has run"
int rebind_witness(zkp_plonk_prover* p, const Fr* d_vals, const Fr* d_pi, hipStream_t st) {
    const uint64_t n = p->n, D = p->D;
    // until the new check has come back the prover has no checked witness: a failure below must not leave the old verdict standing
    p->gate_rows_bad = -1;
    p->perm_closes = false;
    p->pi_e = HFr::zero();
    p->stage = 0;
    GateColsParams gp;
    std::memset(&gp, 0, sizeof gp);
    gp.vals = d_vals;
    gp.pi = d_pi;
    gp.pi_stride = 1;
    gp.g = p->gates;
    gp.n = n;
    gp.cols = p->dom_evals;
    ZCHK(launch_gate_cols(gp, st));
    const int first = d_pi ? C_PI : C_FA;  // pi f_a f_b f_c are neighbours in circuit order
    ZCHK(run_ntt<Fr>(p->dom_evals + (uint64_t)first * n, p->circuit(first), p->log_n, (size_t)(C_FC + 1 - first), 1, nullptr, st));
    if (d_pi && p->fixed_evals_ready) {  // slot 9 of round 3's inputs: pi on the quotient coset
        const HFr g = HFr::from_u64(7);
        Fr* slot = p->ev + (uint64_t)(4 + C_PI) * D;
        HIPCHK(hipMemsetAsync(slot, 0, 32 * D, st));
        HIPCHK(hipMemcpyAsync(slot, p->circuit(C_PI), 32 * n, hipMemcpyDeviceToDevice, st));
        ZCHK(run_ntt<Fr>(slot, p->log_D, 1, 0, g.l, st));
    }
    return gate_check_now(p, st);
}

int check_rebind_args(const zkp_plonk_prover* p, const void* vals, size_t gates) {
    if (!p || !vals) return fail(ZKP_E_ARG, "null argument");
    if (!p->gates)
        return fail(ZKP_E_ARG, "this prover was made from coefficient vectors (zkp_plonk_prover_create): it has no gate table to bind "
                               "a witness to -- use zkp_plonk_prover_create_from_gates");
    if (gates != p->gates)
        return fail(ZKP_E_ARG, "gate count " + std::to_string(gates) + " differs from the " + std::to_string(p->gates) +
                                   " gates the prover was created from");
    return ZKP_OK;
}

}  // namespace

extern "C" {

int zkp_plonk_prover_create_from_gates(const zkp_bases* srs, const zkp_plonk_gates* gates, zkp_plonk_prover** out) try {
    if (!srs || !gates || !out) return fail(ZKP_E_ARG, "null argument");
    const uint64_t g = gates->gates;
    if (g < 2)
        return fail(ZKP_E_ARG, "a circuit needs at least 2 gates: pad_circuit takes (len - 1).ilog2() (circuit.rs:151), which underflows "
                               "for 0 gates and is ilog2(0) for 1");
    unsigned log_n = 1;
    while (log_n < 64 && (g - 1) >> log_n) log_n++;  // (g - 1).ilog2() + 1
    if (log_n > 24) return fail(ZKP_E_ARG, "log_n > 24");
    if (!gates->pos || !gates->sel || !gates->vals) return fail(ZKP_E_ARG, "null argument");
    {   // an SRS handle exists only where a device slot does: without one `srs` cannot be read
        std::lock_guard<std::mutex> lk(g_rt.mu);
        if (g_rt.slots.empty()) return fail(ZKP_E_DEVICE, "no device slot exists (zkp_init): the SRS handle cannot be a live one");
    }
    if (!srs->shards.empty()) return fail(ZKP_E_ARG, kShardedSrsMsg);
    const uint64_t n = 1ull << log_n;
    for (uint64_t i = 0; i < g; i++)
        for (int j = 0; j < 3; j++) {
            const uint32_t col = gates->pos[6 * i + 2 * j], row = gates->pos[6 * i + 2 * j + 1];
            if (col > 2 || row >= n)
                return fail(ZKP_E_ARG, "Invalid position: gate " + std::to_string(i) + " wire " + "abc"[j] + " = Pos(" + std::to_string(col) +
                                           ", " + std::to_string(row) + "), col must be below 3 and row below n = " + std::to_string(n) +
                                           " (circuit.rs:216-222)");
        }
    CTX_ENTER(srs->slot);
    hipStream_t st = nullptr;
    WsOrder ord(st);
    std::unique_ptr<zkp_plonk_prover> p;
    ZCHK(prover_alloc(srs, log_n, HFr::from_u64(2), HFr::from_u64(3), p));  // k1 = w^0 + 1, k2 = k1 + 1 (find_cosets, circuit.rs:238-245)
    p->gates = g;
    ZCHK(p->dom_evals.ensure(32 * 12 * n));
    // w^e = hi[e >> h] lo[e & (2^h - 1)]
    const unsigned h = (log_n + 1) / 2;
    const uint64_t n_lo = 1ull << h, n_hi = n >> h;
    std::vector<uint64_t> tab(4 * (n_lo + n_hi));
    {
        const HFr w = fr_root_of_unity(log_n);
        HFr cur = HFr::one();
        for (uint64_t j = 0; j < n_lo; j++) {
            cur.store(&tab[4 * j]);
            cur = cur * w;
        }
        const HFr step = cur;  // w^(2^h)
        cur = HFr::one();
        for (uint64_t j = 0; j < n_hi; j++) {
            cur.store(&tab[4 * (n_lo + j)]);
            cur = cur * step;
        }
    }
    // staging, none of it in use before the first proof: the gate table in ev (312 g bytes of 1920 n), the power tables in t
    // (n_lo + n_hi <= n + 1 elements of at least 4n)
    Fr* d_sel = p->ev;
    Fr* d_vals = d_sel + 6 * g;
    uint32_t* d_pos = reinterpret_cast<uint32_t*>(d_vals + 3 * g);
    Fr* d_tab = p->t;
    HIPCHK(hipMemcpyAsync(d_sel, gates->sel, 32 * 6 * g, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_vals, gates->vals, 32 * 3 * g, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_pos, gates->pos, 4 * 6 * g, hipMemcpyHostToDevice, st));
    HIPCHK(hipMemcpyAsync(d_tab, tab.data(), 8 * tab.size(), hipMemcpyHostToDevice, st));
    GateColsParams gp;
    std::memset(&gp, 0, sizeof gp);
    gp.pos = d_pos;
    gp.sel = d_sel;
    gp.vals = d_vals;
    gp.pi = d_sel + 5;
    gp.pi_stride = 6;
    gp.w_lo = d_tab;
    gp.w_hi = d_tab + n_lo;
    gp.h = h;
    gp.g = g;
    gp.n = n;
    gp.cols = p->dom_evals;
    int rc = launch_gate_cols(gp, st);
    if (rc == ZKP_OK) rc = run_ntt<Fr>(p->dom_evals, p->circ, log_n, 12, 1, nullptr, st);  // the 12 interpolations (circuit.rs:173-176, 230-232)
    if (rc == ZKP_OK) rc = gate_check_now(p.get(), st);
    if (rc != ZKP_OK) {
        (void)hipStreamSynchronize(st);  // before the prover's buffers and `tab` go
        return rc;
    }
    *out = p.release();
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_plonk_prover_set_witness(zkp_plonk_prover* p, const uint64_t* vals, const uint64_t* pi, size_t gates) try {
    ZCHK(check_rebind_args(p, vals, gates));
    CTX_ENTER(p->srs->slot);
    hipStream_t st = nullptr;
    WsOrder ord(st);
    HIPCHK(hipStreamSynchronize(p->side));
    // staging in the first three slots of ev, scratch between proofs (rounds 2 and 5): 128 g bytes of 384 n
    const uint64_t g = p->gates;
    Fr* d_vals = p->ev;
    Fr* d_pi = pi ? d_vals + 3 * g : nullptr;
    HIPCHK(hipMemcpyAsync(d_vals, vals, 32 * 3 * g, hipMemcpyHostToDevice, st));
    if (pi) HIPCHK(hipMemcpyAsync(d_pi, pi, 32 * g, hipMemcpyHostToDevice, st));
    const int rc = rebind_witness(p, d_vals, d_pi, st);
    if (rc != ZKP_OK) (void)hipStreamSynchronize(st);  // the caller's arrays are no longer read
    return rc;
} ZKP_CATCH_INT

int zkp_plonk_prover_set_witness_dev(zkp_plonk_prover* p, const void* d_vals, const void* d_pi, size_t gates, void* stream) try {
    ZCHK(check_rebind_args(p, d_vals, gates));
    if (((uintptr_t)d_vals | (uintptr_t)d_pi) & 15) return fail(ZKP_E_ARG, "device pointers must be 16-byte aligned");
    CTX_ENTER(p->srs->slot);
    hipStream_t st = (hipStream_t)stream;
    WsOrder ord(st);
    HIPCHK(hipStreamSynchronize(p->side));
    const int rc = rebind_witness(p, static_cast<const Fr*>(d_vals), static_cast<const Fr*>(d_pi), st);
    if (rc != ZKP_OK) (void)hipStreamSynchronize(st);
    return rc;
} ZKP_CATCH_INT

int zkp_plonk_get_circuit_poly(zkp_plonk_prover* p, int which, uint64_t* out, size_t cap_elems, size_t* len) try {
    if (!p || !len) return fail(ZKP_E_ARG, "null argument");
    if (which < 0 || which > 11) return fail(ZKP_E_ARG, "unknown circuit polynomial id");
    CTX_ENTER(p->srs->slot);
    WsOrder ord(nullptr);
    *len = (size_t)p->n;
    const size_t m = std::min<size_t>(cap_elems, (size_t)p->n);
    if (m && out) HIPCHK(hipMemcpy(out, p->circuit(which), 32 * m, hipMemcpyDeviceToHost));
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_plonk_prover_info(const zkp_plonk_prover* p, unsigned* log_n, uint64_t k1[4], uint64_t k2[4]) try {
    if (!p) return fail(ZKP_E_ARG, "null argument");
    if (log_n) *log_n = p->log_n;
    if (k1) p->k1.store(k1);
    if (k2) p->k2.store(k2);
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
