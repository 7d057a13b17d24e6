// g1_check_host.inc -- zkp_g1_validate*, zkp_g1_bases_validate and zkp_srs_check (included at the end of api.hip, after
// verify_host.inc whose g2_validate and pairings_equal the SRS check uses).  The kernels are in g1_check.hpp.  A bad point is a
// finding, not an error: the entries return ZKP_OK with the report filled.

namespace {

constexpr size_t G1_CHECK_LAUNCH = (size_t)1 << 22;  // points per launch: ~0.1 s of kernel at most on a shared device
constexpr size_t G1_CHECK_CHUNK = (size_t)1 << 18;   // points per upload of the host entry: 24 MiB of the slot's staging buffer
constexpr size_t G1_CHECK_HEAD = 64;                 // the report sits at the head of the staging buffer, the data behind it

const G1CheckReport kEmptyReport = {{0, 0, 0}, ~0ull};

// The device-side report of the current slot, reset; the staging buffer holds `payload` more bytes behind it
int g1_check_begin(size_t payload, hipStream_t st, G1CheckReport** rep) {
    ZCHK(ctx().tmp.ensure(G1_CHECK_HEAD + payload));
    *rep = reinterpret_cast<G1CheckReport*>(ctx().tmp.p);
    HIPCHK(hipMemcpyAsync(*rep, &kEmptyReport, sizeof kEmptyReport, hipMemcpyHostToDevice, st));
    return ZKP_OK;
}

// `n` points from device memory in launches of at most G1_CHECK_LAUNCH; `first` = the index the report gives point 0
template <class K>
int g1_check_launch(K kernel, size_t point_bytes, const void* d_pts, const uint8_t* d_inf, size_t n, uint64_t first, uint8_t* d_status,
                    G1CheckReport* rep, hipStream_t st) {
    for (size_t off = 0; off < n; off += G1_CHECK_LAUNCH) {
        const size_t cnt = std::min(G1_CHECK_LAUNCH, n - off);
        hipLaunchKernelGGL(kernel, dim3((unsigned)((cnt + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS), 0, st,
                           reinterpret_cast<const uint4*>(static_cast<const char*>(d_pts) + point_bytes * off), d_inf ? d_inf + off : nullptr,
                           (uint64_t)cnt, first + off, d_status ? d_status + off : nullptr, rep);
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

int g1_check_end(const G1CheckReport* d_rep, hipStream_t st, G1CheckReport* out) {
    HIPCHK(hipMemcpyAsync(out, d_rep, sizeof *out, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZKP_OK;
}

void g1_check_merge(G1CheckReport* into, const G1CheckReport& r) {
    for (int k = 0; k < 3; k++) into->count[k] += r.count[k];
    into->first = std::min(into->first, r.first);
}

void g1_check_fill(const G1CheckReport& r, size_t n, zkp_g1_validation* out) {
    out->checked = n;
    out->non_canonical = r.count[0];
    out->off_curve = r.count[1];
    out->outside_subgroup = r.count[2];
    out->bad = r.count[0] + r.count[1] + r.count[2];
    out->first_bad = r.first == ~0ull ? n : r.first >> 2;
    out->first_status = r.first == ~0ull ? 0 : (int)(r.first & 3);
}

// the points of ONE slot's handle (plane 0 of an expansion is the points themselves); status: host memory or null
int bases_validate_single(const zkp_bases* b, uint8_t* status, uint64_t first, G1CheckReport* out) {
    CTX_ENTER(b->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    *out = kEmptyReport;
    if (!b->n) return ZKP_OK;
    G1CheckReport* rep = nullptr;
    ZCHK(g1_check_begin(status ? b->n : 0, st, &rep));
    uint8_t* d_status = status ? reinterpret_cast<uint8_t*>(ctx().tmp.p) + G1_CHECK_HEAD : nullptr;
    ZCHK(g1_check_launch(g1_validate_internal_kernel, 128, b->d_xy.p, b->d_inf.get(), b->n, first, d_status, rep, st));
    if (status) HIPCHK(hipMemcpyAsync(status, d_status, b->n, hipMemcpyDeviceToHost, st));
    return g1_check_end(rep, st, out);
}

}  // namespace

extern "C" {

int zkp_g1_validate_dev(const void* d_xy, const uint8_t* d_is_inf, size_t n, uint8_t* d_status, void* stream, zkp_g1_validation* out) try {
    if (!out || (n && !d_xy)) return fail(ZKP_E_ARG, "null argument");
    *out = zkp_g1_validation{};
    if (!n) return ZKP_OK;
    int slot = -1;
    ZCHK(slot_of_device_pointer(d_xy, &slot));
    CTX_ENTER(slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    G1CheckReport* rep = nullptr;
    G1CheckReport r;
    ZCHK(g1_check_begin(0, st, &rep));
    ZCHK(g1_check_launch(g1_validate_raw_kernel, 96, d_xy, d_is_inf, n, 0, d_status, rep, st));
    ZCHK(g1_check_end(rep, st, &r));
    g1_check_fill(r, n, out);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_validate(const uint64_t* xy, const uint8_t* is_inf, size_t n, uint8_t* status, zkp_g1_validation* out) try {
    if (!out || (n && !xy)) return fail(ZKP_E_ARG, "null argument");
    *out = zkp_g1_validation{};
    if (!n) return ZKP_OK;
    CTX_ENTER(-1);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t chunk = std::min(n, G1_CHECK_CHUNK);
    G1CheckReport* rep = nullptr;
    G1CheckReport r;
    ZCHK(g1_check_begin(98 * chunk, st, &rep));
    char* d_xy = reinterpret_cast<char*>(ctx().tmp.p) + G1_CHECK_HEAD;
    uint8_t* d_inf = reinterpret_cast<uint8_t*>(d_xy + 96 * chunk);
    uint8_t* d_status = d_inf + chunk;
    for (size_t off = 0; off < n; off += chunk) {  // (stream order: the next upload waits for the kernel that reads this one)
        const size_t cnt = std::min(chunk, n - off);
        HIPCHK(hipMemcpyAsync(d_xy, xy + 12 * off, 96 * cnt, hipMemcpyHostToDevice, st));
        if (is_inf) HIPCHK(hipMemcpyAsync(d_inf, is_inf + off, cnt, hipMemcpyHostToDevice, st));
        ZCHK(g1_check_launch(g1_validate_raw_kernel, 96, d_xy, is_inf ? d_inf : nullptr, cnt, off, status ? d_status : nullptr, rep, st));
        if (status) HIPCHK(hipMemcpyAsync(status + off, d_status, cnt, hipMemcpyDeviceToHost, st));
    }
    ZCHK(g1_check_end(rep, st, &r));
    g1_check_fill(r, n, out);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_bases_validate(const zkp_bases* b, uint8_t* status, zkp_g1_validation* out) try {
    if (!b || !out) return fail(ZKP_E_ARG, "null argument");
    *out = zkp_g1_validation{};
    G1CheckReport total = kEmptyReport;
    if (b->shards.empty()) {
        ZCHK(bases_validate_single(b, status, 0, &total));
    } else {  // every chunk on its own device, indices offset by the chunk's place in the handle
        std::vector<G1CheckReport> part(b->shards.size(), kEmptyReport);
        ZCHK(for_each_shard(b, [&](size_t i) {
            return bases_validate_single(b->shards[i].get(), status ? status + b->shard_off[i] : nullptr, b->shard_off[i], &part[i]);
        }));
        for (const G1CheckReport& p : part) g1_check_merge(&total, p);
    }
    if (b->n) g1_check_fill(total, b->n, out);
    return ZKP_OK;
} ZKP_CATCH_INT

// P_0 = G and e(sum r_i P_i, [s]_2) = e(sum r_i P_{i+1}, G_2) over i < n - 1: with random r_i this holds only if P_{i+1} = [s]P_i for
// every i (up to the 2^-128 of a batched check), i.e. P_i = [s^i]G.
int zkp_srs_check(const zkp_bases* srs, const uint64_t g2s_xy[24], size_t n, const uint64_t* r, int* accepted) try {
    if (!srs || !g2s_xy || !accepted || (n > 1 && !r)) return fail(ZKP_E_ARG, "null argument");
    if (!n) return fail(ZKP_E_ARG, "an SRS check needs at least one point");
    if (n > srs->n) return fail(ZKP_E_SIZE, "n is larger than the SRS handle");
    G2Aff g2s = G2Aff::infinity();
    ZCHK(g2_validate(g2s_xy, "[s]_2", &g2s));
    *accepted = 0;
    // P_0 read as the MSM of the one-term scalar vector [1]: KzgScheme::verify multiplies G1Point::generator() (kzg/src/scheme.rs:165),
    // so an SRS scaled by a constant would commit consistently and never verify
    HXyzz p0;
    ZCHK(msm_host_scalars_any(srs, HFr::one().l, 1, &p0));
    if (!p0.add(g1_generator_host().negate()).is_inf()) return ZKP_OK;
    if (n == 1) {
        *accepted = 1;
        return ZKP_OK;
    }
    std::vector<uint64_t> sc(4 * (n + 1), 0);  // [0, r_0 .. r_{n-2}, 0]: the two scalar vectors are its two windows of n
    std::memcpy(&sc[4], r, 32 * (n - 1));
    HXyzz lo, hi;
    ZCHK(msm_host_scalars_any(srs, &sc[4], n, &lo));  // sum r_i P_i
    ZCHK(msm_host_scalars_any(srs, &sc[0], n, &hi));  // sum r_i P_{i+1}
    *accepted = pairings_equal(lo, g2s, hi, G2Aff::generator()) ? 1 : 0;
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
