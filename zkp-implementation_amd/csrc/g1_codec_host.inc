// g1_codec_host.inc -- zkp_g1_decompress*, zkp_g1_compress*, zkp_g1_bases_create_compressed, zkp_fr_from_bytes_dev and
// zkp_fr_to_bytes_dev (included at the end of api.hip, after g1_check_host.inc whose launch and upload sizes these entries share).  The
// format and the kernels are in g1_codec.hpp.  A point that does not decode is a finding, not an error: the decompress entries return
// ZKP_OK with the report filled; only zkp_g1_bases_create_compressed refuses, because it would have to keep the point.

namespace {

const G1DecodeReport kEmptyDecodeReport = {{0, 0, 0, 0}, ~0ull};
const FrDecodeReport kEmptyFrReport = {0, ~0ull};
const char* const kG1DecodeWord[5] = {"valid", "canonical", "curve", "subgroup", "encoding"};
static_assert(sizeof(G1DecodeReport) <= G1_CHECK_HEAD && sizeof(FrDecodeReport) <= G1_CHECK_HEAD, "the report sits in the staging buffer's head");

unsigned codec_blocks(size_t n) { return (unsigned)((n + MSM_THREADS - 1) / MSM_THREADS); }

// `n` points from device memory in launches of at most G1_CHECK_LAUNCH (as g1_check_launch); `first` = the index the report gives point 0
int g1_decode_launch(bool subgroup, const void* d_bytes, size_t n, uint64_t first, void* d_xy, uint8_t* d_inf, uint8_t* d_status,
                     G1DecodeReport* rep, hipStream_t st) {
    for (size_t off = 0; off < n; off += G1_CHECK_LAUNCH) {
        const size_t cnt = std::min(G1_CHECK_LAUNCH, n - off);
        uint4* xy = reinterpret_cast<uint4*>(static_cast<char*>(d_xy) + 96 * off);
        uint8_t* status = d_status ? d_status + off : nullptr;
        hipLaunchKernelGGL(g1_decode_kernel, dim3(codec_blocks(cnt)), dim3(MSM_THREADS), 0, st,
                           reinterpret_cast<const uint4*>(static_cast<const char*>(d_bytes) + 48 * off), (uint64_t)cnt, first + off, xy,
                           d_inf + off, status, rep);
        HIPCHK(hipGetLastError());
        if (!subgroup) continue;  // the flag chooses the launches, no lane looks at it
        hipLaunchKernelGGL(g1_decode_subgroup_kernel, dim3(codec_blocks(cnt)), dim3(MSM_THREADS), 0, st, xy, d_inf + off, (uint64_t)cnt,
                           first + off, status, rep);
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

int g1_encode_launch(const void* d_xy, const uint8_t* d_inf, size_t n, void* d_bytes, hipStream_t st) {
    for (size_t off = 0; off < n; off += G1_CHECK_LAUNCH) {
        const size_t cnt = std::min(G1_CHECK_LAUNCH, n - off);
        hipLaunchKernelGGL(g1_encode_kernel, dim3(codec_blocks(cnt)), dim3(MSM_THREADS), 0, st,
                           reinterpret_cast<const uint4*>(static_cast<const char*>(d_xy) + 96 * off), d_inf ? d_inf + off : nullptr, (uint64_t)cnt,
                           reinterpret_cast<uint4*>(static_cast<char*>(d_bytes) + 48 * off));
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
}

void g1_decode_fill(const G1DecodeReport& r, size_t n, zkp_g1_decoding* out) {
    out->checked = n;
    out->non_canonical = r.count[0];
    out->off_curve = r.count[1];
    out->outside_subgroup = r.count[2];
    out->malformed = r.count[3];
    out->bad = r.count[0] + r.count[1] + r.count[2] + r.count[3];
    out->first_bad = r.first == ~0ull ? n : r.first >> 3;
    out->first_status = r.first == ~0ull ? 0 : (int)(r.first & 7);
}

// n points from HOST memory on the current slot, uploaded in pieces of G1_CHECK_CHUNK through the staging buffer; indices in the report
// are global.  With d_keep_xy / d_keep_inf the decoded points stay on the device (n x 96 and n bytes); otherwise each piece is decoded
// into the staging buffer.  out_xy, out_inf and status, where given, are host memory.  Returns with the stream drained.
int g1_decode_host(const uint8_t* bytes, size_t n, bool subgroup, char* d_keep_xy, uint8_t* d_keep_inf, uint64_t* out_xy, uint8_t* out_inf,
                   uint8_t* status, hipStream_t st, G1DecodeReport* r) {
    const size_t chunk = std::min(n, G1_CHECK_CHUNK);
    ZCHK(ctx().tmp.ensure(G1_CHECK_HEAD + (48 + 96 + 2) * chunk));
    G1DecodeReport* rep = reinterpret_cast<G1DecodeReport*>(ctx().tmp.p);
    HIPCHK(hipMemcpyAsync(rep, &kEmptyDecodeReport, sizeof kEmptyDecodeReport, hipMemcpyHostToDevice, st));
    char* d_bytes = reinterpret_cast<char*>(ctx().tmp.p) + G1_CHECK_HEAD;
    char* d_tmp_xy = d_bytes + 48 * chunk;
    uint8_t* d_tmp_inf = reinterpret_cast<uint8_t*>(d_tmp_xy + 96 * chunk);
    uint8_t* d_status = d_tmp_inf + chunk;
    for (size_t off = 0; off < n; off += chunk) {  // (stream order: the next upload waits for the kernel that reads this one)
        const size_t cnt = std::min(chunk, n - off);
        char* d_xy = d_keep_xy ? d_keep_xy + 96 * off : d_tmp_xy;
        uint8_t* d_inf = d_keep_inf ? d_keep_inf + off : d_tmp_inf;
        HIPCHK(hipMemcpyAsync(d_bytes, bytes + 48 * off, 48 * cnt, hipMemcpyHostToDevice, st));
        ZCHK(g1_decode_launch(subgroup, d_bytes, cnt, off, d_xy, d_inf, status ? d_status : nullptr, rep, st));
        if (out_xy) HIPCHK(hipMemcpyAsync(out_xy + 12 * off, d_xy, 96 * cnt, hipMemcpyDeviceToHost, st));
        if (out_inf) HIPCHK(hipMemcpyAsync(out_inf + off, d_inf, cnt, hipMemcpyDeviceToHost, st));
        if (status) HIPCHK(hipMemcpyAsync(status + off, d_status, cnt, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipMemcpyAsync(r, rep, sizeof *r, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    return ZKP_OK;
}

int decode_flags(unsigned flags) {
    return flags & ~ZKP_G1_DECODE_SUBGROUP ? fail(ZKP_E_ARG, "unknown flag bits (ZKP_G1_DECODE_SUBGROUP is the only one)") : ZKP_OK;
}
bool misaligned16(const void* a, const void* b = nullptr) { return (((uintptr_t)a | (uintptr_t)b) & 15) != 0; }

// The decoded points of a compressed SRS, resident on the calling thread's slot; a bad point is refused here with the report filled
int decode_for_bases(const uint8_t* bytes, size_t n, unsigned flags, zkp_g1_decoding* report, DevBuf* d_xy, TypedBuf<uint8_t>* d_inf) {
    CTX_ENTER(-1);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    ZCHK(d_xy->ensure(96 * n));
    ZCHK(d_inf->ensure(n));
    G1DecodeReport r;
    ZCHK(g1_decode_host(bytes, n, (flags & ZKP_G1_DECODE_SUBGROUP) != 0, static_cast<char*>(d_xy->p), d_inf->get(), nullptr, nullptr, nullptr, st, &r));
    zkp_g1_decoding rep;
    g1_decode_fill(r, n, &rep);
    if (report) *report = rep;
    if (rep.bad)
        return fail(ZKP_E_ARG, "point " + std::to_string(rep.first_bad) + " of the compressed SRS does not decode (" +
                                   kG1DecodeWord[rep.first_status] + "); " + std::to_string(rep.bad) + " bad of " + std::to_string(n));
    return ZKP_OK;
}

}  // namespace

extern "C" {

int zkp_g1_decompress_dev(const void* d_bytes, size_t n, unsigned flags, void* d_out_xy, uint8_t* d_out_is_inf, uint8_t* d_status, void* stream,
                          zkp_g1_decoding* out) try {
    if (!out || (n && (!d_bytes || !d_out_xy || !d_out_is_inf))) return fail(ZKP_E_ARG, "null argument");
    ZCHK(decode_flags(flags));
    *out = zkp_g1_decoding{};
    if (!n) return ZKP_OK;
    if (misaligned16(d_bytes, d_out_xy)) return fail(ZKP_E_ARG, "device pointers must be 16-byte aligned");
    int slot = -1;
    ZCHK(slot_of_device_pointer(d_bytes, &slot));
    CTX_ENTER(slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    ZCHK(ctx().tmp.ensure(G1_CHECK_HEAD));
    G1DecodeReport* rep = reinterpret_cast<G1DecodeReport*>(ctx().tmp.p);
    G1DecodeReport r;
    HIPCHK(hipMemcpyAsync(rep, &kEmptyDecodeReport, sizeof kEmptyDecodeReport, hipMemcpyHostToDevice, st));
    ZCHK(g1_decode_launch((flags & ZKP_G1_DECODE_SUBGROUP) != 0, d_bytes, n, 0, d_out_xy, d_out_is_inf, d_status, rep, st));
    HIPCHK(hipMemcpyAsync(&r, rep, sizeof r, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    g1_decode_fill(r, n, out);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_decompress(const uint8_t* bytes, size_t n, unsigned flags, uint64_t* out_xy, uint8_t* out_is_inf, uint8_t* status,
                      zkp_g1_decoding* out) try {
    if (!out || (n && (!bytes || !out_xy || !out_is_inf))) return fail(ZKP_E_ARG, "null argument");
    ZCHK(decode_flags(flags));
    *out = zkp_g1_decoding{};
    if (!n) return ZKP_OK;
    CTX_ENTER(-1);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    G1DecodeReport r;
    ZCHK(g1_decode_host(bytes, n, (flags & ZKP_G1_DECODE_SUBGROUP) != 0, nullptr, nullptr, out_xy, out_is_inf, status, st, &r));
    g1_decode_fill(r, n, out);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_compress_dev(const void* d_xy, const uint8_t* d_is_inf, size_t n, void* d_out_bytes, void* stream) try {
    if (n && (!d_xy || !d_out_bytes)) return fail(ZKP_E_ARG, "null argument");
    if (!n) return ZKP_OK;
    if (misaligned16(d_xy, d_out_bytes)) return fail(ZKP_E_ARG, "device pointers must be 16-byte aligned");
    int slot = -1;
    ZCHK(slot_of_device_pointer(d_xy, &slot));
    CTX_ENTER(slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return g1_encode_launch(d_xy, d_is_inf, n, d_out_bytes, st);
} ZKP_CATCH_INT

int zkp_g1_compress(const uint64_t* xy, const uint8_t* is_inf, size_t n, uint8_t* out_bytes) try {
    if (n && (!xy || !out_bytes)) return fail(ZKP_E_ARG, "null argument");
    if (!n) return ZKP_OK;
    CTX_ENTER(-1);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    const size_t chunk = std::min(n, G1_CHECK_CHUNK), inf_room = (chunk + 15) & ~(size_t)15;
    ZCHK(ctx().tmp.ensure(96 * chunk + inf_room + 48 * chunk));
    char* d_xy = reinterpret_cast<char*>(ctx().tmp.p);
    uint8_t* d_inf = reinterpret_cast<uint8_t*>(d_xy + 96 * chunk);
    char* d_bytes = d_xy + 96 * chunk + inf_room;
    for (size_t off = 0; off < n; off += chunk) {
        const size_t cnt = std::min(chunk, n - off);
        HIPCHK(hipMemcpyAsync(d_xy, xy + 12 * off, 96 * cnt, hipMemcpyHostToDevice, st));
        if (is_inf) HIPCHK(hipMemcpyAsync(d_inf, is_inf + off, cnt, hipMemcpyHostToDevice, st));
        ZCHK(g1_encode_launch(d_xy, is_inf ? d_inf : nullptr, cnt, d_bytes, st));
        HIPCHK(hipMemcpyAsync(out_bytes + 48 * off, d_bytes, 48 * cnt, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_bases_create_compressed(const uint8_t* bytes, size_t n, unsigned flags, zkp_g1_decoding* report, zkp_bases** out) try {
    if (!out || (n && !bytes)) return fail(ZKP_E_ARG, "null argument");
    ZCHK(decode_flags(flags));
    if (report) *report = zkp_g1_decoding{};
    if (!n) return zkp_g1_bases_create_dev(nullptr, nullptr, 0, nullptr, out);
    DevBuf d_xy;
    TypedBuf<uint8_t> d_inf;
    ZCHK(decode_for_bases(bytes, n, flags, report, &d_xy, &d_inf));  // (drained; its context is left again)
    return zkp_g1_bases_create_dev(d_xy.p, d_inf.get(), n, nullptr, out);
} ZKP_CATCH_INT

int zkp_fr_from_bytes_dev(const void* d_bytes, size_t n, int big_endian, void* d_out, void* stream, uint64_t* bad, uint64_t* first_bad) try {
    if (!bad || (n && (!d_bytes || !d_out))) return fail(ZKP_E_ARG, "null argument");
    *bad = 0;
    if (first_bad) *first_bad = n;
    if (!n) return ZKP_OK;
    if (misaligned16(d_bytes, d_out)) return fail(ZKP_E_ARG, "device pointers must be 16-byte aligned");
    int slot = -1;
    ZCHK(slot_of_device_pointer(d_bytes, &slot));
    CTX_ENTER(slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    ZCHK(ctx().tmp.ensure(G1_CHECK_HEAD));
    FrDecodeReport* rep = reinterpret_cast<FrDecodeReport*>(ctx().tmp.p);
    FrDecodeReport r;
    HIPCHK(hipMemcpyAsync(rep, &kEmptyFrReport, sizeof kEmptyFrReport, hipMemcpyHostToDevice, st));
    for (size_t off = 0; off < n; off += G1_CHECK_LAUNCH) {
        const size_t cnt = std::min(G1_CHECK_LAUNCH, n - off);
        hipLaunchKernelGGL(fr_from_bytes_kernel, dim3(codec_blocks(cnt)), dim3(MSM_THREADS), 0, st,
                           reinterpret_cast<const uint4*>(static_cast<const char*>(d_bytes) + 32 * off), (uint64_t)cnt, big_endian ? 1u : 0u,
                           reinterpret_cast<uint4*>(static_cast<char*>(d_out) + 32 * off), (uint64_t)off, rep);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipMemcpyAsync(&r, rep, sizeof r, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    *bad = r.bad;
    if (first_bad && r.bad) *first_bad = r.first;
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_fr_to_bytes_dev(const void* d_in, size_t n, int big_endian, void* d_out_bytes, void* stream) try {
    if (n && (!d_in || !d_out_bytes)) return fail(ZKP_E_ARG, "null argument");
    if (!n) return ZKP_OK;
    if (misaligned16(d_in, d_out_bytes)) return fail(ZKP_E_ARG, "device pointers must be 16-byte aligned");
    int slot = -1;
    ZCHK(slot_of_device_pointer(d_in, &slot));
    CTX_ENTER(slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    for (size_t off = 0; off < n; off += G1_CHECK_LAUNCH) {
        const size_t cnt = std::min(G1_CHECK_LAUNCH, n - off);
        hipLaunchKernelGGL(fr_to_bytes_kernel, dim3(codec_blocks(cnt)), dim3(MSM_THREADS), 0, st,
                           reinterpret_cast<const uint4*>(static_cast<const char*>(d_in) + 32 * off), (uint64_t)cnt, big_endian ? 1u : 0u,
                           reinterpret_cast<uint4*>(static_cast<char*>(d_out_bytes) + 32 * off));
        HIPCHK(hipGetLastError());
    }
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"
