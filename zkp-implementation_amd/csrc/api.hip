// api.hip -- host side of libzkp_hip.so: the C ABI of include/zkp_hip.h over the gfx950 kernels in
// ntt.hpp / msm.hpp.  No CPU implementation of an MSM or NTT exists here: every compute entry launches HIP
// kernels and fails with ZKP_E_DEVICE when no gfx950 device is usable.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <tuple>
#include <type_traits>
#include <vector>

#include "../../include/zkp_hip.h"
#include "host_ff.hpp"
#include "kzg_host.hpp"
#include "msm.hpp"
#include "g1_check.hpp"
#include "ntt.hpp"
#include "g1_ntt.hpp"
#include "g1_codec.hpp"
#include "kzg_recover.hpp"
#include "kzg_cells.hpp"
#include "kzg_points.hpp"
#include "kzg_points_each.hpp"
#include "kzg_evals.hpp"
#include "plonk.hpp"
#include "nova.hpp"
#include "fri.hpp"
#include "fri_fr.hpp"
#include "selftest.hpp"
#include "pairing.hpp"
#include "transcript_host.hpp"
#include "pairing_host.hpp"
#define ZKP_PAIRING_TOWER_HOST
#include "pairing_tower.hpp"

using namespace zkp;
using namespace zkp::host;

namespace {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// Every int-returning entry is a function-try-block: a C, Go or Rust caller must never see a C++ exception unwind through
// the boundary (include/zkp_hip.h: "never aborts or unwinds").  Host containers and std::thread are the only sources.
int on_exception() noexcept {
    try {
        throw;
    } catch (const std::bad_alloc&) {
        try { g_err = "host allocation failed"; } catch (...) {}
        return ZKP_E_NOMEM;
    } catch (const std::exception& e) {
        try { g_err = std::string("internal error: ") + e.what(); } catch (...) {}
        return ZKP_E_DEVICE;
    } catch (...) {
        try { g_err = "internal error: unknown exception"; } catch (...) {}
        return ZKP_E_DEVICE;
    }
}
#define ZKP_CATCH_INT catch (...) { return on_exception(); }

#define HIPCHK(expr)                                                                                        \
    do {                                                                                                    \
        hipError_t e_ = (expr);                                                                             \
        if (e_ != hipSuccess)                                                                               \
            return fail(e_ == hipErrorOutOfMemory ? ZKP_E_NOMEM : ZKP_E_DEVICE,                             \
                        std::string(#expr) + ": " + hipGetErrorString(e_));                                 \
    } while (0)
// A failed HIP call as HIPCHK reports it (what + the HIP error text; `what` empty where an entry reports the bare text)
int hip_fail(hipError_t e, const std::string& what) {
    return fail(e == hipErrorOutOfMemory ? ZKP_E_NOMEM : ZKP_E_DEVICE, what + hipGetErrorString(e));
}
#define HIPCHK_BARE(expr)                            \
    do {                                             \
        hipError_t e_ = (expr);                      \
        if (e_ != hipSuccess) return hip_fail(e_, ""); \
    } while (0)
#define ZCHK(expr)             \
    do {                       \
        int r_ = (expr);       \
        if (r_ != ZKP_OK) return r_; \
    } while (0)

// The current device's free and total bytes as it reports them now (zeros where it does not), and the ZKP_E_NOMEM that quotes them
struct DevFree {
    size_t free_b = 0, total_b = 0;
    DevFree() {
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) free_b = total_b = 0, (void)hipGetLastError();
    }
    int refuse(const std::string& what, const std::string& tail = "") const {
        return fail(ZKP_E_NOMEM, what + ", " + std::to_string(free_b) + " of " + std::to_string(total_b) + " bytes free on the device" + tail);
    }
};

#include "host_threads.hpp"  // HostPool (host_pool()), Uploader (uploader(slot)), DeviceWorkers, PhaseBarrier
#include "dev_res.hpp"       // DevBuf, TypedBuf, PinnedBuf, Stream, Event
static_assert(ZKP_HOST_THREADS_E_DEVICE == ZKP_E_DEVICE && ZKP_HOST_THREADS_OK == ZKP_OK, "host_threads.hpp error codes");

DeviceWorkers g_workers;  // joined by zkp_shutdown
void device_workers_stop() { g_workers.stop(); }

// Run fn(i) for i < k on the per-slot workers (job i on thread i).  A job reports through its own (code, message) pair: the thread-local
// error string of a worker is not the caller's.  Which failure the caller reports is the caller's rule.
struct SlotResults {
    std::vector<int> rc;
    std::vector<std::string> msg;
};
SlotResults run_on_slots(size_t k, const std::function<int(size_t)>& fn) {
    SlotResults r{std::vector<int>(k, ZKP_OK), std::vector<std::string>(k)};
    std::vector<std::function<void()>> jobs(k);
    for (size_t i = 0; i < k; i++)
        jobs[i] = [&, i] {
            try {
                r.rc[i] = fn(i);
            } catch (...) {
                r.rc[i] = on_exception();
            }
            if (r.rc[i] != ZKP_OK) r.msg[i] = g_err;
        };
    g_workers.run(jobs);
    return r;
}

// ----------------------------------------------------------------------------------------------------
// optional per-phase timing: HIP events on the launch stream (zkp_profile_* in include/zkp_hip.h)
// ----------------------------------------------------------------------------------------------------
struct ProfRec {
    const char* name = nullptr;
    hipEvent_t a = nullptr;  // device phases: start (own_a, or the previous record's end event for a chained scope) and end
    Event own_a, b;
    double host_ms = 0;      // host phases (a == nullptr)
};
std::atomic<int> g_prof_on{0};  // 0 off, 1 every phase, 2 the dominant kernel only (zkp_profile_enable)
struct Ctx;
Ctx& ctx();
std::vector<ProfRec>& prof_records();
hipStream_t& prof_last_stream();

struct ProfScope {
    ProfRec rec;
    hipStream_t st;
    bool on;
    // chain = true: this phase starts where the previous recorded scope on the same stream ended and NOTHING was enqueued in
    // between, so its start is that scope's end event -- one marker per phase boundary instead of two (each marker is a
    // ~5 us bubble on the stream, inside the region bench.py times)
    // name == nullptr: a phase its caller does not record (fri_host.inc: FriGlTraits::phase)
    ProfScope(const char* name, hipStream_t s, bool chain = false) : st(s), on(false) {
        const int level = g_prof_on.load(std::memory_order_relaxed);
        on = name && (level == 1 || (level == 2 && std::strcmp(name, "msm_accumulate") == 0));
        if (!on) return;
        if (level == 2) chain = false;  // the scope before it was not recorded
        rec.name = name;
        std::vector<ProfRec>& recs = prof_records();
        if (chain && !recs.empty() && recs.back().b && prof_last_stream() == s) {
            rec.a = recs.back().b;  // borrowed: the records are released together (zkp_profile_reset, ~Ctx)
            if (rec.b.make(hipEventDefault) != hipSuccess) on = false;
            return;
        }
        if (rec.own_a.make(hipEventDefault) != hipSuccess || rec.b.make(hipEventDefault) != hipSuccess) { on = false; return; }
        rec.a = rec.own_a;
        (void)hipEventRecord(rec.a, st);
    }
    ~ProfScope() {
        if (!on) return;
        (void)hipEventRecord(rec.b, st);
        prof_records().push_back(std::move(rec));
        prof_last_stream() = st;
    }
};
void prof_host(const char* name, double ms) {
    if (g_prof_on.load(std::memory_order_relaxed) != 1) return;
    ProfRec r;
    r.name = name;
    r.host_ms = ms;
    prof_records().push_back(std::move(r));
}

enum { CLK_MSM_ACCUMULATE = 0, CLK_MAD_PROBE = 1, CLK_NTT_FR = 2, CLK_NTT_GL = 3, CLK_COUNT = 4 };
static const char* const kClkNames[CLK_COUNT] = {"msm_accumulate", "mad_probe", "ntt_fr_pass", "ntt_gl_pass"};

#include "ntt_host.inc"  // HostField, NttState, run_ntt, run_ntt_axis0, get_coset_tables: the single-device NTT driver

// One context per device SLOT.  zkp_init(device) makes a single slot; zkp_init_devices() one per listed HIP device (the same
// device may be listed more than once: two slots on one GPU have separate workspaces and streams, which is how a 1-GPU box
// rehearses the multi-device entries).  Every entry runs inside ONE context, chosen by the handle it is given (bases, prover) or by
// the calling thread's zkp_set_device(); the context's mutex serialises the entries of that slot only -- entries on different
// slots run concurrently.
struct Ctx {
    int slot = 0;
    int device = -1;
    std::mutex mu;
    // Members are released in reverse declaration order, after ~Ctx has drained the device: the streams come first so that they
    // outlive every event and buffer that work on them used.
    Stream stream;       // non-blocking; the per-slot workers of the multi-device entries launch on it
    Stream copy_stream;  // zkp_msm_g1: upload of the next scalar range
    Stream sort_stream;  // shared-bucket MSM in several scalar ranges: digits + sort of range r+1 under accumulate r
    Stream xstream;      // ntt_sharded.inc: the peer copies
    // Workspaces and cached tables are shared by every call on this slot, whatever stream the caller passes.  The `*_dev`
    // entries return without synchronising, so a later call on ANOTHER stream must not touch them before the earlier work
    // is done: each entry records ws_event on its stream when it has enqueued everything, and an entry that arrives with a
    // different stream makes it wait for that event first (WsOrder).
    Event ws_event;
    hipStream_t ws_stream = nullptr;
    bool ws_pending = false;
    std::vector<ProfRec> prof;
    hipStream_t prof_last = nullptr;
    // NTT (ntt_host.inc)
    NttState<Fr> ntt_fr;
    NttState<Gl> ntt_gl;
    DevBuf ntt_scratch;
    // MSM
    DevBuf scalars, over;
    TypedBuf<uint32_t> digits, sorted, counts, start, perm, result;
    TypedBuf<uint2> entries;
    TypedBuf<uint4> pieces, buckets, parts, pyr1, odd0, odd1;
    PinnedBuf host_result;
    PinnedBuf fri_small;          // the few dozen words zkp_fri_prove reads back after the folding phase
    DevBuf fb_table;              // fixed-base table (32 x 255 affine points)
    bool fb_ready = false;
    DevBuf g1_ntt_tw;             // twiddle constants of the transform over points (g1_ntt_host.inc), every size and direction
    bool g1_ntt_tw_ready = false;
    DevBuf tmp;                   // staging for host-pointer entry points
    Event copy_event;
    std::vector<Event> copy_events;  // one per scalar range of a host-fed MSM beyond the first (created on demand)
    Event ev_sort[2], ev_acc[2], ev_begin;
    DevBuf fri_arena, fri_meta;   // zkp_fri_prove: layers (evaluations + Merkle nodes) and the gather descriptors
    DevBuf clk;                   // in-kernel clock stamps (ClkRec per instrumented kernel family, msm.hpp), zkp_profile_clock_read
    // in-process multi-GPU transform (ntt_sharded.inc): two exchange buffers of one slab each and the events that order the peer
    // copies of `xstream` (under the transforms of the launch stream) against the other slots
    uint32_t tail_max_waves = 2048;  // co-residency bound of msm_pyramid_tail_kernel on this device (create_slot_locked)
    DevBuf xchg_a, xchg_b;
    std::vector<Event> xev;
    bool peers_enabled = false;
    // Once no entry is inside the slot: finish its work on the device, then let the members go
    ~Ctx() {
        std::lock_guard<std::mutex> lk(mu);
        (void)hipSetDevice(device);
        (void)hipDeviceSynchronize();
    }
};

struct Runtime {
    std::mutex mu;              // guards `slots` (creation / shutdown); never held while a context works
    std::vector<std::unique_ptr<Ctx>> slots;
    bool multi = false;         // zkp_init_devices() with more than one slot
};
Runtime& g_rt = *new Runtime;  // intentionally leaked: no HIP call at process exit (zkp_shutdown releases the slots)

// The record the stamps of kernel family `which` go to while profiling is on (nullptr otherwise: the kernels then execute no stamp)
ClkRec* clk_record(int which) {
    if (!g_prof_on.load(std::memory_order_relaxed)) return nullptr;
    Ctx& c = ctx();
    if (!c.clk.p) {
        if (c.clk.ensure(sizeof(ClkRec) * CLK_COUNT) != ZKP_OK) return nullptr;
        if (hipMemset(c.clk.p, 0, sizeof(ClkRec) * CLK_COUNT) != hipSuccess) return nullptr;
    }
    return reinterpret_cast<ClkRec*>(c.clk.p) + which;
}
thread_local int t_slot = -1;       // zkp_set_device(): the slot of handle-less entries on this thread; -1 = default (slot 0, and
                                    // zkp_g1_bases_create shards over ALL slots)
thread_local Ctx* t_cur = nullptr;  // the context of the entry this thread is inside
Ctx& ctx() { return *t_cur; }
std::vector<ProfRec>& prof_records() { return ctx().prof; }
hipStream_t& prof_last_stream() { return ctx().prof_last; }
template <class F> NttState<F>& ntt_state() { if constexpr (std::is_same<F, Fr>::value) return ctx().ntt_fr; else return ctx().ntt_gl; }
DevBuf& ntt_scratch() { return ctx().ntt_scratch; }

int create_slot_locked(int device);  // below zkp_init

// Resolve the slot of an entry (`slot` < 0: the thread's zkp_set_device() choice, slot 0 by default; no runtime yet: one slot
// on the current HIP device, as zkp_init(-1)), enter its context and make its device current.
struct CtxScope {
    Ctx* prev;
    std::unique_lock<std::mutex> lk;
    int rc = ZKP_OK;
    int restore_device = -1;  // the caller's current HIP device when it differs from the slot's: put back on exit (a caller such as
                              // torch keeps its own idea of the current device)
    explicit CtxScope(int slot) : prev(t_cur) {
        Ctx* c = nullptr;
        {
            std::lock_guard<std::mutex> g(g_rt.mu);
            if (g_rt.slots.empty()) {
                int dev = 0;
                if (hipGetDevice(&dev) != hipSuccess) dev = 0;
                rc = create_slot_locked(dev);
                if (rc != ZKP_OK) return;
            }
            const int s = slot >= 0 ? slot : (t_slot >= 0 ? t_slot : 0);
            if (s >= (int)g_rt.slots.size()) {
                rc = fail(ZKP_E_ARG, "device slot out of range (zkp_init_devices / zkp_set_device)");
                return;
            }
            c = g_rt.slots[(size_t)s].get();
        }
        lk = std::unique_lock<std::mutex>(c->mu);
        t_cur = c;
        int cur = -1;
        if (hipGetDevice(&cur) == hipSuccess && cur != c->device) restore_device = cur;
        if (cur != c->device && hipSetDevice(c->device) != hipSuccess) rc = fail(ZKP_E_DEVICE, "hipSetDevice failed");
    }
    ~CtxScope() {
        t_cur = prev;
        if (restore_device >= 0 && !prev) (void)hipSetDevice(restore_device);  // (a nested scope leaves the outer one's device alone)
    }
};
#define CTX_ENTER(slot)           \
    CtxScope ctx_scope_(slot);    \
    if (ctx_scope_.rc != ZKP_OK) return ctx_scope_.rc

// The stream of a host-pointer entry, after CTX_ENTER: the null stream, or the slot's own once there are several slots
hipStream_t host_stream() { return g_rt.multi ? ctx().stream : nullptr; }

// See Ctx::ws_event.  Constructed by an entry after CTX_ENTER with the stream it is about to launch on.
struct WsOrder {
    hipStream_t st;
    explicit WsOrder(hipStream_t s) : st(s) {
        Ctx& c = ctx();
        if (c.ws_pending && c.ws_stream != st) (void)hipStreamWaitEvent(st, c.ws_event, 0);
    }
    ~WsOrder() {
        Ctx& c = ctx();
        if (c.ws_event.make(hipEventDisableTiming) != hipSuccess) {
            (void)hipStreamSynchronize(st);  // no event to order later callers with: be done before returning
            c.ws_pending = false;
            return;
        }
        (void)hipEventRecord(c.ws_event, st);
        c.ws_stream = st;
        c.ws_pending = true;
    }
};

template <class K>
int allow_big_lds(K kernel) {
    HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                               160 * 1024));
    return ZKP_OK;
}

template <class F>
int ntt_host_entry(uint64_t* data, unsigned log_n, int inverse, const uint64_t* coset) {
    if (!data) return fail(ZKP_E_ARG, "data is null");
    if (log_n > 32) return fail(ZKP_E_ARG, "log_n > 32");
    CTX_ENTER(-1);
    WsOrder ord(nullptr);
    const size_t bytes = sizeof(F) << log_n;
    ZCHK(ctx().tmp.ensure(bytes));
    HIPCHK(hipMemcpyAsync(ctx().tmp.p, data, bytes, hipMemcpyHostToDevice, nullptr));
    ZCHK(run_ntt<F>(reinterpret_cast<F*>(ctx().tmp.p), log_n, 1, inverse, coset, nullptr));
    HIPCHK(hipMemcpyAsync(data, ctx().tmp.p, bytes, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return ZKP_OK;
}

// ----------------------------------------------------------------------------------------------------
// MSM driver
// ----------------------------------------------------------------------------------------------------
}  // namespace

struct zkp_bases {
    DevBuf d_xy;               // n x 128 B: device-internal affine form (28-bit limbs, fq28.hpp / g1_28.hpp)
    TypedBuf<uint8_t> d_inf;   // nullable
    size_t n = 0;
    int device = 0;
    int slot = 0;              // device slot that owns d_xy (Ctx::slot)
    // zkp_init_devices with more than one slot: the handle is a CONTAINER (no d_xy) over per-slot chunk handles,
    // chunk i = points [shard_off[i], shard_off[i] + shards[i]->n) resident on slot shards[i]->slot (contiguous
    // point/scalar chunk per GPU, sharded once at creation)
    std::vector<std::unique_ptr<zkp_bases>> shards;
    std::vector<size_t> shard_off;
    uint32_t pre_c = 0;        // != 0: d_xy holds pre_planes planes of n points, plane s = 2^pre_off[s] * P (shared-bucket MSM);
                               // pre_c = widest slice in bits (2^(pre_c-1) buckets)
    uint32_t pre_planes = 0;
    uint32_t pre_req = 0;      // window_bits the expansion was requested with
    uint16_t pre_off[36] = {0};
    uint32_t pre_glv = 0;      // 1: the planes cover the 129 bits of a scalar half (zkp_g1_bases_precompute_glv): two bucket sets per MSM
};

namespace {

#include "msm_host.inc"  // msm_partial_batch: plan, workspaces, range walk, bucket reduction, host tail

int ensure_fixed_base_table(hipStream_t st) {
    if (ctx().fb_ready) return ZKP_OK;
    // table[w * 255 + (d - 1)] = d * 2^(8 w) * G, affine; built on the host once (8160 points)
    static const uint64_t gx[6] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL,
                                   0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL};
    static const uint64_t gy[6] = {0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL,
                                   0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    HXyzz base{HFq::load(gx).to_mont(), HFq::load(gy).to_mont(), HFq::one(), HFq::one()};
    const int NW = 32, ND = 255;
    std::vector<HXyzz> pts((size_t)NW * ND);
    for (int w = 0; w < NW; w++) {
        pts[(size_t)w * ND] = base;
        for (int d = 1; d < ND; d++) pts[(size_t)w * ND + d] = pts[(size_t)w * ND + d - 1].add(base);
        base = pts[(size_t)w * ND + ND - 1].add(base);
    }
    std::vector<uint64_t> tab(pts.size() * 12);
    std::vector<uint8_t> inf(pts.size());  // (none of these points is the identity)
    batch_to_affine(pts.data(), pts.size(), tab.data(), inf.data());
    ZCHK(ctx().fb_table.ensure(tab.size() * 8));
    HIPCHK(hipMemcpyAsync(ctx().fb_table.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    ctx().fb_ready = true;
    return ZKP_OK;
}

}  // namespace

// ====================================================================================================
// C ABI
// ====================================================================================================
extern "C" {

int zkp_abi_version(void) { return 1; }

void zkp_profile_enable(int on) { g_prof_on.store(on == 2 ? 2 : on != 0 ? 1 : 0); }
void zkp_profile_reset(void) {
    std::lock_guard<std::mutex> g(g_rt.mu);
    for (const auto& c : g_rt.slots) {
        std::lock_guard<std::mutex> lk(c->mu);
        c->prof.clear();
        if (c->clk.p) {
            int prev = 0;
            const bool restore = hipGetDevice(&prev) == hipSuccess && prev != c->device;
            if (restore) (void)hipSetDevice(c->device);
            (void)hipDeviceSynchronize();
            (void)hipMemset(c->clk.p, 0, sizeof(ClkRec) * CLK_COUNT);
            if (restore) (void)hipSetDevice(prev);
        }
    }
}
// In-kernel clock stamps of the instrumented kernel families, summed over the device slots (msm.hpp, ClkRec): the shader clock held
// under that kernel's load is cycles / ref_ticks x 100 MHz.  Synchronises the devices.
struct DeviceRestore {  // the caller keeps its current HIP device, whichever way an entry leaves
    int dev = -1;
    DeviceRestore() { if (hipGetDevice(&dev) != hipSuccess) dev = -1; }
    ~DeviceRestore() { if (dev >= 0) (void)hipSetDevice(dev); }
};
int zkp_profile_clock_read(const char* name, uint64_t* cycles, uint64_t* ref_ticks, uint64_t* waves) try {
    if (!name || !cycles || !ref_ticks || !waves) return fail(ZKP_E_ARG, "null argument");
    int which = -1;
    for (int i = 0; i < CLK_COUNT; i++)
        if (std::strcmp(name, kClkNames[i]) == 0) which = i;
    if (which < 0) return fail(ZKP_E_ARG, "no clock stamps under this name (msm_accumulate, mad_probe, ntt_fr_pass, ntt_gl_pass)");
    std::lock_guard<std::mutex> g(g_rt.mu);
    *cycles = *ref_ticks = *waves = 0;
    DeviceRestore restore;
    for (const auto& c : g_rt.slots) {
        std::lock_guard<std::mutex> lk(c->mu);
        if (!c->clk.p) continue;
        ClkRec r;
        HIPCHK(hipSetDevice(c->device));
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipMemcpy(&r, reinterpret_cast<ClkRec*>(c->clk.p) + which, sizeof r, hipMemcpyDeviceToHost));
        *cycles += r.cycles;
        *ref_ticks += r.ref;
        *waves += r.waves;
    }
    return ZKP_OK;
} ZKP_CATCH_INT

// v_mad_u64_u32 issue rate of this device, now: `launches` back-to-back launches of mad_rate_probe_kernel (8 blocks of 256 lanes per
// CU, ~1 ms each) timed with HIP events on the slot's stream, with the clock its waves saw.  What bench.py divides the multiply-add
// rate of msm_accumulate by, in the same run on the same box (instead of a constant measured once on another one).
int zkp_probe_mad_rate(unsigned launches, double* lane_mads_per_s, double* clock_mhz, double* ms_per_launch) try {
    if (!lane_mads_per_s || !clock_mhz || !ms_per_launch) return fail(ZKP_E_ARG, "null argument");
    if (launches == 0 || launches > 1000) return fail(ZKP_E_ARG, "launches must be in 1..1000");
    CTX_ENTER(-1);
    WsOrder ord(nullptr);
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, ctx().device));
    const unsigned blocks = (unsigned)prop.multiProcessorCount * 8;
    ZCHK(ctx().tmp.ensure((size_t)blocks * 256 * 4 + sizeof(ClkRec)));
    uint32_t* out = reinterpret_cast<uint32_t*>(ctx().tmp.p);
    ClkRec* rec = reinterpret_cast<ClkRec*>(out + (size_t)blocks * 256);
    HIPCHK(hipMemsetAsync(rec, 0, sizeof(ClkRec), nullptr));
    Event e0, e1;
    ZCHK(e0.ensure(hipEventDefault));
    ZCHK(e1.ensure(hipEventDefault));
    hipLaunchKernelGGL(mad_rate_probe_kernel, dim3(blocks), dim3(256), 0, nullptr, out, 7u, (ClkRec*)nullptr);  // warm-up
    HIPCHK(hipEventRecord(e0, nullptr));
    for (unsigned i = 0; i < launches; i++)
        hipLaunchKernelGGL(mad_rate_probe_kernel, dim3(blocks), dim3(256), 0, nullptr, out, 9u + i, rec);
    HIPCHK(hipEventRecord(e1, nullptr));
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventSynchronize(e1));
    float ms = 0;
    HIPCHK(hipEventElapsedTime(&ms, e0, e1));
    ClkRec r;
    HIPCHK(hipMemcpy(&r, rec, sizeof r, hipMemcpyDeviceToHost));
    const double mads = (double)launches * blocks * 256.0 * MAD_PROBE_ITERS * MAD_PROBE_CHAINS;
    *lane_mads_per_s = mads / (ms * 1e-3);
    *clock_mhz = r.ref ? 100.0 * (double)r.cycles / (double)r.ref : 0.0;
    *ms_per_launch = ms / launches;
    return ZKP_OK;
} ZKP_CATCH_INT
// summed over the device slots (one slot unless zkp_init_devices was used)
int zkp_profile_read(const char* name, double* total_ms, uint64_t* count) try {
    if (!name || !total_ms || !count) return fail(ZKP_E_ARG, "null argument");
    std::lock_guard<std::mutex> g(g_rt.mu);
    double tot = 0;
    uint64_t cnt = 0;
    DeviceRestore restore;
    for (const auto& c : g_rt.slots) {
        std::lock_guard<std::mutex> lk(c->mu);
        HIPCHK(hipSetDevice(c->device));
        for (ProfRec& r : c->prof) {
            if (std::strcmp(r.name, name) != 0) continue;
            if (r.a) {
                HIPCHK(hipEventSynchronize(r.b));
                float ms = 0;
                HIPCHK(hipEventElapsedTime(&ms, r.a, r.b));
                tot += ms;
            } else {
                tot += r.host_ms;
            }
            cnt++;
        }
    }
    *total_ms = tot;
    *count = cnt;
    return ZKP_OK;
} ZKP_CATCH_INT
const char* zkp_last_error(void) { return g_err.c_str(); }

}  // extern "C"

namespace {

// A new slot on HIP device `device`; g_rt.mu held by the caller.
int create_slot_locked(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return fail(ZKP_E_DEVICE, "no HIP device visible");
    if (device < 0 || device >= count) return fail(ZKP_E_ARG, "device index out of range");
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(ZKP_E_DEVICE, std::string("device is ") + prop.gcnArchName + ", this library is built for gfx950 only");
    HIPCHK(hipSetDevice(device));
    ZCHK(allow_big_lds((ntt_pass_strided<Fr, NttOps<Fr>::LOG_T>)));
    ZCHK(allow_big_lds((ntt_pass_strided<Fr, NttOps<Fr>::LOG_T - 1>)));
    ZCHK(allow_big_lds((ntt_pass_strided<Fr, NttOps<Fr>::LOG_T - 2>)));
    ZCHK(allow_big_lds((ntt_pass_strided<Gl, NttOps<Gl>::LOG_T>)));
    ZCHK(allow_big_lds(ntt_pass_last<Fr>));
    ZCHK(allow_big_lds(ntt_pass_last<Gl>));
    ZCHK(allow_big_lds(msm_partscatter_kernel<PS_TILE_BIG>));
    ZCHK(allow_big_lds(msm_partscatter_kernel<PS_TILE_MID>));
    ZCHK(allow_big_lds(msm_partscatter_kernel<PS_TILE_SMALL>));
    ZCHK(allow_big_lds(fri_tail_kernel<FriGl>));
    ZCHK(allow_big_lds(fri_tail_kernel<FriFr>));
    auto c = std::make_unique<Ctx>();
    c->device = device;
    c->slot = (int)g_rt.slots.size();
    {   // what the last-levels launch of the bucket reduction may assume resident: two waves per SIMD (four SIMDs per CU), and no
        // more than the kernel's own occupancy (registers, LDS) allows at its default workgroup size
        int per_cu = 0;
        uint32_t cap = (uint32_t)prop.multiProcessorCount * 4 * 2;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, msm_pyramid_tail_kernel, (int)PYR_TAIL_THREADS, 0) == hipSuccess && per_cu > 0)
            cap = std::min<uint32_t>(cap, (uint32_t)per_cu * (uint32_t)prop.multiProcessorCount * (PYR_TAIL_THREADS / 64));
        else
            (void)hipGetLastError();
        c->tail_max_waves = std::max<uint32_t>(cap, 4);
    }
    if (c->stream.make(hipStreamNonBlocking) != hipSuccess) return fail(ZKP_E_DEVICE, "hipStreamCreate failed");
    g_rt.slots.push_back(std::move(c));
    return ZKP_OK;
}

}  // namespace

extern "C" {

int zkp_init(int device) try {
    std::lock_guard<std::mutex> g(g_rt.mu);
    if (!g_rt.slots.empty()) return ZKP_OK;
    if (device < 0 && hipGetDevice(&device) != hipSuccess) device = 0;
    return create_slot_locked(device);
} ZKP_CATCH_INT

int zkp_init_devices(const int* devices, int n_devices) try {
    if (n_devices < 0 || n_devices > 64) return fail(ZKP_E_ARG, "n_devices out of range");
    std::lock_guard<std::mutex> g(g_rt.mu);
    std::vector<int> want;
    if (n_devices == 0 || !devices) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count == 0) return fail(ZKP_E_DEVICE, "no HIP device visible");
        const int n = n_devices ? n_devices : count;
        if (n > count) return fail(ZKP_E_ARG, "more devices requested than visible");
        for (int i = 0; i < n; i++) want.push_back(i);
    } else {
        want.assign(devices, devices + n_devices);
    }
    if (!g_rt.slots.empty()) {  // idempotent for the same list only
        bool same = g_rt.slots.size() == want.size();
        for (size_t i = 0; same && i < want.size(); i++) same = g_rt.slots[i]->device == want[i];
        return same ? ZKP_OK : fail(ZKP_E_ARG, "library already initialised with another device list (zkp_shutdown first)");
    }
    for (int d : want) {
        const int rc = create_slot_locked(d);
        if (rc != ZKP_OK) {
            g_rt.slots.clear();
            return rc;
        }
    }
    g_rt.multi = g_rt.slots.size() > 1;
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_device_count(void) {
    std::lock_guard<std::mutex> g(g_rt.mu);
    return (int)g_rt.slots.size();
}

int zkp_set_device(int slot) try {
    if (slot < -1) return fail(ZKP_E_ARG, "slot must be -1 (default) or a slot index");
    {
        std::lock_guard<std::mutex> g(g_rt.mu);
        if (slot >= 0 && !g_rt.slots.empty() && slot >= (int)g_rt.slots.size()) return fail(ZKP_E_ARG, "device slot out of range");
    }
    t_slot = slot;
    return ZKP_OK;
} ZKP_CATCH_INT

void zkp_shutdown(void) {
    device_workers_stop();
    std::lock_guard<std::mutex> g(g_rt.mu);
    g_rt.slots.clear();
    g_rt.multi = false;
}

// ---- bases -------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

int bases_alloc(size_t n, bool with_inf, zkp_bases** out) {
    std::unique_ptr<zkp_bases> b(new (std::nothrow) zkp_bases());
    if (!b) return fail(ZKP_E_NOMEM, "host allocation failed");
    b->n = n;
    b->device = ctx().device;
    b->slot = ctx().slot;
    HIPCHK_BARE(b->d_xy.grow(std::max<size_t>(128 * n, 128)));
    if (with_inf) HIPCHK_BARE(b->d_inf.grow(std::max<size_t>(n, 1)));
    *out = b.release();
    return ZKP_OK;
}

// contiguous chunk [lo, hi) of n items owned by shard i of k; sizes differ by at most one (zkp_hip/dist.py: shard_range)
void shard_range(size_t n, size_t i, size_t k, size_t* lo, size_t* hi) {
    const size_t base = n / k, rem = n % k;
    *lo = i * base + std::min(i, rem);
    *hi = *lo + base + (i < rem ? 1 : 0);
}

// n points from host memory onto ONE slot
int bases_create_single(int slot, const uint64_t* xy, const uint8_t* is_inf, size_t n, zkp_bases** out) {
    CTX_ENTER(slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    zkp_bases* b = nullptr;
    ZCHK(bases_alloc(n, is_inf != nullptr, &b));
    hipError_t e = hipSuccess;
    if (n) {
        int rc = ctx().tmp.ensure(96 * n);
        if (rc != ZKP_OK) {
            zkp_g1_bases_destroy(b);
            return rc;
        }
        e = hipMemcpyAsync(ctx().tmp.p, xy, 96 * n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(g1_to_internal_kernel, dim3((unsigned)((n + MSM_THREADS - 1) / MSM_THREADS)),
                               dim3(MSM_THREADS), 0, st, reinterpret_cast<const uint4*>(ctx().tmp.p), (uint64_t)n,
                               static_cast<uint4*>(b->d_xy.p));
            e = hipGetLastError();
        }
        if (e == hipSuccess && is_inf) e = hipMemcpyAsync(b->d_inf.p, is_inf, n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (e != hipSuccess) {
        zkp_g1_bases_destroy(b);
        return fail(ZKP_E_DEVICE, hipGetErrorString(e));
    }
    *out = b;
    return ZKP_OK;
}

// Run fn(i) for every chunk of a sharded handle on the per-slot workers; the first failure (code + message) is the caller's.
int for_each_shard(const zkp_bases* b, const std::function<int(size_t)>& fn) {
    const size_t k = b->shards.size();
    const SlotResults r = run_on_slots(k, fn);
    for (size_t i = 0; i < k; i++)
        if (r.rc[i] != ZKP_OK)  // (while a sharded handle is being created its chunk i is slot i and may still be null)
            return fail(r.rc[i], "device slot " + std::to_string(b->shards[i] ? b->shards[i]->slot : (int)i) + ": " + r.msg[i]);
    return ZKP_OK;
}

// Automatic window width of an expansion (0 = leave the bases as they are)
unsigned auto_window_bits(size_t n) {
    if (n < 64) return 0;
    return n >= (1u << 22) ? 22 : n >= (1u << 19) ? 20 : n > (1u << 13) ? 16 : n > (1u << 11) ? 14 : 12;
}

// check_only: stop after the argument and budget checks, before anything is allocated (the sharded entry asks every chunk's device
// first, so that a refusal leaves the whole handle unexpanded instead of a mixture)
// glv: planes for the endomorphism-split MSM (glv.hpp) -- ceil(129 / window_bits) of them instead of ceil(256 / window_bits)
int precompute_single(zkp_bases* b, unsigned window_bits, bool glv, bool check_only = false) {
    if (b->pre_c && (b->pre_glv != 0) != glv)
        return fail(ZKP_E_ARG, b->pre_glv ? "bases already expanded for the endomorphism-split MSM (zkp_g1_bases_precompute_glv)"
                                          : "bases already expanded for whole scalars (zkp_g1_bases_precompute)");
    if (window_bits == 0) {  // automatic
        // Up to 2^18 points the MSM is a chain of latencies, not of throughput: 16-bit windows (16 slices, 2^15 buckets, 14 reduction
        // levels) with the run of a bucket split over 2 or 4 lanes (msm.hpp, split_run) beat the 18..20 bits of round 1, whose 2^17..2^19
        // buckets were needed to fill the lanes and paid for it in the reduction (tools/split_sweep2.sh, one box, single MSM / batch of
        // three): 2^15 0.509 -> 0.463 / 0.870 -> 0.682 ms, 2^16 0.678 -> 0.529 / 1.112 -> 0.933, 2^17 0.922 -> 0.747 / 1.613 -> 1.454,
        // 2^18 1.121 -> 1.053 / 2.836 -> 2.566; 2^19 stays at 20 bits (1.62 ms against 1.80 at 18).  Below 2^13: 14 bits (2^12 0.312
        // against 0.324 ms), below 2^11: 12 bits (2^10 0.278 against 0.319 ms) -- profiles/r02_n_split_runs.md.
        // From 2^22 points 22 bits: 12 slices of 21/22 bits over 2^21 buckets -- one insertion per scalar less, a 4x larger
        // bucket reduction (0.46 -> 1.26 ms): 2^22 9.57 -> 9.10 ms, 2^24 37.5 -> 33.7 ms, 2^26 149.4 -> 132.5 ms
        // (profiles/r02_c_window22.md).
        if (b->pre_c || b->n < 64) return ZKP_OK;
        window_bits = auto_window_bits(b->n);
    }
    if (window_bits < 9 || window_bits > MSM_MAX_WINDOW_BITS) return fail(ZKP_E_ARG, "window_bits must be 0 (automatic) or in 9.." + std::to_string(MSM_MAX_WINDOW_BITS));
    if (b->pre_c) return b->pre_req == window_bits ? ZKP_OK : fail(ZKP_E_ARG, "bases already expanded with another width");
    CTX_ENTER(b->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    if (!b->n) return ZKP_OK;
    // Slices of a scalar (or of a scalar half): msm_slice_offsets, msm_plan.hpp
    const MsmSlices sl = msm_slice_offsets(glv ? GlvParams::COVER_BITS : 256, window_bits, (uint32_t)knob_int(KNOB_MSM_BALANCE_FROM));  // (tuning aid)
    const uint32_t planes = sl.planes, cmax = sl.widest;
    SliceOffsets so;
    static_assert(sizeof so.off == sizeof sl.off, "SliceOffsets");
    std::memcpy(so.off, sl.off, sizeof so.off);
    DevBuf p;
    {   // The expansion is `planes` x the SRS (13 x at 20 bits, 12 x at 22: 103 GB for 2^26 points, and a 2^27 SRS no longer fits one
        // device; split planes: 7 x and 6 x).  Say so with the numbers instead of a bare allocation failure; the handle stays usable unexpanded (per-window MSM).
        const size_t need = 128 * (size_t)planes * b->n;
        const DevFree mem;
        const size_t budget = std::min<size_t>(mem.free_b ? mem.free_b : ~(size_t)0, (size_t)knob_int(KNOB_SRS_EXPAND_MAX_BYTES));
        auto too_large = [&](const char* why) {
            return mem.refuse("SRS expansion does not fit (" + std::string(why) + "): " + std::to_string(planes) + " planes x " +
                                  std::to_string(b->n) + " points x 128 B = " + std::to_string(need) + " bytes",
                              "; the bases stay unexpanded (per-window MSM), or shard the SRS over more devices (zkp_init_devices)");
        };
        if (need > budget) return too_large(need > mem.free_b && mem.free_b ? "device memory" : "ZKP_SRS_EXPAND_MAX_BYTES");
        if (check_only) return ZKP_OK;
        if (p.ensure(need) != ZKP_OK) {
            (void)hipGetLastError();
            return too_large("hipMalloc");
        }
    }
    hipError_t e = hipMemcpyAsync(p.p, b->d_xy.p, 128 * b->n, hipMemcpyDeviceToDevice, st);
    const uint64_t step = std::min<uint64_t>(b->n, 1ull << 18);  // points per launch: bounds the scratch area (ZZ, ZZZ, products)
    if (e == hipSuccess && ctx().tmp.ensure(192 * (size_t)planes * step) != ZKP_OK) e = hipErrorOutOfMemory;
    for (uint64_t off = 0; e == hipSuccess && off < b->n; off += step) {
        const uint64_t cnt = std::min<uint64_t>(step, b->n - off);
        hipLaunchKernelGGL(g1_expand_planes_kernel, dim3((unsigned)((cnt + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS),
                           0, st, static_cast<uint4*>(p.p), reinterpret_cast<uint4*>(ctx().tmp.p), off, cnt,
                           (uint64_t)b->n, planes, so);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? ZKP_E_NOMEM : ZKP_E_DEVICE, std::string("SRS expansion: ") + hipGetErrorString(e));
    b->d_xy = std::move(p);
    b->pre_c = cmax;
    b->pre_req = window_bits;
    b->pre_planes = planes;
    b->pre_glv = glv ? 1u : 0u;
    std::memcpy(b->pre_off, so.off, sizeof so.off);
    return ZKP_OK;
}

// Back to the plain points (plane 0 of an expansion is the points themselves): roll-back of a sharded expansion that failed half way
int unexpand_single(zkp_bases* b) {
    if (!b->pre_c) return ZKP_OK;
    CTX_ENTER(b->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    DevBuf p;
    ZCHK(p.ensure(128 * std::max<size_t>(b->n, 1)));
    hipError_t e = hipMemcpyAsync(p.p, b->d_xy.p, 128 * b->n, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) return fail(ZKP_E_DEVICE, hipGetErrorString(e));
    b->d_xy = std::move(p);
    b->pre_c = b->pre_req = b->pre_planes = b->pre_glv = 0;
    return ZKP_OK;
}

// device memory belongs to one device: an entry that is given a device pointer works on the slot of that device (the thread's
// zkp_set_device() slot when it matches, else the first slot on the pointer's device)
int slot_of_device_pointer(const void* d_ptr, int* slot) {
    *slot = t_slot;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, d_ptr) != hipSuccess) return ZKP_OK;
    std::lock_guard<std::mutex> g(g_rt.mu);
    if (*slot >= 0 && *slot < (int)g_rt.slots.size() && g_rt.slots[(size_t)*slot]->device != attr.device) *slot = -1;
    for (size_t i = 0; *slot < 0 && i < g_rt.slots.size(); i++)
        if (g_rt.slots[i]->device == attr.device) *slot = (int)i;
    if (*slot < 0 && !g_rt.slots.empty()) return fail(ZKP_E_ARG, "device pointer belongs to a device the library was not initialised on");
    return ZKP_OK;
}

}  // namespace

extern "C" {

int zkp_g1_bases_create(const uint64_t* xy, const uint8_t* is_inf, size_t n, zkp_bases** out) try {
    if (!out || (n && !xy)) return fail(ZKP_E_ARG, "null argument");
    size_t nslots = 0;
    {
        std::lock_guard<std::mutex> g(g_rt.mu);
        nslots = g_rt.slots.size();
    }
    if (nslots <= 1 || t_slot >= 0) return bases_create_single(t_slot >= 0 ? t_slot : 0, xy, is_inf, n, out);
    // several device slots and no zkp_set_device() choice on this thread: shard by contiguous chunk, one chunk per slot
    zkp_bases* c = new (std::nothrow) zkp_bases();
    if (!c) return fail(ZKP_E_NOMEM, "host allocation failed");
    c->n = n;
    c->slot = -1;
    c->shards.resize(nslots);
    c->shard_off.assign(nslots, 0);
    for (size_t i = 0; i < nslots; i++) {
        size_t hi = 0;
        shard_range(n, i, nslots, &c->shard_off[i], &hi);
    }
    const int rc = for_each_shard(c, [&](size_t i) {  // (shards[i] is still null here: for_each_shard only reads its slot on failure)
        size_t lo = 0, hi = 0;
        shard_range(n, i, nslots, &lo, &hi);
        zkp_bases* s = nullptr;
        const int r = bases_create_single((int)i, xy + 12 * lo, is_inf ? is_inf + lo : nullptr, hi - lo, &s);
        c->shards[i].reset(s);
        return r;
    });
    if (rc != ZKP_OK) {
        zkp_g1_bases_destroy(c);
        return rc;
    }
    *out = c;
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_bases_create_dev(const void* d_xy, const uint8_t* d_is_inf, size_t n, void* stream, zkp_bases** out) try {
    if (!out || (n && !d_xy)) return fail(ZKP_E_ARG, "null argument");
    int slot = t_slot;
    if (n) ZCHK(slot_of_device_pointer(d_xy, &slot));
    CTX_ENTER(slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    zkp_bases* b = nullptr;
    ZCHK(bases_alloc(n, d_is_inf != nullptr, &b));
    hipError_t e = hipSuccess;
    if (n) {
        hipLaunchKernelGGL(g1_to_internal_kernel, dim3((unsigned)((n + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS),
                           0, st, reinterpret_cast<const uint4*>(d_xy), (uint64_t)n, static_cast<uint4*>(b->d_xy.p));
        e = hipGetLastError();
    }
    if (e == hipSuccess && n && d_is_inf) e = hipMemcpyAsync(b->d_inf.p, d_is_inf, n, hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        zkp_g1_bases_destroy(b);
        return fail(ZKP_E_DEVICE, hipGetErrorString(e));
    }
    *out = b;
    return ZKP_OK;
} ZKP_CATCH_INT

static int precompute_any(zkp_bases* b, unsigned window_bits, bool glv) {
    if (!b) return fail(ZKP_E_ARG, "null argument");
    if (b->shards.empty()) return precompute_single(b, window_bits, glv);
    // A sharded handle is expanded all-or-nothing and every chunk alike (zkp_g1_bases_info reports chunk 0 for all of them): the
    // automatic width comes from the largest chunk, every chunk's device is asked for room BEFORE any of them allocates, and a
    // failure half way rolls the finished chunks back to the plain points.
    size_t nmax = 0, expanded = 0;
    for (const auto& sh : b->shards) nmax = std::max(nmax, sh->n), expanded += sh->pre_c ? 1 : 0;
    for (const auto& sh : b->shards)  // (the other mode: refused before the automatic width can say "nothing to do")
        if (sh->pre_c && (sh->pre_glv != 0) != glv) return precompute_single(sh.get(), window_bits, glv, true);
    if (window_bits == 0) {
        if (expanded == b->shards.size() || !(window_bits = auto_window_bits(nmax))) return ZKP_OK;
        if (expanded) window_bits = b->shards[0]->pre_req ? b->shards[0]->pre_req : window_bits;
    }
    ZCHK(for_each_shard(b, [&](size_t i) { return precompute_single(b->shards[i].get(), window_bits, glv, true); }));
    std::vector<uint8_t> was(b->shards.size());
    for (size_t i = 0; i < b->shards.size(); i++) was[i] = b->shards[i]->pre_c ? 1 : 0;
    const int rc = for_each_shard(b, [&](size_t i) { return precompute_single(b->shards[i].get(), window_bits, glv); });  // every chunk on its own device
    if (rc != ZKP_OK) {
        const std::string why = zkp_last_error();
        bool mixed = false;
        for (size_t i = 0; i < b->shards.size(); i++)
            if (!was[i] && b->shards[i]->pre_c && unexpand_single(b->shards[i].get()) != ZKP_OK) mixed = true;
        return fail(rc, why + (mixed ? " -- and a finished chunk could not be rolled back: the handle is expanded in part (still usable)"
                                     : " -- every chunk is back to the plain points"));
    }
    return ZKP_OK;
}

int zkp_g1_bases_precompute(zkp_bases* b, unsigned window_bits) try { return precompute_any(b, window_bits, false); } ZKP_CATCH_INT

int zkp_g1_bases_precompute_glv(zkp_bases* b, unsigned window_bits) try { return precompute_any(b, window_bits, true); } ZKP_CATCH_INT

int zkp_g1_bases_expansion(const zkp_bases* b, zkp_bases_expansion* out) try {
    if (!b || !out) return fail(ZKP_E_ARG, "null argument");
    const zkp_bases* s = b->shards.empty() ? b : b->shards[0].get();  // every chunk of a sharded handle is expanded alike
    if (!s) return fail(ZKP_E_ARG, "empty handle");
    *out = zkp_bases_expansion{};
    if (!s->pre_c) return ZKP_OK;  // unexpanded: all zero
    out->window_bits = s->pre_req;
    out->planes = s->pre_planes;
    out->glv = s->pre_glv;
    out->slices = s->pre_planes * (s->pre_glv ? 2u : 1u);
    out->widest_slice_bits = s->pre_c;
    if (b->shards.empty()) out->bytes = 128 * (size_t)s->pre_planes * s->n;
    for (const auto& sh : b->shards) out->bytes += sh->pre_c ? 128 * (size_t)sh->pre_planes * sh->n : 0;
    return ZKP_OK;
} ZKP_CATCH_INT

size_t zkp_g1_bases_len(const zkp_bases* b) { return b ? b->n : 0; }

int zkp_g1_bases_info(const zkp_bases* b, unsigned* window_bits, unsigned* slices) try {
    if (!b || !window_bits || !slices) return fail(ZKP_E_ARG, "null argument");
    const zkp_bases* s = b->shards.empty() ? b : b->shards[0].get();  // every chunk of a sharded handle is expanded alike
    if (!s) return fail(ZKP_E_ARG, "empty handle");
    *window_bits = s->pre_req;
    *slices = s->pre_c ? s->pre_planes * (s->pre_glv ? 2u : 1u) : 0;  // insertions per scalar
    return ZKP_OK;
} ZKP_CATCH_INT

void zkp_g1_bases_destroy(zkp_bases* b) {
    if (!b) return;
    for (auto& s : b->shards) zkp_g1_bases_destroy(s.release());
    DeviceRestore restore;
    (void)hipSetDevice(b->device);
    delete b;
}

// ---- MSM ---------------------------------------------------------------------------------------------
}  // extern "C"

namespace {

const char* const kShardedDev = "bases are sharded over several devices: device-pointer entries take single-device bases "
                                "(zkp_set_device + zkp_g1_bases_create*); use zkp_msm_g1 with host scalars";

// sum_{i<n} scalars[i] * bases[i] for host scalars over ONE slot's bases, unnormalised
int msm_host_scalars(const zkp_bases* bases, const uint64_t* scalars, size_t n, HXyzz* r, unsigned bits = MSM_BITS_MAX) {
    CTX_ENTER(bases->slot);
    hipStream_t st = host_stream();
    WsOrder ord(st);
    if (n > bases->n) return fail(ZKP_E_SIZE, "more scalars than bases (kzg/src/scheme.rs:86)");
    *r = HXyzz::infinity();
    if (!n) return ZKP_OK;
    ZCHK(ctx().scalars.ensure(32 * n));
    const Fr* d_sc = reinterpret_cast<const Fr*>(ctx().scalars.p);
    const bool shared = bases->pre_c != 0;
    if (shared && n >= (1u << 19)) {  // pipeline the PCIe upload against the kernels
        ZCHK(ctx().copy_stream.ensure(hipStreamNonBlocking));
        ZCHK(ctx().copy_event.ensure(hipEventDisableTiming));
        const MsmFeed feed{scalars, ctx().copy_stream, ctx().copy_event, msm_feed_ranges(n)};  // (the range policy: msm_plan.hpp)
        return msm_partial_batch(bases, &d_sc, 1, n, st, r, &feed, bits);
    }
    HIPCHK(hipMemcpyAsync(ctx().scalars.p, scalars, 32 * n, hipMemcpyHostToDevice, st));
    return msm_partial(bases, d_sc, n, st, r, bits);
}

// One MSM over the chunks of a sharded handle: body(i, lo, len, &part) runs chunk i's share [lo, lo + len) of the n terms on that
// chunk's worker (for_each_shard); a chunk at or past n and an empty chunk are skipped.  The per-device partial sums (192 B each) come
// back to the host with each device's result anyway, so the exchange of SURVEY 8e is a host-side EC add of `devices` points, in chunk order
int msm_over_shards(const zkp_bases* bases, size_t n, const std::function<int(size_t, size_t, size_t, HXyzz*)>& body, HXyzz* r) {
    std::vector<HXyzz> part(bases->shards.size(), HXyzz::infinity());
    ZCHK(for_each_shard(bases, [&](size_t i) {
        const size_t lo = bases->shard_off[i], have = bases->shards[i]->n;
        if (lo >= n || !have) return (int)ZKP_OK;
        return body(i, lo, std::min(have, n - lo), &part[i]);
    }));
    *r = HXyzz::infinity();
    for (const HXyzz& p : part) *r = r->add(p);
    return ZKP_OK;
}

// msm_host_scalars over a handle that may be sharded: every device takes the scalars of its chunk (uploaded by its own worker thread
// over its own PCIe link) and runs the whole Pippenger on it
int msm_host_scalars_any(const zkp_bases* bases, const uint64_t* scalars, size_t n, HXyzz* r) {
    if (bases->shards.empty()) return msm_host_scalars(bases, scalars, n, r);
    if (n > bases->n) return fail(ZKP_E_SIZE, "more scalars than bases (kzg/src/scheme.rs:86)");
    return msm_over_shards(bases, n, [&](size_t i, size_t lo, size_t len, HXyzz* part) {
        return msm_host_scalars(bases->shards[i].get(), scalars + 4 * lo, len, part);
    }, r);
}

}  // namespace

extern "C" {

int zkp_msm_g1_partial_dev(const zkp_bases* bases, const void* d_scalars, size_t n, void* stream, uint64_t out_xyzz[24]) try {
    if (!bases || !out_xyzz || (n && !d_scalars)) return fail(ZKP_E_ARG, "null argument");
    if (!bases->shards.empty()) return fail(ZKP_E_ARG, kShardedDev);
    CTX_ENTER(bases->slot);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    HXyzz r;
    ZCHK(msm_partial(bases, reinterpret_cast<const Fr*>(d_scalars), n, reinterpret_cast<hipStream_t>(stream), &r));
    r.store(out_xyzz);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_msm_g1_dev(const zkp_bases* bases, const void* d_scalars, size_t n, void* stream, uint64_t out_xy[12],
                   uint8_t* out_is_inf) try {
    if (!bases || !out_xy || !out_is_inf || (n && !d_scalars)) return fail(ZKP_E_ARG, "null argument");
    if (!bases->shards.empty()) return fail(ZKP_E_ARG, kShardedDev);
    CTX_ENTER(bases->slot);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    HXyzz r;
    ZCHK(msm_partial(bases, reinterpret_cast<const Fr*>(d_scalars), n, reinterpret_cast<hipStream_t>(stream), &r));
    r.to_affine(out_xy, out_is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_msm_g1(const zkp_bases* bases, const uint64_t* scalars, size_t n, uint64_t out_xy[12], uint8_t* out_is_inf) try {
    if (!bases || !out_xy || !out_is_inf || (n && !scalars)) return fail(ZKP_E_ARG, "null argument");
    HXyzz r;
    ZCHK(msm_host_scalars_any(bases, scalars, n, &r));
    r.to_affine(out_xy, out_is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

// ---- bounded scalars: every canonical scalar below 2^bits (include/zkp_hip.h).  From 255 bits on these ARE the entries above.
static int check_scalar_bits(const zkp_bases* bases, unsigned bits) {
    if (bits < 1 || bits > MSM_BITS_MAX) return fail(ZKP_E_ARG, "bits must be 1..256");
    if (bases && !bases->shards.empty()) return fail(ZKP_E_ARG, "bases are sharded over several devices: the bounded MSM entries take single-device bases");
    return ZKP_OK;
}

int zkp_msm_g1_bits(const zkp_bases* bases, const uint64_t* scalars, size_t n, unsigned bits, uint64_t out_xy[12], uint8_t* out_is_inf) try {
    ZCHK(check_scalar_bits(bases, bits));
    if (bits >= MSM_BITS_WHOLE) return zkp_msm_g1(bases, scalars, n, out_xy, out_is_inf);
    if (!bases || !out_xy || !out_is_inf || (n && !scalars)) return fail(ZKP_E_ARG, "null argument");
    HXyzz r;
    ZCHK(msm_host_scalars(bases, scalars, n, &r, bits));
    r.to_affine(out_xy, out_is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_msm_g1_bits_dev(const zkp_bases* bases, const void* d_scalars, size_t n, unsigned bits, void* stream, uint64_t out_xy[12],
                        uint8_t* out_is_inf) try {
    ZCHK(check_scalar_bits(bases, bits));
    if (bits >= MSM_BITS_WHOLE) return zkp_msm_g1_dev(bases, d_scalars, n, stream, out_xy, out_is_inf);
    if (!bases || !out_xy || !out_is_inf || (n && !d_scalars)) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(bases->slot);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    HXyzz r;
    ZCHK(msm_partial(bases, reinterpret_cast<const Fr*>(d_scalars), n, reinterpret_cast<hipStream_t>(stream), &r, bits));
    r.to_affine(out_xy, out_is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_msm_g1_batch_bits_dev(const zkp_bases* bases, const void* const* d_scalars, size_t count, size_t n, unsigned bits, void* stream,
                              uint64_t* out_xy, uint8_t* out_is_inf) try {
    ZCHK(check_scalar_bits(bases, bits));
    if (bits >= MSM_BITS_WHOLE) return zkp_msm_g1_batch_dev(bases, d_scalars, count, n, stream, out_xy, out_is_inf);
    if (!bases || (count && (!d_scalars || !out_xy || !out_is_inf))) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(bases->slot);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    std::vector<HXyzz> r(count);
    ZCHK(msm_partial_batch(bases, reinterpret_cast<const Fr* const*>(d_scalars), count, n, reinterpret_cast<hipStream_t>(stream), r.data(),
                           nullptr, bits));
    batch_to_affine(r.data(), count, out_xy, out_is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

// The largest bit length among n resident scalars: the OR of their canonical words (fr_or_words_kernel), read back and measured here
int zkp_fr_bit_length_dev(const void* d_scalars, size_t n, void* stream, unsigned* out_bits) try {
    if (!out_bits || (n && !d_scalars)) return fail(ZKP_E_ARG, "null argument");
    *out_bits = 0;
    if (!n) return ZKP_OK;
    if (reinterpret_cast<uintptr_t>(d_scalars) & 15) return fail(ZKP_E_ARG, "device pointers must be 16-byte aligned");
    int slot = -1;
    ZCHK(slot_of_device_pointer(d_scalars, &slot));
    CTX_ENTER(slot);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    ZCHK(ctx().tmp.ensure(256));
    uint32_t* d_or = reinterpret_cast<uint32_t*>(ctx().tmp.p);
    uint32_t words[8];
    HIPCHK(hipMemsetAsync(d_or, 0, sizeof words, st));
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)n + MSM_THREADS - 1) / MSM_THREADS, FR_OR_MAX_BLOCKS);
    hipLaunchKernelGGL(fr_or_words_kernel, dim3(blocks), dim3(MSM_THREADS), 0, st, reinterpret_cast<const uint4*>(d_scalars), (uint64_t)n, d_or);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(words, d_or, sizeof words, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    for (int q = 7; q >= 0 && !*out_bits; q--)
        if (words[q]) *out_bits = 32u * (unsigned)q + 32u - (unsigned)__builtin_clz(words[q]);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_bases_shard_count(const zkp_bases* b) { return !b ? 0 : b->shards.empty() ? 1 : (int)b->shards.size(); }

int zkp_g1_bases_shard(const zkp_bases* b, size_t i, int* slot, int* device, size_t* offset, size_t* len) try {
    if (!b || !slot || !device || !offset || !len) return fail(ZKP_E_ARG, "null argument");
    if (i >= (size_t)zkp_g1_bases_shard_count(b)) return fail(ZKP_E_ARG, "chunk index out of range");
    const zkp_bases* s = b->shards.empty() ? b : b->shards[i].get();
    *slot = s->slot;
    *device = s->device;
    *offset = b->shards.empty() ? 0 : b->shard_off[i];
    *len = s->n;
    return ZKP_OK;
} ZKP_CATCH_INT

// Ordering of a chunk's launch after the producer of its scalars: the slot's stream (or the legacy null stream of a single-slot
// runtime) does not wait for work on the caller's non-blocking streams by itself.  With an event the wait happens on the device
// (hipStreamWaitEvent, the host does not block); without one the entry waits for the whole device.
static int order_after_producer(hipStream_t st, void* ready_event) {
    if (ready_event) HIPCHK(hipStreamWaitEvent(st, reinterpret_cast<hipEvent_t>(ready_event), 0));
    else HIPCHK(hipDeviceSynchronize());
    return ZKP_OK;
}

int zkp_msm_g1_sharded_dev_after(const zkp_bases* bases, const void* const* d_scalars, void* const* ready_events, size_t n,
                                 uint64_t out_xy[12], uint8_t* out_is_inf) try {
    if (!bases || !out_xy || !out_is_inf || (n && !d_scalars)) return fail(ZKP_E_ARG, "null argument");
    if (n > bases->n) return fail(ZKP_E_SIZE, "more scalars than bases (kzg/src/scheme.rs:86)");
    HXyzz acc = HXyzz::infinity();
    if (bases->shards.empty()) {
        if (n) {
            if (!d_scalars[0]) return fail(ZKP_E_ARG, "null scalar pointer");
            CTX_ENTER(bases->slot);
            hipStream_t st = host_stream();
            // neither the slot's non-blocking stream nor the legacy null stream is ordered after a producer on a non-blocking
            // stream (torch's side streams are): wait for its event, or for the device (include/zkp_hip.h states this contract)
            ZCHK(order_after_producer(st, ready_events ? ready_events[0] : nullptr));
            WsOrder ord(st);
            ZCHK(msm_partial(bases, reinterpret_cast<const Fr*>(d_scalars[0]), n, st, &acc));
        }
    } else {
        for (size_t i = 0; i < bases->shards.size(); i++)
            if (bases->shard_off[i] < n && bases->shards[i]->n && !d_scalars[i]) return fail(ZKP_E_ARG, "null scalar pointer for a chunk in use");
        ZCHK(msm_over_shards(bases, n, [&](size_t i, size_t, size_t len, HXyzz* part) {
            const zkp_bases* sh = bases->shards[i].get();
            CTX_ENTER(sh->slot);
            // d_scalars[i] may come from a copy or kernel still in flight on another stream of this device (a resident tensor made
            // by .to(device) a moment ago): the slot's stream is non-blocking and would not wait for it
            ZCHK(order_after_producer(ctx().stream, ready_events ? ready_events[i] : nullptr));
            WsOrder ord(ctx().stream);
            return msm_partial(sh, reinterpret_cast<const Fr*>(d_scalars[i]), len, ctx().stream, part);
        }, &acc));
    }
    acc.to_affine(out_xy, out_is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_msm_g1_sharded_dev(const zkp_bases* bases, const void* const* d_scalars, size_t n, uint64_t out_xy[12],
                           uint8_t* out_is_inf) {
    return zkp_msm_g1_sharded_dev_after(bases, d_scalars, nullptr, n, out_xy, out_is_inf);
}

int zkp_msm_g1_partial(const zkp_bases* bases, const uint64_t* scalars, size_t n, uint64_t out_xyzz[24]) try {
    if (!bases || !out_xyzz || (n && !scalars)) return fail(ZKP_E_ARG, "null argument");
    HXyzz r;
    ZCHK(msm_host_scalars_any(bases, scalars, n, &r));
    r.store(out_xyzz);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_msm_g1_batch_dev(const zkp_bases* bases, const void* const* d_scalars, size_t count, size_t n, void* stream,
                         uint64_t* out_xy, uint8_t* out_is_inf) try {
    if (!bases || (count && (!d_scalars || !out_xy || !out_is_inf))) return fail(ZKP_E_ARG, "null argument");
    if (!bases->shards.empty()) return fail(ZKP_E_ARG, kShardedDev);
    CTX_ENTER(bases->slot);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    std::vector<HXyzz> r(count);
    ZCHK(msm_partial_batch(bases, reinterpret_cast<const Fr* const*>(d_scalars), count, n, reinterpret_cast<hipStream_t>(stream),
                           r.data()));
    batch_to_affine(r.data(), count, out_xy, out_is_inf);  // one field inversion for the batch: a PLONK proof makes nine commitments in four batches
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_xyzz_sum(const uint64_t* partials, size_t count, uint64_t out_xy[12], uint8_t* out_is_inf) try {
    if ((count && !partials) || !out_xy || !out_is_inf) return fail(ZKP_E_ARG, "null argument");
    HXyzz acc = HXyzz::infinity();
    for (size_t i = 0; i < count; i++) acc = acc.add(HXyzz::load(partials + 24 * i));
    acc.to_affine(out_xy, out_is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_kzg_commit(const zkp_bases* srs, const uint64_t* coeffs, size_t len, uint64_t out_xy[12], uint8_t* out_is_inf) try {
    if (!srs || !out_xy || !out_is_inf || (len && !coeffs)) return fail(ZKP_E_ARG, "null argument");
    KzgScheme scheme(srs);
    KzgCommitment cm;
    int rc = scheme.commit(coeffs, len, &cm);
    if (rc == ZKP_E_SIZE && g_err.empty()) g_err = "SRS shorter than the polynomial (kzg/src/scheme.rs:86)";
    if (rc != ZKP_OK) return rc;
    std::memcpy(out_xy, cm.p.xy, 96);
    *out_is_inf = cm.p.infinity;
    return ZKP_OK;
} ZKP_CATCH_INT

int kzg_open_device(const zkp_bases* srs, const uint64_t* coeffs, size_t len, const uint64_t z[4], uint64_t out_xy[12],
                    uint8_t* out_is_inf, uint64_t out_eval[4]);  // plonk_host.inc

int zkp_kzg_open(const zkp_bases* srs, const uint64_t* coeffs, size_t len, const uint64_t z[4], uint64_t out_xy[12],
                 uint8_t* out_is_inf, uint64_t out_eval[4]) try {
    if (!srs || !out_xy || !out_is_inf || !out_eval || !z || (len && !coeffs)) return fail(ZKP_E_ARG, "null argument");
    if (len == 0) return fail(ZKP_E_ARG, "open of an empty polynomial (kzg/src/scheme.rs:112 expects at least 1)");
    // long polynomials: Horner evaluation and the division by (X - z) run on the GPU too (they are O(n) serial loops in
    // the reference, scheme.rs:110-118, and would dwarf the MSM on the host); short ones use the C++ mirror as is
    if (len >= 4096) return kzg_open_device(srs, coeffs, len, z, out_xy, out_is_inf, out_eval);
    KzgScheme scheme(srs);
    KzgOpening op;
    int rc = scheme.open(coeffs, len, z, &op);
    if (rc != ZKP_OK) return rc;
    std::memcpy(out_xy, op.p.xy, 96);
    *out_is_inf = op.p.infinity;
    op.eval.store(out_eval);
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_g1_mul(const uint64_t base_xy[12], uint8_t base_is_inf, const uint64_t scalar[4], uint64_t out_xy[12],
               uint8_t* out_is_inf) try {
    if (!base_xy || !scalar || !out_xy || !out_is_inf) return fail(ZKP_E_ARG, "null argument");
    HFr k = HFr::load(scalar).from_mont();
    HXyzz r = HXyzz::from_affine(base_xy, base_is_inf != 0).mul(k.l);
    r.to_affine(out_xy, out_is_inf);
    return ZKP_OK;
} ZKP_CATCH_INT

static int fixed_base_mul_locked(const void* d_scalars, size_t n, void* d_out_xy, uint8_t* d_out_is_inf, hipStream_t st) {
    ZCHK(ensure_fixed_base_table(st));
    hipLaunchKernelGGL(g1_fixed_base_kernel, dim3((unsigned)((n + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS), 0,
                       st, reinterpret_cast<const Fr*>(d_scalars), (uint64_t)n,
                       reinterpret_cast<const uint4*>(ctx().fb_table.p), reinterpret_cast<uint4*>(d_out_xy), d_out_is_inf);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
}

int zkp_g1_fixed_base_mul_dev(const void* d_scalars, size_t n, void* d_out_xy, uint8_t* d_out_is_inf, void* stream) try {
    if (n && (!d_scalars || !d_out_xy)) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    return fixed_base_mul_locked(d_scalars, n, d_out_xy, d_out_is_inf, reinterpret_cast<hipStream_t>(stream));
} ZKP_CATCH_INT

int zkp_selftest_fq_inverse_dev(const void* d_in, size_t n, int form, void* d_out, void* stream) try {
    if (n && (!d_in || !d_out)) return fail(ZKP_E_ARG, "null argument");
    if (form != 0 && form != 1) return fail(ZKP_E_ARG, "form must be 0 (12 x u32, radix 2^384) or 1 (14 x 28 bit + 2 pad words, radix 2^392)");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    hipLaunchKernelGGL(fq_inverse_selftest_kernel, dim3((unsigned)((n + MSM_THREADS - 1) / MSM_THREADS)), dim3(MSM_THREADS), 0,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint32_t*>(d_in), reinterpret_cast<uint32_t*>(d_out),
                       (uint64_t)n, form);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

// ---- lane-level self-tests of the field and curve primitives (kernels: csrc/selftest.hip) ----
namespace {
unsigned selftest_grid(size_t lanes) { return (unsigned)((lanes + ST_THREADS - 1) / ST_THREADS); }
int selftest_args(const void* d_in, size_t n, const void* d_out) {
    if (n && (!d_in || !d_out)) return fail(ZKP_E_ARG, "null argument");
    if (d_in && d_in == d_out) return fail(ZKP_E_ARG, "d_out must not be d_in");
    if (n > (size_t)1 << 24) return fail(ZKP_E_SIZE, "a self-test takes at most 2^24 cases");
    return ZKP_OK;
}
}  // namespace

int zkp_selftest_fq28_dev(int op, const void* d_in, size_t n, void* d_out, void* stream) try {
    ZCHK(selftest_args(d_in, n, d_out));
    if (op < 0 || op >= ST_FQ28_OPS) return fail(ZKP_E_ARG, "unknown Fq28 self-test operation");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    selftest_fq28_launch(op, selftest_grid(n), reinterpret_cast<hipStream_t>(stream), d_in, d_out, (uint64_t)n);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_selftest_fr29_dev(int op, const void* d_in, size_t n, void* d_out, void* stream) try {
    ZCHK(selftest_args(d_in, n, d_out));
    if (op < 0 || op >= ST_FR29_OPS) return fail(ZKP_E_ARG, "unknown Fr29 self-test operation");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    selftest_fr29_launch(op, selftest_grid(n), reinterpret_cast<hipStream_t>(stream), d_in, d_out, (uint64_t)n);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_selftest_fp_dev(int field, int op, const void* d_in, size_t n, void* d_out, void* stream) try {
    ZCHK(selftest_args(d_in, n, d_out));
    if (field != 0 && field != 1) return fail(ZKP_E_ARG, "field must be 0 (Fq, 12 words) or 1 (Fr, 8 words)");
    if (op < 0 || op >= ST_FP_OPS) return fail(ZKP_E_ARG, "unknown Fp self-test operation");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    selftest_fp_launch(field, op, selftest_grid(n), reinterpret_cast<hipStream_t>(stream), d_in, d_out, (uint64_t)n);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_selftest_gl_dev(int op, const void* d_in, size_t n, void* d_out, void* stream) try {
    ZCHK(selftest_args(d_in, n, d_out));
    if (op < 0 || op >= ST_GL_OPS) return fail(ZKP_E_ARG, "unknown Goldilocks self-test operation");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    selftest_gl_launch(op, selftest_grid(n), reinterpret_cast<hipStream_t>(stream), d_in, d_out, (uint64_t)n);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_selftest_g1_dev(int op, const void* d_a, const void* d_b, size_t n, size_t stride, void* d_out, void* d_flag, void* stream) try {
    if (op < 0 || op >= ST_G1_OPS) return fail(ZKP_E_ARG, "unknown G1 self-test operation");
    const bool in_place = op == ST_G1_ADD_INPLACE || op == ST_G1_ADD_INPLACE_CHAIN || op == ST_G1_ADD_QUAD_INPLACE;
    const bool planes = op >= ST_G1_ADD_STREAM;
    if (n && ((!d_a && !in_place) || !d_b || !d_out || !d_flag)) return fail(ZKP_E_ARG, "null argument");
    if (d_b && d_b == d_out) return fail(ZKP_E_ARG, "d_out must not be d_b");
    if ((op == ST_G1_ADD_STREAM || op == ST_G1_ADD_STREAM_CHAIN) && d_a == d_out) return fail(ZKP_E_ARG, "the streaming add does not alias: use the in-place operation");
    if (n > (size_t)1 << 24) return fail(ZKP_E_SIZE, "a self-test takes at most 2^24 cases");
    if (planes && stride < n) return fail(ZKP_E_ARG, "stride below the number of cases");
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    const bool quad = op == ST_G1_ADD_QUAD || op == ST_G1_ADD_QUAD_INPLACE;
    selftest_g1_launch(op, selftest_grid(quad ? 4 * n : n), reinterpret_cast<hipStream_t>(stream), d_a, d_b, d_out, d_flag, (uint64_t)n,
                       (uint64_t)stride);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_selftest_glv_split_dev(const void* d_scalars, size_t n, void* d_out, void* stream) try {
    ZCHK(selftest_args(d_scalars, n, d_out));
    CTX_ENTER(-1);
    if (!n) return ZKP_OK;
    selftest_glv_split_launch(selftest_grid(n), reinterpret_cast<hipStream_t>(stream), d_scalars, d_out, (uint64_t)n);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_selftest_msm_sort_dev(const zkp_bases* bases, const void* const* d_scalars, size_t count, size_t n, size_t range_index, void* stream,
                              zkp_msm_sort_geometry* geom, const zkp_msm_sort_outputs* out) try {
    if (!bases || !geom || (count && !d_scalars)) return fail(ZKP_E_ARG, "null argument");
    if (!bases->shards.empty()) return fail(ZKP_E_ARG, kShardedDev);
    for (size_t m = 0; n && m < count && m < (size_t)MSM_MAX_BATCH; m++)
        if (!d_scalars[m]) return fail(ZKP_E_ARG, "null scalar pointer");
    CTX_ENTER(bases->slot);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    return msm_sort_selftest(bases, reinterpret_cast<const Fr* const*>(d_scalars), count, n, range_index, reinterpret_cast<hipStream_t>(stream),
                             geom, out);
} ZKP_CATCH_INT

int zkp_selftest_msm_sort_bits_dev(const zkp_bases* bases, const void* const* d_scalars, size_t count, size_t n, size_t range_index, unsigned bits,
                                   void* stream, zkp_msm_sort_geometry* geom, const zkp_msm_sort_outputs* out) try {
    ZCHK(check_scalar_bits(bases, bits));
    if (bits >= MSM_BITS_WHOLE) return zkp_selftest_msm_sort_dev(bases, d_scalars, count, n, range_index, stream, geom, out);
    if (!bases || !geom || (count && !d_scalars)) return fail(ZKP_E_ARG, "null argument");
    for (size_t m = 0; n && m < count && m < (size_t)MSM_MAX_BATCH; m++)
        if (!d_scalars[m]) return fail(ZKP_E_ARG, "null scalar pointer");
    CTX_ENTER(bases->slot);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    return msm_sort_selftest(bases, reinterpret_cast<const Fr* const*>(d_scalars), count, n, range_index, reinterpret_cast<hipStream_t>(stream),
                             geom, out, bits);
} ZKP_CATCH_INT

int zkp_selftest_msm_reduce_dev(int slot, const zkp_msm_reduce_io* in, void* stream, zkp_msm_reduce_geometry* geom) try {
    if (!in || !geom) return fail(ZKP_E_ARG, "null argument");
    CTX_ENTER(slot);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    return msm_reduce_selftest(*in, reinterpret_cast<hipStream_t>(stream), geom);
} ZKP_CATCH_INT

int zkp_srs_g1(const uint64_t secret[4], size_t n, uint64_t* out_xy) try {
    if (!secret || (n && !out_xy)) return fail(ZKP_E_ARG, "null argument");
    if (!n) return ZKP_OK;
    std::vector<uint64_t> pw(4 * n);
    HFr s = HFr::load(secret), cur = HFr::one();
    for (size_t i = 0; i < n; i++) {  // cur *= secret, kzg/src/srs.rs:58
        cur.store(&pw[4 * i]);
        cur = cur * s;
    }
    CTX_ENTER(-1);
    WsOrder ord(nullptr);
    ZCHK(ctx().tmp.ensure(32 * n + 96 * n));
    char* d = reinterpret_cast<char*>(ctx().tmp.p);
    HIPCHK(hipMemcpy(d, pw.data(), 32 * n, hipMemcpyHostToDevice));
    ZCHK(fixed_base_mul_locked(d, n, d + 32 * n, nullptr, nullptr));
    HIPCHK(hipMemcpy(out_xy, d + 32 * n, 96 * n, hipMemcpyDeviceToHost));
    return ZKP_OK;
} ZKP_CATCH_INT

// ---- NTT ---------------------------------------------------------------------------------------------
}  // extern "C"
bool ntt_should_shard(unsigned log_n);                                                         // ntt_sharded.inc
int ntt_fr_sharded_host(uint64_t* data, unsigned log_n, int inverse, const uint64_t* coset);  // ntt_sharded.inc
extern "C" {
int zkp_ntt_fr(uint64_t* data, unsigned log_n, int inverse, const uint64_t* coset) try {
    // several device slots and a transform worth spreading: the four-step transform over all of them (natural order in and out)
    if (ntt_should_shard(log_n)) return ntt_fr_sharded_host(data, log_n, inverse, coset);
    return ntt_host_entry<Fr>(data, log_n, inverse, coset);
} ZKP_CATCH_INT
int zkp_ntt_goldilocks(uint64_t* data, unsigned log_n, int inverse, const uint64_t* coset) try {
    return ntt_host_entry<Gl>(data, log_n, inverse, coset);
} ZKP_CATCH_INT
int zkp_ntt_fr_dev(void* d_data, unsigned log_n, size_t batch, int inverse, const uint64_t* coset, void* stream) try {
    if (!d_data) return fail(ZKP_E_ARG, "data is null");
    CTX_ENTER(-1);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    return run_ntt<Fr>(reinterpret_cast<Fr*>(d_data), log_n, batch, inverse, coset, reinterpret_cast<hipStream_t>(stream));
} ZKP_CATCH_INT
int zkp_ntt_goldilocks_dev(void* d_data, unsigned log_n, size_t batch, int inverse, const uint64_t* coset, void* stream) try {
    if (!d_data) return fail(ZKP_E_ARG, "data is null");
    CTX_ENTER(-1);
    WsOrder ord(reinterpret_cast<hipStream_t>(stream));
    return run_ntt<Gl>(reinterpret_cast<Gl*>(d_data), log_n, batch, inverse, coset, reinterpret_cast<hipStream_t>(stream));
} ZKP_CATCH_INT

int zkp_ntt_fr_twiddle_dev(void* d_data, size_t rows, size_t cols, size_t row0, unsigned log_n, int inverse, void* stream) try {
    if (!d_data) return fail(ZKP_E_ARG, "data is null");
    if (log_n > 32 || log_n == 0) return fail(ZKP_E_ARG, "log_n out of range");
    if ((uint64_t)(row0 + rows - 1) * (cols - 1) >= (1ull << log_n) && rows && cols)
        return fail(ZKP_E_ARG, "twiddle exponent (row0 + rows - 1) * (cols - 1) must stay below n");
    CTX_ENTER(-1);
    if (!rows || !cols) return ZKP_OK;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    PowTab<Fr> tab;
    HFr w = fr_root_of_unity(log_n);  // get_coset_tables inverts the base itself when inverse != 0
    ZCHK(get_coset_tables<Fr>(log_n, inverse ? 1 : 0, w.l, HFr::one(), &tab, st));
    const uint64_t total = (uint64_t)rows * cols;
    hipLaunchKernelGGL(twiddle_rows_kernel<Fr>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st,
                       reinterpret_cast<Fr*>(d_data), (uint64_t)rows, (uint64_t)cols, (uint64_t)row0, tab);
    HIPCHK(hipGetLastError());
    return ZKP_OK;
} ZKP_CATCH_INT

int zkp_ntt_fr_axis0_dev(const void* d_in, void* d_out, unsigned log_len, size_t cols, int inverse, unsigned tw_log_n,
                         size_t tw_col0, void* stream) try {
    if (!d_in || !d_out) return fail(ZKP_E_ARG, "data is null");
    CTX_ENTER(-1);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    return run_ntt_axis0<Fr>(reinterpret_cast<const Fr*>(d_in), reinterpret_cast<Fr*>(d_out), log_len, cols, inverse, tw_log_n,
                             (uint64_t)tw_col0, st);
} ZKP_CATCH_INT

int zkp_ntt_fr_layout_dev(const void* d_in, void* d_out, unsigned log_n, size_t batch, int inverse, const zkp_ntt_layout* in_layout,
                          const zkp_ntt_layout* out_layout, unsigned tw_log_n, size_t tw_row0, void* stream) try {
    if (!d_in || !d_out) return fail(ZKP_E_ARG, "data is null");
    if (log_n > 32) return fail(ZKP_E_ARG, "log_n > 32");
    NttRemap rin, rout;
    const zkp_ntt_layout* ls[2] = {in_layout, out_layout};
    NttRemap* rs[2] = {&rin, &rout};
    for (int i = 0; i < 2; i++) {
        std::memset(rs[i], 0, sizeof(NttRemap));
        if (!ls[i]) continue;
        if (ls[i]->lo_bits + ls[i]->mid_bits > log_n || ls[i]->lo_bits < 2)
            return fail(ZKP_E_ARG, "layout: lo_bits must be >= 2 (16-byte runs of four elements) and lo_bits + mid_bits <= log_n");
        rs[i]->on = 1;
        rs[i]->lo_bits = ls[i]->lo_bits;
        rs[i]->mid_bits = ls[i]->mid_bits;
        rs[i]->mid_stride = ls[i]->mid_stride;
        rs[i]->hi_stride = ls[i]->hi_stride;
        rs[i]->batch_stride = ls[i]->batch_stride;
    }
    if (d_in == d_out && (in_layout || out_layout))
        return fail(ZKP_E_ARG, "a transform with a gathered or scattered layout cannot run in place");
    CTX_ENTER(-1);
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    WsOrder ord(st);
    NttIo io;
    io.in_remap = in_layout ? &rin : nullptr;
    io.out_remap = out_layout ? &rout : nullptr;
    io.tw_log_n = tw_log_n;
    io.tw_row0 = (uint64_t)tw_row0;
    return run_ntt<Fr>(reinterpret_cast<const Fr*>(d_in), reinterpret_cast<Fr*>(d_out), log_n, batch, inverse, nullptr, st, &io);
} ZKP_CATCH_INT

int zkp_poly_mul_fr(const uint64_t* a, size_t la, const uint64_t* b, size_t lb, uint64_t* out) try {
    if (la == 0 || lb == 0) return ZKP_OK;  // zero operand => zero polynomial (no coefficients)
    if (!a || !b || !out) return fail(ZKP_E_ARG, "null argument");
    const size_t lo = la + lb - 1;
    unsigned log_n = 0;
    while (((size_t)1 << log_n) < lo) log_n++;
    const size_t n = (size_t)1 << log_n;
    CTX_ENTER(-1);
    WsOrder ord(nullptr);
    ZCHK(ctx().tmp.ensure(2 * 32 * n));
    char* d = reinterpret_cast<char*>(ctx().tmp.p);
    HIPCHK(hipMemsetAsync(d, 0, 2 * 32 * n, nullptr));
    HIPCHK(hipMemcpyAsync(d, a, 32 * la, hipMemcpyHostToDevice, nullptr));
    HIPCHK(hipMemcpyAsync(d + 32 * n, b, 32 * lb, hipMemcpyHostToDevice, nullptr));
    ZCHK(run_ntt<Fr>(reinterpret_cast<Fr*>(d), log_n, 2, 0, nullptr, nullptr));
    hipLaunchKernelGGL(pointwise_mul_kernel<Fr>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, nullptr,
                       reinterpret_cast<const Fr*>(d), reinterpret_cast<const Fr*>(d + 32 * n), reinterpret_cast<Fr*>(d),
                       (uint64_t)n);
    HIPCHK(hipGetLastError());
    ZCHK(run_ntt<Fr>(reinterpret_cast<Fr*>(d), log_n, 1, 1, nullptr, nullptr));
    HIPCHK(hipMemcpyAsync(out, d, 32 * lo, hipMemcpyDeviceToHost, nullptr));
    HIPCHK(hipStreamSynchronize(nullptr));
    return ZKP_OK;
} ZKP_CATCH_INT

}  // extern "C"

#include "ntt_sharded.inc"
#include "plonk_host.inc"
#include "plonk_compile_host.inc"
#include "fri_host.inc"
#include "verify_host.inc"
#include "g1_check_host.inc"
#include "g1_codec_host.inc"
#include "kzg_handle.inc"
#include "g1_ntt_host.inc"
#include "kzg_recover_host.inc"
#include "kzg_cells_host.inc"
#include "kzg_evals_host.inc"
#include "kzg_points_host.inc"
#include "pairing_host.inc"
#include "nova_host.inc"
