// Owning handles of the HIP resources the host side holds: device buffers, pinned host buffers, streams and events, and the polled
// wait on a stream (poll_or_sync, at the end).  Each type is
// move-only and releases its resource in its destructor with `(void)hip...`.  The destructors never synchronise and never switch
// device: an owner that may still have work in flight, or that lives on another device, drains it and makes its device current
// first (~Ctx, zkp_plonk_prover_destroy, zkp_g1_bases_destroy).  Kernels and launch sites receive the raw handles (.p, .get(),
// or the implicit conversion of Stream and Event).  api.hip includes this file inside its anonymous namespace, after fail() and hip_fail().
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdint>
#include <string>
#include <utility>

// One raw handle H released by Free; moves hand it over, copies do not exist.
template <class H, hipError_t (*Free)(H)>
class Owned {
protected:
    H h_ = nullptr;

public:
    Owned() = default;
    Owned(Owned&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Owned& operator=(Owned&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    Owned(const Owned&) = delete;
    Owned& operator=(const Owned&) = delete;
    ~Owned() { reset(); }
    void reset() {
        if (h_) (void)Free(h_);
        h_ = nullptr;
    }
    H get() const { return h_; }
    operator H() const { return h_; }
};

// Created on first use with the owner's flags (non-blocking streams; DisableTiming events except where they are timed).  make()
// returns the HIP error and leaves the handle empty on failure; ensure() reports it as "<create call>: <HIP error text>".
struct Stream : Owned<hipStream_t, hipStreamDestroy> {
    hipError_t make(unsigned flags) {
        if (h_) return hipSuccess;
        const hipError_t e = hipStreamCreateWithFlags(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
    int ensure(unsigned flags) {
        const hipError_t e = make(flags);
        return e == hipSuccess ? ZKP_OK : hip_fail(e, "hipStreamCreateWithFlags(&s, flags): ");
    }
};
struct Event : Owned<hipEvent_t, hipEventDestroy> {
    hipError_t make(unsigned flags) {
        if (h_) return hipSuccess;
        const hipError_t e = hipEventCreateWithFlags(&h_, flags);
        if (e != hipSuccess) h_ = nullptr;
        return e;
    }
    int ensure(unsigned flags) {
        const hipError_t e = make(flags);
        return e == hipSuccess ? ZKP_OK : hip_fail(e, "hipEventCreateWithFlags(&e, flags): ");
    }
};

// Grow-only allocation: grow(bytes) keeps the buffer when it is large enough, else replaces it.  On any failure it leaves
// p == nullptr, cap == 0: the old pointer is forgotten before it is freed, so no stale pointer or capacity survives an error.
// grow() returns the HIP error (for entries that report its bare text); ensure() reports "<HIP call>: <HIP error text>".
template <class Mem>
struct GrowBuf {
    void* p = nullptr;
    size_t cap = 0;
    GrowBuf() = default;
    GrowBuf(GrowBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
    GrowBuf& operator=(GrowBuf&& o) noexcept {
        if (this != &o) {
            release();
            p = std::exchange(o.p, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    GrowBuf(const GrowBuf&) = delete;
    GrowBuf& operator=(const GrowBuf&) = delete;
    ~GrowBuf() { release(); }
    hipError_t grow(size_t bytes, unsigned flags = Mem::FLAGS, const char** failed = nullptr) {
        if (bytes <= cap) return hipSuccess;
        void* old = std::exchange(p, nullptr);
        cap = 0;
        hipError_t e = old ? Mem::free(old) : hipSuccess;
        if (e != hipSuccess) {
            if (failed) *failed = Mem::FREE_CALL;
            return e;
        }
        e = Mem::alloc(&p, bytes, flags);
        if (e != hipSuccess) {
            p = nullptr;
            if (failed) *failed = Mem::ALLOC_CALL;
            return e;
        }
        cap = bytes;
        return hipSuccess;
    }
    int ensure(size_t bytes, unsigned flags = Mem::FLAGS) {
        const char* call = "";
        const hipError_t e = grow(bytes, flags, &call);
        return e == hipSuccess ? ZKP_OK : hip_fail(e, std::string(call) + ": ");
    }
    void release() {
        if (p) (void)Mem::free(p);
        p = nullptr;
        cap = 0;
    }
};
struct DeviceMem {
    static hipError_t alloc(void** p, size_t bytes, unsigned) { return hipMalloc(p, bytes); }
    static hipError_t free(void* p) { return hipFree(p); }
    static constexpr unsigned FLAGS = 0;
    static constexpr const char* ALLOC_CALL = "hipMalloc(&p, bytes)";
    static constexpr const char* FREE_CALL = "hipFree(p)";
};
struct PinnedMem {  // the owner gives the flags
    static hipError_t alloc(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
    static hipError_t free(void* p) { return hipHostFree(p); }
    static constexpr unsigned FLAGS = hipHostMallocDefault;
    static constexpr const char* ALLOC_CALL = "hipHostMalloc(&p, bytes, flags)";
    static constexpr const char* FREE_CALL = "hipHostFree(p)";
};
typedef GrowBuf<DeviceMem> DevBuf;     // device memory
typedef GrowBuf<PinnedMem> PinnedBuf;  // pinned host memory

template <class T, class Buf = DevBuf> struct TypedBuf : Buf {  // the same, holding T elements
    T* get() const { return static_cast<T*>(this->p); }
    operator T*() const { return get(); }
};

// Wait for the work on `st` whose end a kernel announces in pinned host memory (the MSM's result flags, the PLONK prover's sequence
// number): the stream wait costs 30-60 us of wake-up (profiles/r05_k), so the host spins on done() instead -- a pause between two
// looks, the clock every 1024 spins.  After POLL_TIMEOUT without the announcement (a kernel that faulted never writes it), or at
// once when `poll` is false, the stream wait.  From the return on the kernels' writes to pinned memory are visible to the host:
// done() reads with acquire loads.
constexpr std::chrono::seconds POLL_TIMEOUT(2);
template <class Done>
int poll_or_sync(bool poll, hipStream_t st, Done done) {
    if (poll) {
        const auto t0 = std::chrono::steady_clock::now();
        for (uint64_t spins = 0;; __builtin_ia32_pause()) {
            if (done()) return ZKP_OK;
            if ((++spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > POLL_TIMEOUT) break;
        }
    }
    const hipError_t e = hipStreamSynchronize(st);
    return e == hipSuccess ? ZKP_OK : hip_fail(e, "hipStreamSynchronize(st): ");
}
