// Host-side thread helpers of the library (pure C++17, no HIP): the resident pool for the serial tails of MSM batches, the uploader
// thread of host-fed MSMs and the caller's guard of an uploader job, the per-slot workers of the multi-device entries and the barrier
// their jobs meet at.  In a header of their own so that tests/abi/host_threads_stress.cpp
// can run them under ThreadSanitizer (tests/test_host_threads_cpu.py); api.hip includes this file inside its anonymous namespace.
#pragma once
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#ifndef ZKP_HOST_THREADS_E_DEVICE
#define ZKP_HOST_THREADS_E_DEVICE (-3)  // = ZKP_E_DEVICE (include/zkp_hip.h); api.hip asserts the equality
#endif
#ifndef ZKP_HOST_THREADS_OK
#define ZKP_HOST_THREADS_OK 0
#endif

// ----------------------------------------------------------------------------------------------------
// A few resident host threads for the short serial chains that follow a batch of MSMs (one Horner chain of ~35 group
// operations, ~30 us, per MSM).  Creating threads per call cost as much as the chains themselves (three chains: ~100 us with
// std::thread per call, the same as running them one after the other).  The workers are detached and the pool is never
// destroyed: they sleep on a condition variable between calls and end with the process.  run() serialises its callers; the jobs
// are pure host arithmetic and take no other lock.
// ----------------------------------------------------------------------------------------------------
class HostPool {
    std::mutex run_mu;  // one run() at a time
    std::mutex mu;
    std::condition_variable cv, cv_done;
    const std::function<void(size_t)>* fn = nullptr;
    size_t next = 0, total = 0, finished = 0;
    bool started = false;
    // warm(): a caller that knows a run() is coming within the next few hundred microseconds (the MSM is waiting for its last kernel)
    // wakes the workers early; they spin on `posted` until the job arrives or the deadline passes.  A sleeping thread takes 20-50 us
    // (at times hundreds) to come back, as long as the chains it is woken for (profiles/r05_q_host_pool_warm.md).
    std::atomic<bool> posted{false};
    std::chrono::steady_clock::time_point warm_until{};
    void worker() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return (fn != nullptr && next < total) || std::chrono::steady_clock::now() < warm_until; });
            if (!(fn != nullptr && next < total)) {  // woken early: spin outside the lock until a job is posted or the deadline passes
                const auto until = warm_until;
                lk.unlock();
                while (!posted.load(std::memory_order_acquire) && std::chrono::steady_clock::now() < until) __builtin_ia32_pause();
                lk.lock();
                if (!(fn != nullptr && next < total)) {
                    if (std::chrono::steady_clock::now() >= warm_until) warm_until = {};  // back to sleep
                    continue;
                }
            }
            const size_t i = next++;
            const std::function<void(size_t)>* f = fn;
            lk.unlock();
            (*f)(i);
            lk.lock();
            if (++finished == total) cv_done.notify_one();
        }
    }

public:
    void run(const std::function<void(size_t)>& f, size_t n) {
        std::lock_guard<std::mutex> one(run_mu);
        std::unique_lock<std::mutex> lk(mu);
        if (!started) {
            started = true;
            for (int i = 0; i < 3; i++) std::thread([this] { worker(); }).detach();
        }
        fn = &f;
        next = 0;
        total = n;
        finished = 0;
        warm_until = {};  // (a worker that finds no job left sleeps until the next run or warm)
        posted.store(true, std::memory_order_release);
        cv.notify_all();
        while (next < total) {  // the caller works too
            const size_t i = next++;
            lk.unlock();
            f(i);
            lk.lock();
            ++finished;
        }
        cv_done.wait(lk, [&] { return finished == total; });
        fn = nullptr;
        posted.store(false, std::memory_order_release);
        warm_until = {};
    }
    void warm(std::chrono::microseconds how_long) {
        std::unique_lock<std::mutex> lk(mu, std::try_to_lock);  // never wait for it: a run() in progress needs no warming
        if (!lk.owns_lock() || !started) return;
        warm_until = std::chrono::steady_clock::now() + how_long;
        cv.notify_all();
    }
};
HostPool& host_pool() {
    static HostPool* pool = new HostPool;  // intentionally leaked, see above
    return *pool;
}

// One resident host thread that issues the uploads of the later scalar ranges of a host-fed MSM (zkp_msm_g1) while the caller's thread
// enqueues the kernels of the first range: hipMemcpyAsync from pageable memory holds its caller for most of the transfer, and issued in
// line -- after the dozen launches of the first range -- the second upload started 100 us late and ended after the first range's kernels
// (profiles/r05_o_range_handover.md).  Same life cycle as the pool above: created on first use, detached, ends with the process.
// submit() hands over one job; wait() returns its result once it has run (every submit is followed by exactly one wait).
class Uploader {
    std::mutex mu;
    std::condition_variable cv, cv_done;
    std::function<int()> job;
    bool pending = false, running = false, started = false;
    int rc = ZKP_HOST_THREADS_OK;
    void worker() {
        std::unique_lock<std::mutex> lk(mu);
        for (;;) {
            cv.wait(lk, [&] { return pending; });
            pending = false;
            running = true;
            std::function<int()> f = std::move(job);
            lk.unlock();
            int r;
            try {
                r = f();
            } catch (...) {
                r = ZKP_HOST_THREADS_E_DEVICE;
            }
            lk.lock();
            rc = r;
            running = false;
            cv_done.notify_all();
        }
    }

public:
    void submit(std::function<int()> f) {
        std::unique_lock<std::mutex> lk(mu);
        if (!started) {
            started = true;
            std::thread([this] { worker(); }).detach();
        }
        job = std::move(f);
        pending = true;
        cv.notify_one();
    }
    int wait() {
        std::unique_lock<std::mutex> lk(mu);
        cv_done.wait(lk, [&] { return !pending && !running; });
        return rc;
    }
};
Uploader& uploader(int slot) {  // one per device slot (the chunk MSMs of sharded bases run concurrently, one caller thread per slot)
    static std::mutex mu;
    static std::vector<Uploader*> all;  // intentionally leaked, as the pool
    std::lock_guard<std::mutex> lk(mu);
    if (slot < 0) slot = 0;
    while (all.size() <= (size_t)slot) all.push_back(new Uploader);
    return *all[(size_t)slot];
}

// The caller's side of one Uploader job that issues the later scalar ranges of a host-fed MSM.  It owns everything the job shares
// with the caller (the hand-over flags and the range lengths), so the job never refers to the caller's frame; join() -- also run by
// the destructor, on every way out of the caller's scope, exceptions included -- cancels a job that was never released and waits
// for it.  The job is submitted before the caller issues the first range and spins until release(): a sleeping thread takes
// 50-300 us to come back, as long as the first upload itself.
class RangeUpload {
    std::atomic<uint64_t> issued_{0};  // later ranges whose upload has been issued
    std::atomic<int> rc_{ZKP_HOST_THREADS_OK}, go_{0};  // go: 0 wait, 1 issue, -1 give up
    std::vector<uint64_t> lens_;       // the later ranges' lengths
    Uploader* up_ = nullptr;           // != nullptr: a job was submitted and not yet joined

public:
    RangeUpload() = default;
    RangeUpload(const RangeUpload&) = delete;
    RangeUpload& operator=(const RangeUpload&) = delete;
    ~RangeUpload() { (void)join(); }
    // prepare() runs first; after release(true), issue(k, offset, length) for the later ranges k = 0, 1, ... (offsets from `first`)
    // until one returns an error
    template <class Prepare, class Issue>
    void submit(Uploader& up, std::vector<uint64_t> later, uint64_t first, Prepare prepare, Issue issue) {
        lens_ = std::move(later);
        up.submit([this, first, prepare, issue]() -> int {
            int rc = prepare();
            int go;
            while ((go = go_.load(std::memory_order_acquire)) == 0) __builtin_ia32_pause();  // the first range is being issued
            if (go < 0) return ZKP_HOST_THREADS_OK;  // the caller gave up
            uint64_t o = first;
            for (size_t k = 0; rc == ZKP_HOST_THREADS_OK && k < lens_.size(); o += lens_[k++])
                if ((rc = issue(k, o, lens_[k])) == ZKP_HOST_THREADS_OK) issued_.store(k + 1, std::memory_order_release);
            if (rc != ZKP_HOST_THREADS_OK) rc_.store(rc, std::memory_order_release);
            return rc;
        });
        up_ = &up;
    }
    void release(bool ok) { go_.store(ok ? 1 : -1, std::memory_order_release); }
    // true once the first k later ranges have been issued; false if the upload failed first
    bool wait_issued(uint64_t k) const {
        for (; issued_.load(std::memory_order_acquire) < k; __builtin_ia32_pause())
            if (rc_.load(std::memory_order_acquire) != ZKP_HOST_THREADS_OK) return false;
        return true;
    }
    // the job's result (ZKP_HOST_THREADS_OK when none was submitted); a job still waiting for release() is cancelled first
    int join() {
        if (!up_) return ZKP_HOST_THREADS_OK;
        int unreleased = 0;
        go_.compare_exchange_strong(unreleased, -1, std::memory_order_acq_rel);
        Uploader* up = up_;
        up_ = nullptr;
        return up->wait();
    }
};

// ----------------------------------------------------------------------------------------------------
// One resident host thread per device slot for the multi-device entries (zkp_init_devices): job i of a batch runs on thread i,
// enters its slot's context there and launches on that slot's stream, so the per-device pieces of one call (the chunk MSMs
// over sharded bases, the per-chunk SRS expansion, the slots of a sharded transform) run concurrently.  Threads are created on first
// use and joined by stop() (zkp_shutdown); a run() after a stop() starts them again.
// ----------------------------------------------------------------------------------------------------
class DeviceWorkers {
    struct W {
        std::thread th;
        std::mutex mu;
        std::condition_variable cv;
        const std::function<void()>* job = nullptr;
        bool busy = false, quit = false;
    };
    std::mutex run_mu;
    std::vector<W*> ws;
    static void loop(W* w) {
        std::unique_lock<std::mutex> lk(w->mu);
        for (;;) {
            w->cv.wait(lk, [&] { return w->job != nullptr || w->quit; });
            if (w->quit) return;
            const std::function<void()>* j = w->job;
            lk.unlock();
            (*j)();
            lk.lock();
            w->job = nullptr;
            w->busy = false;
            w->cv.notify_all();
        }
    }

public:
    void run(const std::vector<std::function<void()>>& jobs) {
        std::lock_guard<std::mutex> one(run_mu);
        while (ws.size() < jobs.size()) {
            W* w = new W;
            w->th = std::thread(loop, w);
            ws.push_back(w);
        }
        for (size_t i = 0; i < jobs.size(); i++) {
            std::lock_guard<std::mutex> lk(ws[i]->mu);
            ws[i]->job = &jobs[i];
            ws[i]->busy = true;
            ws[i]->cv.notify_all();
        }
        for (size_t i = 0; i < jobs.size(); i++) {
            std::unique_lock<std::mutex> lk(ws[i]->mu);
            ws[i]->cv.wait(lk, [&] { return !ws[i]->busy; });
        }
    }
    void stop() {
        std::lock_guard<std::mutex> one(run_mu);
        for (W* w : ws) {
            {
                std::lock_guard<std::mutex> lk(w->mu);
                w->quit = true;
                w->cv.notify_all();
            }
            w->th.join();
            delete w;
        }
        ws.clear();
    }
};

// Jobs that run side by side on the workers above meet here: every thread arrives with its own verdict and leaves with the
// conjunction, so a slot that failed takes the others out of their protocol at the same barrier and nobody is left waiting for an
// event that will never be recorded (ntt_sharded.inc).  Once false, the verdict stays false.  A waiter leaves with the verdict of ITS
// barrier (`verdict`, fixed by the last arrival), not with `ok`: a fast thread may already have arrived at the next barrier with `false`,
// and a waiter that read that would leave one barrier early while the fast thread waits for it at the next one for ever.
struct PhaseBarrier {
    std::mutex mu;
    std::condition_variable cv;
    size_t n = 1, arrived = 0;
    uint64_t gen = 0;
    bool ok = true, verdict = true;
    bool arrive(bool mine) {
        std::unique_lock<std::mutex> lk(mu);
        ok = ok && mine;
        if (++arrived == n) {
            arrived = 0;
            verdict = ok;
            gen++;
            cv.notify_all();
        } else {
            const uint64_t g0 = gen;
            cv.wait(lk, [&] { return gen != g0; });  // (the next barrier cannot complete, and overwrite `verdict`, before this thread arrives at it)
        }
        return verdict;
    }
};
