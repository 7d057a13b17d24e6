// Stress of the library's host-side thread helpers (csrc/host_threads.hpp) for ThreadSanitizer: tests/test_host_threads_cpu.py builds this
// with g++ -fsanitize=thread and runs it.  No GPU, no HIP: the helpers are plain C++.
//   HostPool: run() from several caller threads (serialised inside), with and without a preceding warm(), warm() without a run() after it
//   Uploader: submit() / wait() pairs whose job spins on a flag the submitter sets later (the shape of msm_partial_batch's use), a job that
//             throws, one uploader per slot from concurrent caller threads
//   RangeUpload: the guard of an uploader job -- released normally, released with an error, and a submitter that leaves its scope by
//             return or by throw before it releases the job: the guard must cancel and join it
//   DeviceWorkers: run() with 1 to 8 jobs (job i on thread i) over many rounds, from several caller threads (serialised inside), and again
//             after stop() has joined the threads
//   PhaseBarrier: the jobs of one run() meet at it generation after generation; one of them arrives with `false`, after which every
//             participant must leave with `false` at that same barrier (and at every later one)
#include <cstdio>
#include <cstdlib>
#include "host_threads.hpp"

static std::atomic<long> g_sum{0};

int main() {
    int bad = 0;
    // ---- HostPool
    for (int round = 0; round < 300; round++) {
        if (round % 3 == 0) host_pool().warm(std::chrono::microseconds(200));
        if (round % 7 == 6) { host_pool().warm(std::chrono::microseconds(50)); continue; }  // a warm() that no run() follows
        const size_t n = 1 + (size_t)(round % 5);
        std::vector<long> out(n, 0);
        const std::function<void(size_t)> job = [&](size_t i) {
            long s = 0;
            for (int k = 0; k < 2000; k++) s += (long)(i + 1) * k;
            out[i] = s;
        };
        host_pool().run(job, n);
        for (size_t i = 0; i < n; i++)
            if (out[i] != (long)(i + 1) * (2000L * 1999 / 2)) bad++;
    }
    {   // several caller threads: run() serialises them
        std::vector<std::thread> callers;
        for (int t = 0; t < 4; t++)
            callers.emplace_back([&, t] {
                for (int r = 0; r < 50; r++) {
                    if ((r + t) & 1) host_pool().warm(std::chrono::microseconds(100));
                    const std::function<void(size_t)> job = [&](size_t i) { g_sum.fetch_add((long)i + 1, std::memory_order_relaxed); };
                    host_pool().run(job, 3);
                }
            });
        for (auto& c : callers) c.join();
        if (g_sum.load() != 4L * 50 * 6) bad++;
    }
    // ---- Uploader
    for (int round = 0; round < 200; round++) {
        std::atomic<int> go{0};
        std::atomic<uint64_t> issued{0};
        long payload[4] = {0, 0, 0, 0};
        uploader(0).submit([&]() -> int {
            int g;
            while ((g = go.load(std::memory_order_acquire)) == 0) { }
            if (g < 0) return ZKP_HOST_THREADS_OK;
            for (int k = 0; k < 4; k++) {
                payload[k] = round + k;
                issued.store((uint64_t)k + 1, std::memory_order_release);
            }
            return round % 11 == 10 ? ZKP_HOST_THREADS_E_DEVICE : ZKP_HOST_THREADS_OK;
        });
        go.store(round % 13 == 12 ? -1 : 1, std::memory_order_release);
        if (round % 13 != 12)
            for (uint64_t k = 1; k <= 4; k++) {
                while (issued.load(std::memory_order_acquire) < k) { }
                if (payload[k - 1] != round + (long)k - 1) bad++;
            }
        const int rc = uploader(0).wait();
        const int want = (round % 13 != 12 && round % 11 == 10) ? ZKP_HOST_THREADS_E_DEVICE : ZKP_HOST_THREADS_OK;
        if (rc != want) bad++;
    }
    uploader(1).submit([]() -> int { throw 1; });
    if (uploader(1).wait() != ZKP_HOST_THREADS_E_DEVICE) bad++;
    {   // one uploader per slot, concurrent callers
        std::vector<std::thread> callers;
        std::atomic<int> errs{0};
        for (int slot = 0; slot < 4; slot++)
            callers.emplace_back([&, slot] {
                for (int r = 0; r < 50; r++) {
                    std::atomic<int> done{0};
                    uploader(slot).submit([&]() -> int { done.store(r + 1, std::memory_order_release); return ZKP_HOST_THREADS_OK; });
                    if (uploader(slot).wait() != ZKP_HOST_THREADS_OK || done.load(std::memory_order_acquire) != r + 1) errs++;
                }
            });
        for (auto& c : callers) c.join();
        bad += errs.load();
    }
    // ---- RangeUpload
    for (int round = 0; round < 200; round++) {
        std::atomic<int> issued_calls{0};
        const int mode = round % 4;  // 0 released, 1 released with an error, 2 leave by return, 3 leave by throw
        auto submitter = [&]() -> int {
            RangeUpload ru;
            ru.submit(uploader(2), std::vector<uint64_t>{3, 5, 7}, 2, [] { return ZKP_HOST_THREADS_OK; },
                      [&](size_t k, uint64_t off, uint64_t len) {
                          issued_calls.fetch_add(1, std::memory_order_relaxed);
                          const uint64_t want_off[3] = {2, 5, 10}, want_len[3] = {3, 5, 7};
                          if (off != want_off[k] || len != want_len[k]) return ZKP_HOST_THREADS_E_DEVICE;
                          return mode == 1 && k == 1 ? ZKP_HOST_THREADS_E_DEVICE : ZKP_HOST_THREADS_OK;
                      });
            if (mode == 2) return -1;
            if (mode == 3) throw round;
            ru.release(true);
            if (mode == 0 && !ru.wait_issued(3)) return 1;
            if (mode == 1 && ru.wait_issued(3)) return 1;
            return ru.join() == (mode == 0 ? ZKP_HOST_THREADS_OK : ZKP_HOST_THREADS_E_DEVICE) ? 0 : 1;
        };
        int r;
        try {
            r = submitter();
        } catch (int) {
            r = -1;
        }
        if (mode >= 2 ? (r != -1 || issued_calls.load() != 0) : r != 0) bad++;
        if (mode == 0 && issued_calls.load() != 3) bad++;
    }
    {   // the uploader is free again after a cancelled job
        std::atomic<int> done{0};
        uploader(2).submit([&]() -> int { done.store(1, std::memory_order_release); return ZKP_HOST_THREADS_OK; });
        if (uploader(2).wait() != ZKP_HOST_THREADS_OK || done.load(std::memory_order_acquire) != 1) bad++;
    }
    // ---- DeviceWorkers
    {
        DeviceWorkers workers;
        auto rounds = [&](int count, std::atomic<int>& errs) {
            for (int round = 0; round < count; round++) {
                const size_t n = 1 + (size_t)(round % 8);
                std::vector<long> out(n, 0);
                std::vector<std::function<void()>> jobs(n);
                for (size_t i = 0; i < n; i++) jobs[i] = [&out, i, round] { out[i] = (long)(i + 1) * (round + 1); };
                workers.run(jobs);
                for (size_t i = 0; i < n; i++)
                    if (out[i] != (long)(i + 1) * (round + 1)) errs++;
            }
        };
        std::atomic<int> errs{0};
        rounds(400, errs);
        {
            std::vector<std::thread> callers;
            for (int t = 0; t < 4; t++) callers.emplace_back([&] { rounds(100, errs); });
            for (auto& c : callers) c.join();
        }
        workers.stop();
        rounds(50, errs);  // the threads come back
        workers.stop();
        workers.stop();    // nothing left to join
        // ---- PhaseBarrier, on the workers as ntt_sharded.inc uses it
        for (int round = 0; round < 100; round++) {
            const size_t n = 2 + (size_t)(round % 7);
            const int generations = 6, bad_gen = round % generations;
            const size_t bad_one = (size_t)round % n;
            PhaseBarrier bar;
            bar.n = n;
            std::vector<int> left_at(n, -1);  // the barrier at which participant i was told `false`
            std::vector<long> seen(n, 0);
            std::vector<long> shared(n, 0);   // written before a barrier, read by the neighbour behind it
            std::vector<std::function<void()>> jobs(n);
            for (size_t i = 0; i < n; i++)
                jobs[i] = [&, i] {
                    for (int gen = 0; gen < generations; gen++) {
                        shared[i] = 1000L * gen + (long)i;
                        if (!bar.arrive(!(gen == bad_gen && i == bad_one))) {
                            left_at[i] = gen;
                            return;
                        }
                        seen[i] += shared[(i + 1) % n];
                        if (!bar.arrive(true)) {  // (nobody writes `shared` again before everybody has read it)
                            left_at[i] = -2;
                            return;
                        }
                    }
                };
            workers.run(jobs);
            long want = 0;
            for (int gen = 0; gen < bad_gen; gen++) want += 1000L * gen;
            for (size_t i = 0; i < n; i++)
                if (left_at[i] != bad_gen || seen[i] != want + (long)bad_gen * (long)((i + 1) % n)) errs++;
            bar.n = 1;  // a lone arrival: the verdict stays false
            if (bar.arrive(true)) errs++;
        }
        workers.stop();
        bad += errs.load();
    }
    std::printf("host threads stress: %d failures\n", bad);
    return bad ? 1 : 0;
}
