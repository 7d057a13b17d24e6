#!/usr/bin/env python3
"""Reporting grid of SURVEY.md §8d on ONE GPU: MSM and Fr NTT at n = 2^20, 2^22, 2^24, 2^26 (inputs resident in HBM).
Prints a markdown table; the multi-GPU columns are produced by the driver's bench.py --gpus N runs.
--glv [LOG_N ...]: instead, the plain against the endomorphism-split expansion (zkp_g1_bases_precompute / _glv) of the same points in one
process, automatic widths, resident scalars, at 2^16, 2^20, 2^22, 2^24 (or the sizes given): expansion ms and bytes, ms per MSM (median
of alternating calls) and the msm_bucket_reduce / msm_tail_host phases from a profiled pass of its own."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zkp-implementation_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
import zkp_hip as zkp  # noqa: E402

zkp.init()
dev = torch.device("cuda", 0)


def glv_grid(logs):
    print(f"shader clock under the multiply-add probe: {zkp.probe_mad_rate(10)[1]:.0f} MHz")
    print("| n | mode | width | planes | expansion ms | expansion bytes | ms per MSM (median) | min..max | msm_bucket_reduce ms | msm_tail_host ms |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for ln in logs:
        n = 1 << ln
        ks = bench.rand_fr_tensor(torch, n, 1000 + ln, dev)
        sc = bench.rand_fr_tensor(torch, n, 2000 + ln, dev)
        pts = torch.zeros(n * 12, dtype=torch.int64, device=dev)
        zkp.g1_fixed_base_mul_dev(ks, n, pts)
        torch.cuda.synchronize()
        handles, expand_ms = {}, {}
        for mode in ("plain", "split"):  # back to back; the expansion is synchronous
            handles[mode] = zkp.G1Bases.from_device(pts, n)
            t0 = time.perf_counter()
            handles[mode].precompute(0, glv=mode == "split")
            expand_ms[mode] = (time.perf_counter() - t0) * 1e3
        del pts, ks
        res = {m: zkp.msm_g1_dev(h, sc, n) for m, h in handles.items()}  # warm-up of both shapes, and the results agree
        assert res["plain"][1] == res["split"][1] and np.array_equal(res["plain"][0], res["split"][0])
        reps = 30 if ln <= 20 else 10 if ln <= 22 else 5
        times = {"plain": [], "split": []}
        for _ in range(reps):  # alternating, so that a drift of the clock meets both alike
            for mode, h in handles.items():
                t0 = time.perf_counter()
                zkp.msm_g1_dev(h, sc, n)  # returns the host result: synchronous
                times[mode].append((time.perf_counter() - t0) * 1e3)
        phases = {}
        zkp.profile_enable(True)
        for mode, h in handles.items():
            zkp.profile_reset()
            for _ in range(3):
                zkp.msm_g1_dev(h, sc, n)
            phases[mode] = [zkp.profile_read(name)[0] / 3 for name in ("msm_bucket_reduce", "msm_tail_host")]
        zkp.profile_enable(False)
        for mode, h in handles.items():
            e, t = h.expansion(), sorted(times[mode])
            print(f"| 2^{ln} | {mode} | {e['window_bits']} | {e['planes']} | {expand_ms[mode]:.1f} | {e['bytes']} | {t[len(t) // 2]:.3f} | "
                  f"{t[0]:.3f}..{t[-1]:.3f} | {phases[mode][0]:.3f} | {phases[mode][1]:.3f} |", flush=True)
            h.close()
        del sc
        torch.cuda.empty_cache()


if "--glv" in sys.argv:
    glv_grid([int(a) for a in sys.argv[sys.argv.index("--glv") + 1:]] or [16, 20, 22, 24])
    sys.exit(0)
print("| workload | n | ms | throughput | algorithmic GB/s | % of 8 TB/s |")
print("|---|---|---|---|---|---|")
for ln in (20, 22, 24, 26):
    n = 1 << ln
    ks = bench.rand_fr_tensor(torch, n, 1000 + ln, dev)
    sc = bench.rand_fr_tensor(torch, n, 2000 + ln, dev)
    pts = torch.zeros(n * 12, dtype=torch.int64, device=dev)
    zkp.g1_fixed_base_mul_dev(ks, n, pts)
    torch.cuda.synchronize()
    bases = zkp.G1Bases.from_device(pts, n)
    del pts, ks
    for mode in ("plain c=16", "expanded c=20"):
        if mode.startswith("expanded"):
            t0 = time.perf_counter()
            bases.precompute(20)
            torch.cuda.synchronize()
            print(f"| (one-off SRS expansion) | 2^{ln} | {(time.perf_counter() - t0) * 1e3:.1f} | | | |", flush=True)
        zkp.msm_g1_dev(bases, sc, n)
        reps = 5 if ln <= 22 else 2
        t0 = time.perf_counter()
        for _ in range(reps):
            zkp.msm_g1_dev(bases, sc, n)
        dt = (time.perf_counter() - t0) / reps
        print(f"| G1 MSM, {mode} | 2^{ln} | {dt * 1e3:.2f} | {n / dt:.3e} scalar-muls/s | {128 * n / dt / 1e9:.1f} | "
              f"{128 * n / dt / 8e12 * 100:.2f} |", flush=True)
    bases.close()
    del sc
    torch.cuda.empty_cache()
for ln in (20, 22, 24, 26):
    n = 1 << ln
    data = bench.rand_fr_tensor(torch, n, 3000 + ln, dev).reshape(-1)
    ref = data.clone()
    zkp.ntt_fr_dev(data, ln)
    zkp.ntt_fr_dev(data, ln, inverse=True)
    torch.cuda.synchronize()
    assert torch.equal(data, ref)
    reps = 10 if ln <= 22 else 3
    t0 = time.perf_counter()
    for _ in range(reps):
        zkp.ntt_fr_dev(data, ln)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    print(f"| Fr NTT (one transform) | 2^{ln} | {dt * 1e3:.3f} | {n / dt:.3e} elem/s | {64 * n / dt / 1e9:.1f} | {64 * n / dt / 8e12 * 100:.2f} |", flush=True)
    del data, ref
    torch.cuda.empty_cache()
for ln in (20, 24, 26):
    n = 1 << ln
    g = torch.Generator(device=dev)
    g.manual_seed(ln)
    t = torch.randint(0, 2 ** 62, (n,), dtype=torch.int64, device=dev, generator=g)
    zkp.ntt_goldilocks_dev(t, ln)
    torch.cuda.synchronize()
    reps = 10
    t0 = time.perf_counter()
    for _ in range(reps):
        zkp.ntt_goldilocks_dev(t, ln)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    print(f"| Goldilocks NTT | 2^{ln} | {dt * 1e3:.3f} | {n / dt:.3e} elem/s | {16 * n / dt / 1e9:.1f} | {16 * n / dt / 8e12 * 100:.2f} |", flush=True)
