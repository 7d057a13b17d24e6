"""Cell recovery (zkp_kzg_recover_cosets_dev), one process, device events around each call, median of `--reps` after a warm-up of the
same shape, with the spread (max - min) / median; the shader clock of the library's multiply-add probe is printed before and after.
Not part of bench.py.
  - half of the r cosets missing, in three patterns: the first half, every other coset, a random half; len = n / 2 (exactly enough)
  - for every leaf width of the sweep (ZKP_KZG_RECOVER_LEAF_LOG, set around the creation of each recoverer)
  - the split of one call between the build of the vanishing polynomial and the transforms of n plus the pointwise passes, from the
    library's own phase records ("kzg_recover_zs", "kzg_recover_rest") in a separate profiled call
  - in the same run the three zkp_ntt_fr_dev calls of 2^log_n the algorithm cannot do without (inverse, forward on the coset,
    inverse on the coset): its floor, and the ratio of every row to it
Prints markdown tables (profiles/kzg_recover.md).
python tools/kzg_recover_bench.py [--shape 20:6] [--leaf 1,2,3,4,5,6,7,8] [--reps 5]"""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zkp-implementation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import zkp_hip as zkp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="20:6")
ap.add_argument("--leaf", default="1,2,3,4,5,6,7,8")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
log_n, log_l = (int(x) for x in args.shape.split(":"))
n, r = 1 << log_n, 1 << (log_n - log_l)
KNOB = "ZKP_KZG_RECOVER_LEAF_LOG"

zkp.init()
dev = torch.device("cuda", 0)


def event_times(fn, reps):
    """device times of `reps` calls of fn(), which enqueues on the current stream; one warm-up of the same shape first"""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def clock():
    rate, mhz, _ = zkp.probe_mad_rate()
    return f"{mhz:.0f} MHz ({rate / 1e12:.2f} T lane-mads/s)"


def mask(missing):
    present = np.ones(r, dtype=np.uint8)
    present[list(missing)] = 0
    return present


PATTERNS = [("first half", mask(range(r // 2))), ("every other", mask(range(0, r, 2))),
            ("random half", mask(random.Random(1).sample(range(r), r // 2)))]
length = n // 2
evals = bench.rand_fr_tensor(torch, n, 5, dev)
out = torch.zeros(length * 4, dtype=torch.int64, device=dev)
flag = torch.zeros(1, dtype=torch.int32, device=dev)
work = bench.rand_fr_tensor(torch, n, 6, dev)
g = bench.fr_mont([7])[0]


def three_transforms():
    zkp.ntt_fr_dev(work, log_n, inverse=True)
    zkp.ntt_fr_dev(work, log_n, coset=g)
    zkp.ntt_fr_dev(work, log_n, inverse=True, coset=g)


print(f"shape (log_n, log_l) = ({log_n}, {log_l}): n = 2^{log_n}, r = {r} cosets, {r // 2} missing, len = {length}, median of {args.reps}")
print(f"shader clock of the multiply-add probe before: {clock()}\n")
floor_before = event_times(three_transforms, args.reps)
print("| leaf width 2^v | pattern | zkp_kzg_recoverer_create (one call) | zkp_kzg_recover_cosets_dev, median | spread (max - min) / median | "
      "vanishing polynomial (profiled call) | transforms of n + pointwise (profiled call) | median / floor |")
print("|---|---|---|---|---|---|---|---|")
floor = statistics.median(floor_before)
rows = []
for leaf_log in [int(x) for x in args.leaf.split(",") if x]:
    os.environ[KNOB] = str(leaf_log)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    rc = zkp.KzgRecoverer(log_n, log_l)
    t_create = (time.perf_counter() - t0) * 1e3
    del os.environ[KNOB]
    for name, present in PATTERNS:
        ts = event_times(lambda: rc.recover_dev(evals, present, length, out, flag), args.reps)
        med = statistics.median(ts)
        zkp.profile_reset()
        zkp.profile_enable(1)
        rc.recover_dev(evals, present, length, out, flag)
        torch.cuda.synchronize()
        t_zs, t_rest = zkp.profile_read("kzg_recover_zs")[0], zkp.profile_read("kzg_recover_rest")[0]
        zkp.profile_enable(0)
        zkp.profile_reset()
        assert int(flag.item()) == 0  # exactly enough cells: every input is consistent
        rows.append((leaf_log, name, med))
        print(f"| {leaf_log} | {name} | {t_create:.1f} ms | {med:.3f} ms | {(max(ts) - min(ts)) / med * 100:.1f} % | {t_zs:.3f} ms | "
              f"{t_rest:.3f} ms | {med / floor:.2f} |", flush=True)
    rc.close()
floor_after = event_times(three_transforms, args.reps)
print(f"\nthree zkp_ntt_fr_dev calls of 2^{log_n} (inverse, forward on the coset, inverse on the coset), median of {args.reps}: "
      f"{statistics.median(floor_before):.3f} ms before the sweep, {statistics.median(floor_after):.3f} ms after it")
best = {}
for leaf_log, name, med in rows:
    best.setdefault(leaf_log, []).append(med)
if best:
    order = sorted(best, key=lambda k: statistics.mean(best[k]))
    print("mean over the patterns per leaf width: " + ", ".join(f"2^{k}: {statistics.mean(best[k]):.3f} ms" for k in sorted(best)) +
          f"; fastest: 2^{order[0]}")
print(f"\nshader clock of the multiply-add probe after: {clock()}")
