"""Batched cell recovery (zkp_kzg_recover_cosets_batch_dev) against P calls of zkp_kzg_recover_cosets_dev on the same handle in the
same process: device events around each window, median of `--reps` after a warm-up of the same shape, with the spread
(max - min) / median; the two are timed alternately, and the shader clock of the library's multiply-add probe is printed before and
after.  Not part of bench.py.
  - half of the r cosets missing (every other one), len = n / 2 (exactly enough), both layouts of the evaluations
  - the rows of a batch against the single entry's results for the first and the last row, bit for bit, before anything is timed
  - the split of one batch call between the build of the vanishing polynomial and everything behind it, from the library's own
    phase records ("kzg_recover_zs", "kzg_recover_rest") in a separate profiled call
  - the bytes the masked multiply moves (read the present half, write every element: 48 B per element) for the rate of that kernel,
    whose time comes from a kernel trace of this script (rocprofv3 --kernel-trace --stats -- python tools/kzg_recover_batch_bench.py
    --trace): --trace runs one warmed call per layout and batch and nothing else
Prints a markdown table (profiles/kzg_recover_batch.md).
python tools/kzg_recover_batch_bench.py [--shape 13:6] [--polys 1,16,64,128] [--reps 5] [--trace]"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zkp-implementation_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import zkp_hip as zkp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shape", default="13:6")
ap.add_argument("--polys", default="1,16,64,128")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--trace", action="store_true")
args = ap.parse_args()
log_n, log_l = (int(x) for x in args.shape.split(":"))
n, r = 1 << log_n, 1 << (log_n - log_l)
batches = [int(x) for x in args.polys.split(",") if x]
max_polys = max(batches)

zkp.init()
dev = torch.device("cuda", 0)


def event_times(fn, reps):
    """device times of `reps` calls of fn(), which enqueues on the current stream"""
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


def spread(ts):
    return (max(ts) - min(ts)) / statistics.median(ts)


present = np.ones(r, dtype=np.uint8)
present[0:r:2] = 0
length = n // 2
evals = bench.rand_fr_tensor(torch, n * max_polys, 5, dev)  # rows of field elements; natural order and cell layout read the same buffer
rows = evals.view(max_polys, n * 4)
out = torch.zeros(max_polys * length * 4, dtype=torch.int64, device=dev)
out_single = torch.zeros(length * 4, dtype=torch.int64, device=dev)
flags = torch.zeros(max_polys, dtype=torch.int32, device=dev)
rc = zkp.KzgRecoverer(log_n, log_l, max_polys)


def batch_call(polys, cells):
    rc.recover_batch_dev(evals, polys, present, length, length, out, flags, cells=cells)


def single_calls(polys):
    for p in range(polys):
        rc.recover_dev(rows[p], present, length, out_single, flags)


if args.trace:
    for polys in batches:
        for cells in (False, True):
            batch_call(polys, cells)
            batch_call(polys, cells)
    torch.cuda.synchronize()
    print(f"traced: two calls per layout at ({log_n}, {log_l}) for P in {batches}; the masked multiply moves 48 B per element: " +
          ", ".join(f"P = {p}: {48 * n * p} B" for p in batches))
    sys.exit(0)

# natural order: rows 0 and P - 1 of the largest batch are what the single entry returns for them
batch_call(max_polys, False)
torch.cuda.synchronize()
got = out.cpu().numpy().reshape(max_polys, -1)
for p in (0, max_polys - 1):
    rc.recover_dev(rows[p], present, length, out_single, flags)
    torch.cuda.synchronize()
    assert np.array_equal(got[p], out_single.cpu().numpy()), p

print(f"shape (log_n, log_l) = ({log_n}, {log_l}): n = 2^{log_n}, r = {r} cosets, {r // 2} missing, len = {length}, median of {args.reps}, "
      f"one recoverer of max_polys = {max_polys}")
print(f"shader clock of the multiply-add probe before: {clock()}\n")
print("| P | layout | P calls of zkp_kzg_recover_cosets_dev, median | spread | one zkp_kzg_recover_cosets_batch_dev, median | spread | "
      "singles / batch | vanishing polynomial (profiled batch call) | everything behind it (profiled batch call) |")
print("|---|---|---|---|---|---|---|---|---|")
for polys in batches:
    for cells in (False, True):
        single_calls(polys)  # warm-up of both, same shape
        batch_call(polys, cells)
        torch.cuda.synchronize()
        ts_single, ts_batch = [], []
        for _ in range(args.reps):  # alternately: what disturbs one disturbs the other
            ts_single += event_times(lambda: single_calls(polys), 1)
            ts_batch += event_times(lambda: batch_call(polys, cells), 1)
        zkp.profile_reset()
        zkp.profile_enable(1)
        batch_call(polys, cells)
        torch.cuda.synchronize()
        t_zs, t_rest = zkp.profile_read("kzg_recover_zs")[0], zkp.profile_read("kzg_recover_rest")[0]
        zkp.profile_enable(0)
        zkp.profile_reset()
        assert not flags[:polys].any().item()  # exactly enough cells: every input is consistent
        ms, mb = statistics.median(ts_single), statistics.median(ts_batch)
        print(f"| {polys} | {'cells' if cells else 'natural'} | {ms:.3f} ms | {spread(ts_single) * 100:.1f} % | {mb:.3f} ms | "
              f"{spread(ts_batch) * 100:.1f} % | {ms / mb:.2f} | {t_zs:.3f} ms | {t_rest:.3f} ms |", flush=True)
print(f"\nshader clock of the multiply-add probe after: {clock()}")
rc.close()
