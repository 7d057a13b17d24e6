"""Evaluation-form openings (zkp_kzg_open_evals_batch_dev) against what the library offered for the same result before: one batched
inverse zkp_ntt_fr_dev of the rows, the copy of the coefficients to the host, and P calls of zkp_kzg_open over the monomial SRS.  One
process; device events around each window, median of `--reps` after a warm-up of the same shape, with the spread (max - min) /
median; the two windows are timed alternately, and the shader clock of the library's multiply-add probe is printed before and after.
Not part of bench.py.
  - rows of random values in natural order, one random point per row; both SRS handles expanded as KzgScheme expands them
  - rows 0 and P - 1 of the batch are byte for byte what the old path returns for them, before anything is timed
  - the field half alone (zkp_kzg_open_evals_field_dev) with ZKP_KZG_EVALS_INVERSE at 0 (division steps) and at 1 (the Fermat power),
    timed alternately
  - the split of one batch call between the field half and the points, from the library's own phase records ("kzg_evals_field",
    "kzg_evals_points") in a separate profiled call
Prints markdown tables (profiles/kzg_open_evals.md).
python tools/kzg_open_evals_bench.py [--shapes 12:1,12:16,12:64,20:1,20:4] [--reps 5] [--no-expand]"""
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
from zkp_hip import kzg_evals  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="12:1,12:16,12:64,20:1,20:4")
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--no-expand", action="store_true")
args = ap.parse_args()
shapes = {}
for item in args.shapes.split(","):
    log_n, polys = (int(x) for x in item.split(":"))
    shapes.setdefault(log_n, []).append(polys)
KNOB = "ZKP_KZG_EVALS_INVERSE"

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


def pct(x):
    return f"{x * 100:.1f} %"


secret = np.array([0x1F2E3D4C5B6A7988, 0, 0, 0], dtype=np.uint64)
print(f"median of {args.reps} after a warm-up; SRS handles {'plain' if args.no_expand else 'expanded (precompute(0))'}")
print(f"shader clock of the multiply-add probe before: {clock()}\n")
open_rows, field_rows = [], []
for log_n, batches in shapes.items():
    n, max_polys = 1 << log_n, max(batches)
    mono = zkp.G1Bases.from_host(zkp.srs_g1(secret, n))
    lag = mono.lagrange(log_n)
    if not args.no_expand:
        mono.precompute(0)
        lag.precompute(0)
    op = kzg_evals.KzgEvalOpener(lag, log_n, max_polys)
    rows = bench.rand_fr_tensor(torch, n * max_polys, 5 + log_n, dev)
    zs = bench.rand_fr_tensor(torch, max_polys, 7 + log_n, dev)
    zs_host = zs.cpu().numpy().view(np.uint64).reshape(max_polys, 4)
    scratch = torch.empty_like(rows)
    d_y = torch.zeros(4 * max_polys, dtype=torch.int64, device=dev)
    d_q = torch.zeros(4 * n * max_polys, dtype=torch.int64, device=dev)

    def batch_call(polys):
        return op.open_batch_dev(rows, polys, zs)

    def parent_calls(polys):
        """scratch holds a copy of the rows (made outside the window): transform, copy out, one zkp_kzg_open per row"""
        zkp.ntt_fr_dev(scratch, log_n, batch=polys, inverse=True)
        coeffs = scratch[:polys * n].cpu().numpy().view(np.uint64).reshape(polys, n, 4)
        return [zkp.kzg_open(mono, coeffs[p], zs_host[p]) for p in range(polys)]

    def refill(polys):
        scratch[:polys * n].copy_(rows[:polys * n])
        torch.cuda.synchronize()

    def field_call(polys, method):
        os.environ[KNOB] = str(method)
        try:
            op.field_dev(rows, polys, zs, d_y, d_q)
        finally:
            del os.environ[KNOB]

    # rows 0 and P - 1 of the largest batch are what the old path returns for them
    (bxy, binf), by = batch_call(max_polys)
    refill(max_polys)
    old = parent_calls(max_polys)
    for p in (0, max_polys - 1):
        (oxy, oinf), oy = old[p]
        assert bxy[p].tobytes() == oxy.tobytes() and binf[p] == oinf and np.array_equal(by[p], oy), (log_n, p)

    for polys in batches:
        refill(polys)
        parent_calls(polys)  # warm-up of both, same shape
        batch_call(polys)
        torch.cuda.synchronize()
        ts_parent, ts_batch = [], []
        for _ in range(args.reps):  # alternately: what disturbs one disturbs the other
            refill(polys)
            ts_parent += event_times(lambda: parent_calls(polys), 1)
            ts_batch += event_times(lambda: batch_call(polys), 1)
        zkp.profile_reset()
        zkp.profile_enable(1)
        batch_call(polys)
        torch.cuda.synchronize()
        t_field, t_points = zkp.profile_read("kzg_evals_field")[0], zkp.profile_read("kzg_evals_points")[0]
        zkp.profile_enable(0)
        zkp.profile_reset()
        mp, mb = statistics.median(ts_parent), statistics.median(ts_batch)
        open_rows.append(f"| {log_n} | {polys} | {mp:.3f} ms | {pct(spread(ts_parent))} | {mb:.3f} ms | {pct(spread(ts_batch))} | {mp / mb:.2f} | "
                         f"{t_field:.3f} ms | {t_points:.3f} ms |")
        for method in (0, 1):
            field_call(polys, method)
        torch.cuda.synchronize()
        ts = {0: [], 1: []}
        for _ in range(args.reps):
            for method in (0, 1):
                ts[method] += event_times(lambda: field_call(polys, method), 1)
        m0, m1 = statistics.median(ts[0]), statistics.median(ts[1])
        field_rows.append(f"| {log_n} | {polys} | {m0:.4f} ms | {pct(spread(ts[0]))} | {m1:.4f} ms | {pct(spread(ts[1]))} | {m1 / m0:.2f} | "
                          f"{pct((m1 - m0) / m1)} |")
    op.close()
    del mono, lag

print("| log_n | P | inverse transform + copy + P calls of zkp_kzg_open, median | spread | one zkp_kzg_open_evals_batch_dev, median | spread | "
      "old / batch | field half (profiled batch call) | points (profiled batch call) |")
print("|---|---|---|---|---|---|---|---|---|")
print("\n".join(open_rows))
print("\n| log_n | P | zkp_kzg_open_evals_field_dev, division steps (0), median | spread | Fermat power (1), median | spread | "
      "Fermat / division steps | saved by division steps |")
print("|---|---|---|---|---|---|---|---|")
print("\n".join(field_rows))
print(f"\nshader clock of the multiply-add probe after: {clock()}")
