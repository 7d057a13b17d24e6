"""Batched cell verification (zkp_kzg_verify_cells_dev) against the per-cell route (zkp_kzg_verify_coset), one process, after a
warm-up of every shape; the shader clock of the library's multiply-add probe is printed before and after.  Not part of bench.py.
  - n = 2^13, l = 64 (r = 128 cells per blob): batches of N = 1, 2, 8, 128 (one blob) and 8192 (64 blobs) cells, host clock around
    the call (it blocks: it ends in the host's pairings), median of `--reps`, with the spread (max - min) / median
  - the split of one call between "kzg_cells_field", "kzg_cells_points" and "kzg_cells_pairing" from the library's own phase
    records, in a separate profiled call
  - next to these the median of zkp_kzg_verify_coset over 8 of the same cells: the only route before the batched entry, whose cost
    for N cells is N times that median (EXTRAPOLATED in the table, not run N times)
  - the sweep of ZKP_KZG_CELLS_CHUNK_LOG on the field half alone (zkp_kzg_cells_aggregate_dev, device events) at N = 8192, with the
    cells spread evenly over the cosets and with all of them in one coset
Prints markdown tables (profiles/kzg_verify_cells.md).
python tools/kzg_verify_cells_bench.py [--shape 13:6] [--blobs 64] [--chunk 0,1,2,3,4,5,6,8] [--reps 7]"""
import argparse
import os
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
ap.add_argument("--shape", default="13:6")
ap.add_argument("--blobs", type=int, default=64)
ap.add_argument("--chunk", default="0,1,2,3,4,5,6,8")
ap.add_argument("--reps", type=int, default=7)
args = ap.parse_args()
log_n, log_l = (int(x) for x in args.shape.split(":"))
n, l = 1 << log_n, 1 << log_l
r = n // l
KNOB = "ZKP_KZG_CELLS_CHUNK_LOG"
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SECRET = 0x1F2E3D4C5B6A7988

zkp.init()
dev = torch.device("cuda", 0)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).to(dev)


def clock():
    rate, mhz, _ = zkp.probe_mad_rate()
    return f"{mhz:.0f} MHz ({rate / 1e12:.2f} T lane-mads/s)"


def host_times(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def event_times(fn, reps):
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


print(f"shape (log_n, log_l) = ({log_n}, {log_l}): n = 2^{log_n}, l = {l}, r = {r} cells per blob, {args.blobs} blobs, median of {args.reps}")
print(f"shader clock of the multiply-add probe before: {clock()}\n")

# the blobs: polynomials of full length, their cells, proofs and commitments from the entries that were there before
secret = bench.fr_mont([SECRET])[0]
srs_xy = zkp.srs_g1(secret, n)
bases = zkp.G1Bases.from_host(srs_xy)
g2_sl = zkp.g2_mul(zkp.g2_generator(), bench.fr_mont([pow(SECRET, l, R)])[0])[0]
opener = zkp.KzgOpener(bases, log_n, log_l)
commits = np.zeros((args.blobs, 12), dtype=np.uint64)
cells_ev = np.zeros((args.blobs, r, l, 4), dtype=np.uint64)
cells_xy = np.zeros((args.blobs, r, 12), dtype=np.uint64)
for b in range(args.blobs):
    f = bench.rand_fr_tensor(torch, n, 100 + b, dev).cpu().numpy().view(np.uint64).reshape(n, 4)
    (xy, inf), ev = opener.open_cosets(f, evals=True)
    assert not inf.any()
    commits[b] = zkp.kzg_commit(bases, f)[0]
    cells_xy[b] = xy
    cells_ev[b] = ev.reshape(l, r, 4).transpose(1, 0, 2)  # coset k: ev[k::r]
opener.close()
rng = np.random.default_rng(7)


def batch(cells):
    """cells: [(blob, coset)] -> host and device forms"""
    ci = np.array([c[0] for c in cells], dtype=np.uint32)
    ki = np.array([c[1] for c in cells], dtype=np.uint32)
    ev = np.ascontiguousarray(cells_ev[ci, ki])
    xy = np.ascontiguousarray(cells_xy[ci, ki])
    wt = bench.fr_mont([int.from_bytes(rng.bytes(16), "little") for _ in cells])
    return dict(ci=ci, ki=ki, ev=ev, xy=xy, wt=wt, d_ev=to_dev(ev), d_xy=to_dev(xy), d_wt=to_dev(wt))


d_commits = to_dev(commits)
total = args.blobs * r
ver = zkp.KzgCellVerifier(bases, g2_sl, log_n, log_l, total, args.blobs)
every = [(b, k) for b in range(args.blobs) for k in range(r)]
w = pow(pow(7, (R - 1) >> 32, R), 1 << (32 - log_n), R)

# the per-cell route on 8 cells
singles = []
for b, k in every[:8]:
    x = bench.fr_mont([pow(w, k, R)])[0]
    ts = host_times(lambda: zkp.kzg_verify_coset(bases, g2_sl, (commits[b], 0), (cells_xy[b, k], 0), x, cells_ev[b, k]), 3)
    singles.append(statistics.median(ts))
per_cell = statistics.median(singles)
print(f"zkp_kzg_verify_coset, one cell: median {per_cell:.2f} ms over 8 cells (min {min(singles):.2f}, max {max(singles):.2f})\n")

print("| N cells | zkp_kzg_verify_cells_dev, median | spread | zkp_kzg_verify_cells (host arrays), median | field (profiled call) | "
      "points (profiled call) | pairing (profiled call) | N x per-cell median (extrapolated) | ratio |")
print("|---|---|---|---|---|---|---|---|---|")
for count in [c for c in (1, 2, 8, r, total) if c <= total]:
    bt = batch(every[:count])
    commits_used = max(int(bt["ci"].max()) + 1, 1)

    def run_dev():
        assert ver.verify_dev(d_commits, commits_used, bt["ci"], bt["ki"], bt["d_ev"], bt["d_xy"], bt["d_wt"])

    def run_host():
        assert ver.verify(commits[:commits_used], bt["ci"], bt["ki"], bt["ev"], bt["xy"], bt["wt"])

    ts = host_times(run_dev, args.reps)
    th = host_times(run_host, args.reps)
    med = statistics.median(ts)
    zkp.profile_reset()
    zkp.profile_enable(1)
    run_dev()
    torch.cuda.synchronize()
    phases = [zkp.profile_read(name)[0] for name in ("kzg_cells_field", "kzg_cells_points", "kzg_cells_pairing")]
    zkp.profile_enable(0)
    zkp.profile_reset()
    print(f"| {count} | {med:.2f} ms | {(max(ts) - min(ts)) / med * 100:.1f} % | {statistics.median(th):.2f} ms | {phases[0]:.3f} ms | "
          f"{phases[1]:.3f} ms | {phases[2]:.2f} ms | {count * per_cell:.1f} ms | {count * per_cell / med:.1f} x |", flush=True)
    # one altered evaluation is seen at this size too
    bad = bt["d_ev"].clone()
    bad[-1, -1, 0] ^= 1
    assert not ver.verify_dev(d_commits, commits_used, bt["ci"], bt["ki"], bad, bt["d_xy"], bt["d_wt"])
ver.close()

# the chunk log: the field half alone
print(f"\nzkp_kzg_cells_aggregate_dev at N = {total}, device events, median of {args.reps}:\n")
print("| ZKP_KZG_CELLS_CHUNK_LOG | cells spread over the cosets | all cells in one coset |")
print("|---|---|---|")
spread = batch(every)
one = batch([(b, 5) for b in range(args.blobs)] * r)
out_i = torch.zeros(l * 4, dtype=torch.int64, device=dev)
out_c = torch.zeros(args.blobs * 4, dtype=torch.int64, device=dev)
out_p = torch.zeros(total * 4, dtype=torch.int64, device=dev)
for chunk_log in [int(x) for x in args.chunk.split(",") if x]:
    os.environ[KNOB] = str(chunk_log)
    v = zkp.KzgCellVerifier(bases, g2_sl, log_n, log_l, total, args.blobs)
    del os.environ[KNOB]
    cols = []
    for bt in (spread, one):
        ts = event_times(lambda: v.aggregate_dev(args.blobs, bt["ci"], bt["ki"], bt["d_ev"], bt["d_wt"], out_i, out_c, out_p), args.reps)
        cols.append(f"{statistics.median(ts):.3f} ms ({(max(ts) - min(ts)) / statistics.median(ts) * 100:.0f} %)")
    print(f"| {chunk_log} | {cols[0]} | {cols[1]} |", flush=True)
    v.close()
print(f"\nshader clock of the multiply-add probe after: {clock()}")
