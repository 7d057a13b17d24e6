"""Batched verification of point openings (zkp_kzg_verify_points_dev) against the host loop it stands next to (zkp_kzg_batch_verify),
one process, after a warm-up of every shape; the shader clock of the library's multiply-add probe is printed before and after.  Not
part of bench.py.
  - openings of 16 polynomials of degree < 256 at random points (the degree is nothing to a verifier), made in scalars from the
    known secret of the SRS (y = f(z), W = [(f(s) - y) / (s - z)]G by the fixed-base entry), opening i against its own copy of its
    commitment: the identity index, the arrays zkp_kzg_batch_verify takes
  - N = 1, 2, 4, 8 (where the two routes cross), 64 and 4096: host clock around the call (it blocks: it ends in the host's
    pairings), median of `--reps`, with the spread (max - min) / median; the split of one call between "kzg_points_field",
    "kzg_points_points" and "kzg_points_pairing" from the library's own phase records, in a separate profiled call
  - zkp_kzg_batch_verify on the same arrays up to N = 64, median of `--reps`; at 4096 it is run once, and only when 64 times its
    time at N = 64 stays under `--host-limit` seconds (the table says which)
  - N = 4096 over the 16 commitments themselves (an index instead of 4096 copies)
  - zkp_kzg_verify_points_find_bad_dev at N = 4096 with one wrong value, and the pairing checks it took
Prints markdown tables (profiles/kzg_verify_points.md).
python tools/kzg_verify_points_bench.py [--sizes 1,2,4,8,64,4096] [--reps 7] [--host-limit 120]"""
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
import zkp_hip.kzg_points as kp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1,2,4,8,64,4096")
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--host-limit", type=float, default=120.0)
args = ap.parse_args()
sizes = [int(x) for x in args.sizes.split(",") if x]
total, polys, degree = max(sizes), 16, 256
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


def evaluate(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def fixed_base(scalars):
    count = len(scalars)
    xy = torch.zeros(count * 12, dtype=torch.int64, device=dev)
    inf = torch.zeros(count, dtype=torch.uint8, device=dev)
    zkp.g1_fixed_base_mul_dev(to_dev(bench.fr_mont(scalars)), count, xy, inf)
    torch.cuda.synchronize()
    assert not inf.any()
    return xy.cpu().numpy().view(np.uint64).reshape(count, 12)


print(f"{total} openings of {polys} polynomials of degree < {degree}, median of {args.reps}")
print(f"shader clock of the multiply-add probe before: {clock()}\n")

rng = np.random.default_rng(11)
rand = lambda: int.from_bytes(rng.bytes(32), "little") % R
coeffs = [[rand() for _ in range(degree)] for _ in range(polys)]
at_s = [evaluate(f, SECRET) for f in coeffs]
index = np.arange(total, dtype=np.uint32) % polys
zs_int = [rand() for _ in range(total)]
ys_int = [evaluate(coeffs[m], z) for m, z in zip(index, zs_int)]
quot = [(at_s[m] - y) * pow(SECRET - z, -1, R) % R for m, z, y in zip(index, zs_int, ys_int)]
commits16 = fixed_base(at_s)
commits = np.ascontiguousarray(commits16[index])  # opening i against its own copy: the arrays of zkp_kzg_batch_verify
proofs = fixed_base(quot)
zs, ys = bench.fr_mont(zs_int), bench.fr_mont(ys_int)
wt = bench.fr_mont([int.from_bytes(rng.bytes(16), "little") for _ in range(total)])
g2s = zkp.g2_mul(zkp.g2_generator(), bench.fr_mont([SECRET])[0])[0]
d_commits, d_commits16, d_proofs, d_zs, d_ys, d_wt = (to_dev(a) for a in (commits, commits16, proofs, zs, ys, wt))
ver = kp.KzgPointVerifier(g2s, total, total)


def phases(fn):
    zkp.profile_reset()
    zkp.profile_enable(1)
    fn()
    torch.cuda.synchronize()
    out = [zkp.profile_read(name) for name in ("kzg_points_field", "kzg_points_points", "kzg_points_pairing")]
    zkp.profile_enable(0)
    zkp.profile_reset()
    return out


print("| N openings | zkp_kzg_verify_points_dev, median | spread | zkp_kzg_verify_points (host arrays), median | field (profiled call) | "
      "points (profiled call) | pairing (profiled call) | zkp_kzg_batch_verify (host loop) | ratio |")
print("|---|---|---|---|---|---|---|---|---|")
host_ms, dev_ms = {}, {}
for count in sizes:
    def run_dev():
        assert ver.verify_dev(d_commits, count, count, d_zs, d_ys, d_proofs, d_wt)

    def run_host():
        assert ver.verify(commits[:count], zs[:count], ys[:count], proofs[:count], wt[:count])

    def run_old():
        assert zkp.kzg_batch_verify(g2s, commits[:count], zs[:count], proofs[:count], ys[:count], wt[:count])

    ts = host_times(run_dev, args.reps)
    th = host_times(run_host, args.reps)
    med = dev_ms[count] = statistics.median(ts)
    ph = phases(run_dev)
    if count <= 64:
        host_ms[count] = statistics.median(host_times(run_old, args.reps))
        old = f"{host_ms[count]:.2f} ms (median of {args.reps})"
    elif host_ms and max(host_ms.values()) * count / max(host_ms) / 1e3 <= args.host_limit:
        t0 = time.perf_counter()
        run_old()
        host_ms[count] = (time.perf_counter() - t0) * 1e3
        old = f"{host_ms[count]:.0f} ms (run once)"
    else:
        old = "not run"
    ratio = f"{host_ms[count] / med:.2f} x" if count in host_ms else "-"
    print(f"| {count} | {med:.2f} ms | {(max(ts) - min(ts)) / med * 100:.1f} % | {statistics.median(th):.2f} ms | {ph[0][0]:.3f} ms | "
          f"{ph[1][0]:.3f} ms | {ph[2][0]:.2f} ms | {old} | {ratio} |", flush=True)
    bad = d_ys.clone()  # one altered value is seen at this size too
    bad[count - 1, 0] ^= 1
    assert not ver.verify_dev(d_commits, count, count, d_zs, bad, d_proofs, d_wt)


wins = [c for c in sizes if c in host_ms and host_ms[c] > dev_ms[c]]
print(f"\nthe device entry first wins at N = {wins[0]} of the sizes run" if wins else "\nthe device entry wins at none of the sizes run")


def run_indexed():
    assert ver.verify_dev(d_commits16, polys, total, d_zs, d_ys, d_proofs, d_wt, commit_index=index)


ts = host_times(run_indexed, args.reps)
ph = phases(run_indexed)
print(f"\nN = {total} over the {polys} commitments (commit_index): median {statistics.median(ts):.2f} ms, field {ph[0][0]:.3f} ms, "
      f"points {ph[1][0]:.3f} ms, pairing {ph[2][0]:.2f} ms")

bad_at = total - total // 3
bad = d_ys.clone()
bad[bad_at, 0] ^= 1


def run_find():
    assert ver.find_bad_dev(d_commits16, polys, total, d_zs, bad, d_proofs, d_wt, commit_index=index) == bad_at


ts = host_times(run_find, max(args.reps // 2, 1))
ph = phases(run_find)
print(f"zkp_kzg_verify_points_find_bad_dev, N = {total}, opening {bad_at} wrong: median {statistics.median(ts):.1f} ms in {ph[2][1]} pairing checks "
      f"(field {ph[0][0]:.3f} ms, points {ph[1][0]:.3f} ms, pairings {ph[2][0]:.1f} ms); one zkp_kzg_verify per opening would be {total} pairing checks")
ver.close()
print(f"\nshader clock of the multiply-add probe after: {clock()}")
