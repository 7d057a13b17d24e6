"""Pairing-product checks on the device (zkp_pairing_check_batch_dev, k = 2, validate = 0) against the one host check that gives a
per-item verdict without them (zkp_kzg_verify), one process, after a warm-up of every shape; the shader clock of the library's
multiply-add probe is printed before and after.  Not part of bench.py.
  - check c is e(P_c1, G_2) e(P_c2, [s]_2) == 1 over points made in scalars ([a]G and [-a / s]G by the fixed-base entry): the shape of
    one KZG opening's check.  Every odd check is broken, and the verdict bytes are compared with that before anything is timed
  - n = 1, 64, 1024, 4096: events around the call on the stream, median of `--reps` after a warm-up, with the spread
    (max - min) / median, and the split between "pairing_miller" and "pairing_final_exp" from the library's phase records in a
    separate profiled call
  - zkp_kzg_verify on one opening, median of `--reps`, under ZKP_PAIRING_FINAL_EXP=chain (the default) and =plain
  - zkp_kzg_verify_points_each_dev at the same sizes (host clock: it blocks), with its three phases
Prints markdown tables (profiles/pairing_dev.md).
python tools/pairing_bench.py [--sizes 1,64,1024,4096] [--reps 5]"""
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
import zkp_hip.pairing as zp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="1,64,1024,4096")
ap.add_argument("--reps", type=int, default=5)
args = ap.parse_args()
sizes = [int(x) for x in args.sizes.split(",") if x]
total = max(sizes)
R = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SECRET = 0x1F2E3D4C5B6A7988

zkp.init()
dev = torch.device("cuda", 0)


def to_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).to(dev)


def clock():
    rate, mhz, _ = zkp.probe_mad_rate()
    return f"{mhz:.0f} MHz ({rate / 1e12:.2f} T lane-mads/s)"


def event_times(fn, reps):
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return out


def host_times(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


print(f"pairing-product checks, k = 2 (G_2, [s]_2), validate = 0, median of {args.reps}")
print(f"shader clock of the multiply-add probe before: {clock()}\n")

rng = np.random.default_rng(12)
s_inv = pow(SECRET, -1, R)
scalars = []
for c in range(total):
    a = int.from_bytes(rng.bytes(32), "little") % R
    scalars += [a, (-a * s_inv + (c & 1)) % R]  # a * 1 + (-a / s) * s = 0; every odd check is one off
xy = torch.zeros(2 * total * 12, dtype=torch.int64, device=dev)
zkp.g1_fixed_base_mul_dev(to_dev(bench.fr_mont(scalars)), 2 * total, xy, None)
g2s = zkp.g2_mul(zkp.g2_generator(), bench.fr_mont([SECRET])[0])[0]
checker = zp.PairingChecker(np.stack([zkp.g2_generator(), g2s]), total)
ok = torch.zeros(total, dtype=torch.uint8, device=dev)
checker.check_batch_dev(xy, total, ok_tensor=ok, validate=False)
torch.cuda.synchronize()
assert ok.cpu().numpy().tolist() == [1 - (c & 1) for c in range(total)], "the verdicts are wrong: nothing is timed"


def phases(fn):
    zkp.profile_reset()
    zkp.profile_enable(1)
    fn()
    torch.cuda.synchronize()
    out = [zkp.profile_read(name)[0] for name in ("pairing_miller", "pairing_final_exp")]
    zkp.profile_enable(0)
    zkp.profile_reset()
    return out

# one host check: zkp_kzg_verify of one honest opening, f = X at z = 7: C = [s]G, y = 7, W = [(s - z) / (s - z)]G = G
f_s = SECRET % R
z = 7
w_scalar = 1
pts = torch.zeros(2 * 12, dtype=torch.int64, device=dev)
zkp.g1_fixed_base_mul_dev(to_dev(bench.fr_mont([f_s, w_scalar])), 2, pts, None)
torch.cuda.synchronize()
cw = pts.cpu().numpy().view(np.uint64).reshape(2, 12)
y_l, z_l = bench.fr_mont([z])[0], bench.fr_mont([z])[0]
host = {}
for mode in ("chain", "plain"):
    os.environ["ZKP_PAIRING_FINAL_EXP"] = mode

    def run_host():
        assert zkp.kzg_verify(g2s, (cw[0], 0), (cw[1], 0), y_l, z_l)

    host[mode] = statistics.median(host_times(run_host, args.reps))
os.environ.pop("ZKP_PAIRING_FINAL_EXP", None)
print(f"one host check (zkp_kzg_verify, two Miller loops and one final exponentiation): {host['chain']:.2f} ms with the x-chain "
      f"(ZKP_PAIRING_FINAL_EXP=chain, the default), {host['plain']:.2f} ms with the plain power (=plain)\n")

print("| n checks | zkp_pairing_check_batch_dev, median | spread | per check | Miller (profiled call) | final exponentiation (profiled call) | "
      "n x host check (chain) | n x host check (plain) |")
print("|---|---|---|---|---|---|---|---|")
dev_ms = {}
for n in sizes:
    def run():
        checker.check_batch_dev(xy, n, ok_tensor=ok, validate=False)

    ts = event_times(run, args.reps)
    med = dev_ms[n] = statistics.median(ts)
    ph = phases(run)
    print(f"| {n} | {med:.2f} ms | {(max(ts) - min(ts)) / med * 100:.1f} % | {med / n * 1e3:.1f} us | {ph[0]:.2f} ms | {ph[1]:.2f} ms | "
          f"{n * host['chain']:.0f} ms | {n * host['plain']:.0f} ms |", flush=True)

# a verdict per opening: zkp_kzg_verify_points_each_dev over openings of f = X (C = [s]G, y_i = z_i, W_i = G), every odd value one off
import zkp_hip.kzg_points as kp  # noqa: E402

zs_int = [int.from_bytes(rng.bytes(32), "little") % R for _ in range(total)]
d_zs = to_dev(bench.fr_mont(zs_int))
d_ys = to_dev(bench.fr_mont([(zv + (i & 1)) % R for i, zv in enumerate(zs_int)]))
d_commit = pts[:12].clone()
d_proofs = pts[12:].repeat(total)
index = np.zeros(total, dtype=np.uint32)
ver = kp.KzgPointVerifier(g2s, total, 1)
each_ok = torch.zeros(total, dtype=torch.uint8, device=dev)
assert ver.verify_each_dev(d_commit, 1, total, d_zs, d_ys, d_proofs, each_ok, commit_index=index) == total // 2
assert each_ok.cpu().numpy().tolist() == [1 - (i & 1) for i in range(total)], "the verdicts are wrong: nothing is timed"
print("\n| n openings | zkp_kzg_verify_points_each_dev, median (host clock, it blocks) | spread | per opening | left points (profiled call) | "
      "Miller | final exponentiation | n x host check (chain) |")
print("|---|---|---|---|---|---|---|---|")
each_ms = {}
for n in sizes:
    def run_each():
        ver.verify_each_dev(d_commit, 1, n, d_zs, d_ys, d_proofs, each_ok, commit_index=index[:n])

    ts = host_times(run_each, args.reps)
    med = each_ms[n] = statistics.median(ts)
    zkp.profile_reset()
    zkp.profile_enable(1)
    run_each()
    ph = [zkp.profile_read(name)[0] for name in ("kzg_each_points", "pairing_miller", "pairing_final_exp")]
    zkp.profile_enable(0)
    zkp.profile_reset()
    print(f"| {n} | {med:.2f} ms | {(max(ts) - min(ts)) / med * 100:.1f} % | {med / n * 1e3:.1f} us | {ph[0]:.2f} ms | {ph[1]:.2f} ms | {ph[2]:.2f} ms | "
          f"{n * host['chain']:.0f} ms |", flush=True)
ver.close()

for mode in ("chain", "plain"):
    wins = [n for n in sizes if n * host[mode] > dev_ms[n]]
    print(f"\nagainst n x the host check ({mode}) the device entry first wins at n = {wins[0]} of the sizes run" if wins
          else f"\nagainst n x the host check ({mode}) the device entry wins at none of the sizes run")
checker.close()
print(f"\nshader clock of the multiply-add probe after: {clock()}")
