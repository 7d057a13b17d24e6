"""The coset openings of a batch of polynomials (zkp_kzg_open_cosets_batch_dev) next to as many single calls, one process, device
events around each measurement, median of three after a warm-up of the same shape with the spread (max - min) / median; the shader
clock of the library's multiply-add probe is printed before and after.  Not part of bench.py.
  - per (log_n, log_l) and n_polys: one batch call, its time per polynomial, its split between the library's own phase records
    ("kzg_open_scalars", "kzg_open_mac", "kzg_open_transforms", from one separate profiled call) and, in the same process, n_polys
    sequential zkp_kzg_open_cosets_dev calls on an opener made for one polynomial
  - the sweep of the group size B = 1, 2, 4 of the multiply-accumulate pass (ZKP_KZG_COSET_GROUP_LOG, set around the creation of
    each opener) at the shapes and batch sizes of --groups
Prints markdown tables (profiles/kzg_open_cosets_batch.md).
python tools/kzg_open_batch_bench.py [--shapes 12:6:1,2,4,8,16,32,64/13:6:1,2,4,8,16,32,64/16:6:1,4,16] [--groups 13:6:16,64]
(an empty value skips a part)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zkp-implementation_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
import zkp_hip as zkp  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--shapes", default="12:6:1,2,4,8,16,32,64/13:6:1,2,4,8,16,32,64/16:6:1,4,16")
ap.add_argument("--groups", default="13:6:16,64")
args = ap.parse_args()
KNOB = "ZKP_KZG_COSET_GROUP_LOG"
PHASES = ("kzg_open_scalars", "kzg_open_mac", "kzg_open_transforms")

zkp.init()
dev = torch.device("cuda", 0)
SECRET = bench.fr_mont([0x1F2E3D4C5B6A7988])[0]


def shapes_of(text):
    for part in text.split("/"):
        if part:
            ln, ll, polys = part.split(":")
            yield int(ln), int(ll), [int(x) for x in polys.split(",") if x]


def event_times(fn, reps=3):
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


def med_spread(ts):
    med = statistics.median(ts)
    return f"{med:.2f} ms ({(max(ts) - min(ts)) / med * 100:.1f} %)"


def clock():
    rate, mhz, _ = zkp.probe_mad_rate()
    return f"{mhz:.0f} MHz ({rate / 1e12:.2f} T lane-mads/s)"


def make_opener(srs, ln, ll, max_polys, group_log=None):
    if group_log is not None:
        os.environ[KNOB] = str(group_log)
    try:
        return zkp.KzgOpener(srs, ln, ll, max_polys)
    finally:
        os.environ.pop(KNOB, None)


class Batch:
    """the device buffers of a batch of `polys` polynomials of n coefficients each, and the calls that are timed"""

    def __init__(self, ln, ll, polys):
        self.n, self.r, self.polys = 1 << ln, 1 << (ln - ll), polys
        self.coeffs = bench.rand_fr_tensor(torch, self.n * polys, 4, dev)
        self.xy = torch.zeros(polys * self.r * 12, dtype=torch.int64, device=dev)
        self.inf = torch.zeros(polys * self.r, dtype=torch.uint8, device=dev)
        self.ev = torch.zeros(polys * self.n * 4, dtype=torch.int64, device=dev)

    def batch(self, op):
        op.open_cosets_batch_dev(self.coeffs, self.polys, self.n, self.n, self.xy, self.inf, self.ev)

    def sequential(self, op):
        n, r = self.n, self.r
        for p in range(self.polys):
            op.open_cosets_dev(self.coeffs[n * p:n * (p + 1)], n, self.xy[12 * r * p:12 * r * (p + 1)], self.inf[r * p:r * (p + 1)],
                               self.ev[4 * n * p:4 * n * (p + 1)])

    def phases(self, op):
        zkp.profile_reset()
        zkp.profile_enable(1)
        self.batch(op)
        torch.cuda.synchronize()
        out = [zkp.profile_read(name)[0] for name in PHASES]
        zkp.profile_enable(0)
        zkp.profile_reset()
        return out


print(f"shader clock of the multiply-add probe before: {clock()}\n")
if args.shapes:
    print("| log_n | log_l | n_polys | zkp_kzg_open_cosets_batch_dev, median of 3 (spread) | per polynomial | scalars / multiply-accumulate / "
          "transforms (profiled call) | n_polys x zkp_kzg_open_cosets_dev, median of 3 (spread) | sequential / batch |")
    print("|---|---|---|---|---|---|---|---|")
    for ln, ll, counts in shapes_of(args.shapes):
        srs = zkp.G1Bases.from_host(zkp.srs_g1(SECRET, 1 << ln))
        single = make_opener(srs, ln, ll, 1)
        for polys in counts:
            b = Batch(ln, ll, polys)
            op = make_opener(srs, ln, ll, polys)
            ts = event_times(lambda: b.batch(op))
            got = b.xy.clone()
            ph = b.phases(op)
            seq = event_times(lambda: b.sequential(single))
            assert torch.equal(got, b.xy), "the batch and the single calls disagree"
            med = statistics.median(ts)
            print(f"| {ln} | {ll} | {polys} | {med_spread(ts)} | {med / polys:.2f} ms | {ph[0]:.2f} / {ph[1]:.2f} / {ph[2]:.2f} ms | {med_spread(seq)} | "
                  f"{statistics.median(seq) / med:.2f} |", flush=True)
            op.close()
            del b
        single.close()
        srs.close()

if args.groups:
    print("\n| log_n | log_l | n_polys | B | zkp_kzg_open_cosets_batch_dev, median of 3 (spread) | per polynomial | scalars / multiply-accumulate / "
          "transforms (profiled call) | against B = 1 |")
    print("|---|---|---|---|---|---|---|---|")
    for ln, ll, counts in shapes_of(args.groups):
        srs = zkp.G1Bases.from_host(zkp.srs_g1(SECRET, 1 << ln))
        for polys in counts:
            b = Batch(ln, ll, polys)
            base = None
            for group_log in range(3):
                op = make_opener(srs, ln, ll, polys, group_log)
                ts = event_times(lambda: b.batch(op))
                ph = b.phases(op)
                med = statistics.median(ts)
                base = med if base is None else base
                print(f"| {ln} | {ll} | {polys} | {1 << group_log} | {med_spread(ts)} | {med / polys:.2f} ms | {ph[0]:.2f} / {ph[1]:.2f} / {ph[2]:.2f} ms | "
                      f"{med / base:.3f} |", flush=True)
                op.close()
            del b
        srs.close()

print(f"\nshader clock of the multiply-add probe after: {clock()}")
