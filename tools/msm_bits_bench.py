"""What a bound on the scalars buys: zkp_msm_g1_bits_dev against zkp_msm_g1_dev, and this build's zkp_msm_g1_dev against the parent
commit's, over n in {2^16, 2^20, 2^22}, bits in {1, 8, 32, 64, 128, 256} and three handles (unexpanded, automatic expansion, split
expansion), the same scalars -- uniform below 2^bits -- for every column.  Writes profiles/msm_short_scalars.md.

    python3 zkp-implementation_amd/build.py -o/tmp/libzkp_hip_parent.so      # in a checkout of the parent commit
    python3 tools/msm_bits_bench.py --parent-lib /tmp/libzkp_hip_parent.so [--logs 16,20,22] [--rounds 3] [--out FILE]

Every library is measured in processes of its own (ZKP_HIP_LIB picks it), the two alternating `rounds` times (the one that goes first
alternates too), one process at a time: the difference between runs of the same library is the run-to-run spread quoted next to every
comparison.  A process warms every
shape up, then times `LOOPS` loops of back-to-back calls with the host clock (the entries return the host result, i.e. after the
stream is drained) and keeps the median loop; the phases and the shader clock msm_accumulate held come from a separate profiled pass."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zkp-implementation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests", "model"))

BITS = (1, 8, 32, 64, 128, 256)
HANDLES = ("unexpanded", "expanded", "split")
LOOPS = 3
PHASES = ("msm_digits", "msm_sort", "msm_accumulate", "msm_bucket_reduce")


def reps_for(log_n):
    return 20 if log_n <= 16 else 10 if log_n <= 20 else 5


# ---------------------------------------------------------------------------------------------------------------- one library, one process
def child(args):
    import torch
    import bench
    import zkp_hip as zkp
    probe = C.CDLL(zkp.LIB_PATH)  # the parent's library lacks the entries this commit adds: bind what it has
    for name in [k for k in zkp._SIGS if not hasattr(probe, k)]:
        del zkp._SIGS[name]
    bounded = "zkp_msm_g1_bits_dev" in zkp._SIGS
    zkp.init()
    dev = torch.device("cuda", 0)
    rows = []

    def timed(call, reps):
        for _ in range(3):
            call()
        loops = []
        for _ in range(LOOPS):
            t0 = time.perf_counter()
            for _ in range(reps):
                call()
            loops.append((time.perf_counter() - t0) / reps * 1e3)
        return {"ms": statistics.median(loops), "lo": min(loops), "hi": max(loops)}

    def setup(log_n):
        n = 1 << log_n
        ks = bench.rand_fr_tensor(torch, n, 1, dev)
        pts = torch.zeros(n * 12, dtype=torch.int64, device=dev)
        zkp.g1_fixed_base_mul_dev(ks, n, pts)
        torch.cuda.synchronize()
        scalars = {}
        for bits in BITS:  # canonical little-endian bytes below 2^bits -> the Fr memory form, on the device
            if bits >= 255:
                scalars[bits] = bench.rand_fr_tensor(torch, n, 100 + bits, dev)
                continue
            g = torch.Generator(device=dev)
            g.manual_seed(100 + bits)
            raw = torch.randint(0, 256, (n, 32), dtype=torch.uint8, device=dev, generator=g)
            full, rest = divmod(bits, 8)
            raw[:, full + (1 if rest else 0):] = 0
            if rest:
                raw[:, full] &= (1 << rest) - 1
            out = torch.zeros(n * 4, dtype=torch.int64, device=dev)
            bad, _ = zkp.fr_from_bytes_dev(raw.contiguous(), n, out, big_endian=False)
            assert bad == 0
            scalars[bits] = out
        return pts, scalars

    def handle(pts, n, hname):
        h = zkp.G1Bases.from_device(pts, n)
        torch.cuda.synchronize()
        if hname != "unexpanded":
            h.precompute(0, glv=hname == "split")
        return h

    def phases(call, reps):
        zkp.profile_reset()
        zkp.profile_enable(True)
        for _ in range(reps):
            call()
        zkp.profile_enable(False)
        cyc, ref, _ = zkp.profile_clock_read("msm_accumulate")
        return {k: zkp.profile_read(k)[0] / reps for k in PHASES}, round(100.0 * cyc / ref) if ref else 0

    # Pass 1, the same sequence of calls whichever library is loaded: the unbounded entry on every row.  Pass 2, this build only: the
    # bounded entry and the profiled calls.  (Interleaved, the bounded and profiled calls of one row would warm the device for the
    # unbounded timing of the next in one library and not in the other.)
    for second in ((False, True) if bounded else (False,)):
        for log_n in args.logs:
            n, reps = 1 << log_n, reps_for(log_n)
            pts, scalars = setup(log_n)
            for hname in HANDLES:
                h = handle(pts, n, hname)
                for bits in BITS:
                    t = scalars[bits]
                    row = {"log_n": log_n, "handle": hname, "bits": bits, "reps": reps, "pass": 2 if second else 1}
                    if not second:
                        row["full"] = timed(lambda: zkp.msm_g1_dev(h, t, n), reps)
                    else:
                        want, got = zkp.msm_g1_dev(h, t, n), zkp.msm_g1_dev(h, t, n, bits=bits)
                        assert got[1] == want[1] and (got[0] == want[0]).all(), (log_n, hname, bits)
                        assert zkp.fr_bit_length_dev(t, n) <= bits
                        row["bits_call"] = timed(lambda: zkp.msm_g1_dev(h, t, n, bits=bits), reps)
                        gf, gb = zkp.selftest_msm_sort_dev(h, [t], n), zkp.selftest_msm_sort_dev(h, [t], n, bits=bits)
                        sets = lambda g: (2 if g["glv"] else 1) * g["nslice"]  # noqa: E731  insertions per scalar at most
                        row["slices"], row["slices_full"], row["c"] = sets(gb), sets(gf), gf["c"]
                        row["phases"], row["acc_mhz"] = phases(lambda: zkp.msm_g1_dev(h, t, n, bits=bits), reps)
                        row["phases_full"], _ = phases(lambda: zkp.msm_g1_dev(h, t, n), reps)
                    rows.append(row)
                    print(json.dumps(row), flush=True)
                del h
            del scalars, pts
            torch.cuda.empty_cache()
    with open(args.json_out, "w") as f:
        json.dump(rows, f)


# ---------------------------------------------------------------------------------------------------------------- the report
def key(r):
    return (r["log_n"], r["handle"], r["bits"])


def report(runs_parent, runs_this, out_path):
    pct = lambda a, b: 100.0 * (a - b) / b  # noqa: E731
    lines = ["# MSM over short scalars: what the bound buys", "",
             f"Written by `tools/msm_bits_bench.py`: {len(runs_parent)} processes over the parent commit's library and "
             f"{len(runs_this)} over this build's, alternating, one at a time on one MI355X.  Times are milliseconds per call: the median of "
             f"{LOOPS} loops of `reps` back-to-back calls after three warm-up calls, host clock around entries that return the host result.  "
             "Scalars are uniform below 2^bits, the same tensors for every column.  A process times the unbounded entry on every row first -- "
             "the same sequence of calls for both libraries -- and, this build only, the bounded entry and the profiled calls afterwards.  "
             "`spread` is the largest difference between runs of the same library and entry on that row (max - min over the processes, in "
             "percent of the median): a difference below it is not a difference.", ""]
    def merged(run):  # a row's two passes under one key
        out = {}
        for r in run:
            out.setdefault(key(r), {}).update(r)
        return out
    by_p = [merged(run) for run in runs_parent]
    by_t = [merged(run) for run in runs_this]
    med = lambda runs, k, col: statistics.median(run[k][col]["ms"] for run in runs)  # noqa: E731
    rng = lambda runs, k, col: (max(run[k][col]["ms"] for run in runs) - min(run[k][col]["ms"] for run in runs)) / med(runs, k, col) * 100  # noqa: E731
    lines += ["| n | handle | c | bits | slices t/T | parent full | this full | diff % | spread % | bounded | bounded / full | spread % | "
              "digits | sort | accumulate | reduce | acc MHz | accumulate, full |", "|" + "---|" * 18]
    moved, slower, at256, diffs, noise = [], [], [], [], []
    for k in sorted(by_t[0], key=lambda k: (k[0], HANDLES.index(k[1]), k[2])):
        r = by_t[-1][k]
        pf, tf, tb = med(by_p, k, "full"), med(by_t, k, "full"), med(by_t, k, "bits_call")
        spread, spread_b = max(rng(by_p, k, "full"), rng(by_t, k, "full")), max(rng(by_t, k, "full"), rng(by_t, k, "bits_call"))
        d = pct(tf, pf)
        diffs.append(d)
        noise += [rng(by_p, k, "full"), rng(by_t, k, "full")]
        if abs(d) > spread:
            moved.append((k, d, spread))
        if tb > tf and pct(tb, tf) > spread_b:
            slower.append((k, pct(tb, tf), spread_b))
        if k[2] == 256:
            at256.append((k, pct(tb, tf), spread_b))
        ph = r["phases"]
        lines.append(f"| 2^{k[0]} | {k[1]} | {r['c']} | {k[2]} | {r['slices']}/{r['slices_full']} = {r['slices'] / r['slices_full']:.2f} | {pf:.3f} | {tf:.3f} | "
                     f"{d:+.1f} | {spread:.1f} | {tb:.3f} | {tb / tf:.2f} | {spread_b:.1f} | {ph['msm_digits']:.3f} | {ph['msm_sort']:.3f} | "
                     f"{ph['msm_accumulate']:.3f} | {ph['msm_bucket_reduce']:.3f} | {r['acc_mhz']} | {r['phases_full']['msm_accumulate']:.3f} |")
    q = lambda v, f: sorted(v)[min(len(v) - 1, int(f * len(v)))]  # noqa: E731
    lines += ["", "The phase columns are the bounded call's, from profiled calls of their own (event markers add a few microseconds each); "
              "`acc MHz` is the shader clock msm_accumulate held there (in-kernel stamps); the last column is msm_accumulate of the unbounded "
              "call on the same scalars.", "",
              "## The two conditions", "",
              f"- Over all {len(diffs)} rows this build's `zkp_msm_g1_dev` differs from the parent's by {statistics.median(diffs):+.2f} % in the median "
              f"({min(diffs):+.1f} % to {max(diffs):+.1f} %); two runs of the SAME library differ by {statistics.median(noise):.2f} % in the median, "
              f"{q(noise, 0.9):.1f} % at the 90th percentile and {max(noise):.1f} % at most.",
              f"- Row by row, {len(moved)} of {len(by_t[0])} rows differ by more than that row's own spread"
              + ("." if not moved else ": " + "; ".join(f"2^{k[0]} {k[1]} bits {k[2]}: {d:+.1f} % (spread {s:.1f} %)" for k, d, s in moved) + "."),
              "- `zkp_msm_g1_bits_dev` at bits = 256 against this build's `zkp_msm_g1_dev`: "
              + "; ".join(f"2^{k[0]} {k[1]}: {d:+.1f} % (spread {s:.1f} %)" for k, d, s in at256) + ".", "",
              "## Rows where the bounded call is slower than the full-width one by more than the spread", ""]
    lines += [f"- 2^{k[0]} {k[1]} bits {k[2]}: {d:+.1f} % (spread {s:.1f} %)" for k, d, s in slower] or ["None."]
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--logs", default="16,20,22")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "msm_short_scalars.md"))
    ap.add_argument("--scratch", help="where the processes leave their rows and logs (default: a temporary directory)")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--json-out")
    args = ap.parse_args()
    args.logs = [int(x) for x in str(args.logs).split(",")]
    if args.child:
        return child(args)
    if not args.parent_lib or not os.path.exists(args.parent_lib):
        sys.exit("--parent-lib: the library built from the parent commit (see the head of this file)")
    if not args.scratch:
        args.scratch = tempfile.mkdtemp(prefix="msm_bits_bench_")
    os.makedirs(args.scratch, exist_ok=True)
    runs = {"parent": [], "this": []}
    for rnd in range(args.rounds):
        for which in (("parent", "this") if rnd % 2 == 0 else ("this", "parent")):  # a fresh process per library and round, one at a time
            env = dict(os.environ)
            env.pop("ZKP_HIP_LIB", None)
            if which == "parent":
                env["ZKP_HIP_LIB"] = os.path.abspath(args.parent_lib)
            path = os.path.join(args.scratch, f"msm_bits_{which}_{rnd}.json")
            log = open(os.path.join(args.scratch, f"msm_bits_{which}_{rnd}.log"), "w")
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--json-out", path, "--logs", ",".join(map(str, args.logs))],
                               env=env, stdout=log, stderr=subprocess.STDOUT, timeout=900)
            log.close()
            if p.returncode != 0:  # nothing more is started on the device after a process that failed
                sys.exit(f"{which} round {rnd}: exit {p.returncode}, see {log.name}")
            runs[which].append(json.load(open(path)))
            print(f"{which} round {rnd}: {len(runs[which][-1])} rows", flush=True)
    report(runs["parent"], runs["this"], args.out)


if __name__ == "__main__":
    main()
