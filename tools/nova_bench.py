#!/usr/bin/env python3
"""Per-stage times of one Nova folding step (NIFS::prover + NIFS::prove) on a synthetic sparse R1CS, measured with HIP events.

R1CS: rows = num_vars = 2^k, about one entry per row in each of A, B, C (~3 per row) and a few rows of 1024 entries in A; the SRS
is expanded (KzgScheme).  Stages: cross term (zkp_nova_cross_term_dev), com_T (the MSM over T, zkp_msm_g1_dev), fold
(zkp_nova_fold_witness_dev), the two openings (zkp_nova_nifs_prove_dev, transcript included), and the whole prover + prove.  Each
stage: median of --reps timed runs after --warmup.  Also prints the shader clock the v_mad_u64_u32 probe held right after the
runs (zkp_probe_mad_rate), since the chip's clock under load differs from box to box.  Prints one JSON line.

    python tools/nova_bench.py [--log-rows 16,20,22] [--reps 5] [--warmup 2]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zkp-implementation_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def synthetic_r1cs(orc, rows, nv, nio, seed):
    rng = np.random.default_rng(seed)
    mats = []
    for k in range(3):
        lens = np.ones(rows, dtype=np.int64)
        if k == 0:
            lens[rng.choice(rows, 16, replace=False)] = 1024
        rp = np.zeros(rows + 1, dtype=np.uint64)
        rp[1:] = np.cumsum(lens)
        nnz = int(rp[-1])
        mats.append((rp, rng.integers(0, nv + nio + 1, nnz).astype(np.uint32), orc.rand_fr(seed * 3 + k, nnz)))
    return mats


def timed(torch, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return round(statistics.median(out), 3)


def bench_size(zkp, orc, torch, log_rows, reps, warmup):
    rows = nv = 1 << log_rows
    nio = 2
    mats = synthetic_r1cs(orc, rows, nv, nio, log_rows)
    secret = orc.rand_fr(7, 1)[0]
    scheme = zkp.KzgScheme(zkp.Srs.new_from_secret(secret, rows))
    r1cs = zkp.NovaR1CS(scheme, rows, nv, nio, *mats)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()
    fw = [zkp.FWitness(dev(orc.rand_fr(10 + k, rows)), dev(orc.rand_fr(20 + k, nv))) for k in range(2)]
    fi = [f.commit(scheme, orc.rand_fr(30 + k, nio)) for k, f in enumerate(fw)]
    t = torch.zeros(rows * 4, dtype=torch.int64, device="cuda")
    e_out, w_out = torch.empty_like(fw[0].e), torch.empty_like(fw[0].w)
    r = orc.rand_fr(40, 1)[0]
    bases = scheme.srs.bases
    res = {"rows": rows, "nnz": int(sum(int(m[0][-1]) for m in mats))}
    res["cross_term_ms"] = timed(torch, lambda: r1cs.cross_term_dev(fw[0].w, fi[0].x, fi[0].u, fw[1].w, fi[1].x, fi[1].u, t), reps, warmup)
    res["com_t_msm_ms"] = timed(torch, lambda: zkp.msm_g1_dev(bases, t, rows), reps, warmup)
    res["fold_ms"] = timed(torch, lambda: r1cs.fold_witness_dev(r, fw[0].e, fw[0].w, fw[1].e, fw[1].w, t, e_out, w_out), reps, warmup)
    fwo = zkp.FWitness(e_out, w_out)

    def openings():
        tr = zkp.NovaTranscript()
        tr.feed_scalar_num(r)
        zkp.nifs_prove(r1cs, r, fwo, fi[0], tr)
    res["openings_ms"] = timed(torch, openings, reps, warmup)

    def step():
        tr = zkp.NovaTranscript()
        w3, i3, _ct, rr = zkp.nifs_prover(r1cs, fw[0], fw[1], fi[0], fi[1], tr)
        zkp.nifs_prove(r1cs, rr, w3, i3, tr)
    res["prover_plus_prove_ms"] = timed(torch, step, reps, warmup)
    msm3 = res["com_t_msm_ms"] * 3
    res["three_msm_share_est"] = round(msm3 / res["prover_plus_prove_ms"], 3)  # com_T + 2 openings ~ three MSMs of n terms
    r1cs.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-rows", default="16,20,22")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("nova_bench needs a GPU")
    import zkp_hip as zkp
    from oracle import oracle as orc
    orc.build()
    zkp.init(0)
    out = {"bench": "nova_fold_step", "sizes": []}
    for lr in (int(v) for v in a.log_rows.split(",")):
        out["sizes"].append(bench_size(zkp, orc, torch, lr, a.reps, a.warmup))
    _rate, mhz, _ms = zkp.probe_mad_rate(20)
    out["clock_mhz_probe"] = round(mhz, 1)
    out["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
