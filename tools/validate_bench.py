"""G1 validation against the SRS expansions it is meant to precede, one process, median of five after a warm-up:
zkp_g1_validate_dev, zkp_g1_bases_validate, zkp_g1_bases_precompute and ..._glv (automatic width) on the same 2^16 / 2^20 / 2^22 points,
zkp_srs_check at 2^20, and the shader clock of the library's multiply-add probe.  Prints a markdown table (profiles/g1_validate.md).
python tools/validate_bench.py [LOG_N ...]"""
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

zkp.init()
dev = torch.device("cuda", 0)
sizes = [int(a) for a in sys.argv[1:]] or [16, 20, 22]


def median_ms(fn, reps=5):
    fn()  # warm-up
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(out)


def expansion_ms(pts, n, glv, reps=5):
    """precompute alone: the handle (upload + conversion) is made outside the timed region, a fresh one per repetition"""
    out = []
    for i in range(reps + 1):
        h = zkp.G1Bases.from_device(pts, n)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        h.precompute(0, glv=glv)
        out.append((time.perf_counter() - t0) * 1e3)
        h.close()
    return statistics.median(out[1:])


rate, mhz, _ = zkp.probe_mad_rate()
print(f"shader clock of the multiply-add probe: {mhz:.0f} MHz ({rate / 1e12:.2f} T lane-mads/s)\n")
print("| points | validate_dev (raw) | bases_validate (handle) | precompute | precompute_glv | us per 2^10 points, raw |")
print("|---|---|---|---|---|---|")
for ln in sizes:
    n = 1 << ln
    pts = torch.zeros(n * 12, dtype=torch.int64, device=dev)
    zkp.g1_fixed_base_mul_dev(bench.rand_fr_tensor(torch, n, 1, dev), n, pts)
    torch.cuda.synchronize()
    rep = zkp.g1_validate_dev(pts, n)
    assert rep["bad"] == 0 and rep["checked"] == n, rep
    t_raw = median_ms(lambda: zkp.g1_validate_dev(pts, n))
    h = zkp.G1Bases.from_device(pts, n)
    t_int = median_ms(lambda: h.validate())
    h.close()
    t_plain, t_glv = expansion_ms(pts, n, False), expansion_ms(pts, n, True)
    print(f"| 2^{ln} | {t_raw:.2f} ms | {t_int:.2f} ms | {t_plain:.2f} ms | {t_glv:.2f} ms | {t_raw * 1e3 / (n >> 10):.2f} |", flush=True)
    del pts

if 20 in sizes:
    n = 1 << 20
    secret = bench.fr_mont([0x1F2E3D4C5B6A7988])[0]
    srs = zkp.G1Bases.from_host(zkp.srs_g1(secret, n))
    g2s, _ = zkp.g2_mul(zkp.g2_generator(), secret)
    r = bench.rand_fr_tensor(torch, n - 1, 7, dev).cpu().numpy().view(np.uint64)
    for what, prep in (("plain handle", lambda: None), ("precompute(0)", lambda: srs.precompute(0))):
        prep()
        assert zkp.srs_check(srs, g2s, n, r) == 1
        print(f"\nzkp_srs_check at 2^20, {what}: {median_ms(lambda: zkp.srs_check(srs, g2s, n, r)):.1f} ms")
