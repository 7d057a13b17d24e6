"""Compressed G1 points on the device against the validation they are built next to, one process, median of five after a warm-up:
zkp_g1_decompress_dev without and with the subgroup test, zkp_g1_validate_dev on the decoded points (the subgroup chain alone, the
code that was there before), zkp_g1_compress_dev, and the two scalar conversions, at 2^16 / 2^18 / 2^20 points; and the shader clock
of the library's multiply-add probe.  Prints a markdown table (profiles/g1_codec.md).
python tools/g1_codec_bench.py [LOG_N ...]"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "zkp-implementation_amd"))
import torch  # noqa: E402

import bench  # noqa: E402
import zkp_hip as zkp  # noqa: E402

zkp.init()
dev = torch.device("cuda", 0)
sizes = [int(a) for a in sys.argv[1:]] or [16, 18, 20]


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


rate, mhz, _ = zkp.probe_mad_rate()
print(f"shader clock of the multiply-add probe: {mhz:.0f} MHz ({rate / 1e12:.2f} T lane-mads/s)\n")
print("| points | decompress_dev | decompress_dev + subgroup | validate_dev (decoded points) | compress_dev | fr_from_bytes_dev | fr_to_bytes_dev "
      "| us per 2^10 points, decode | decode + subgroup / validate |")
print("|---|---|---|---|---|---|---|---|---|")
for ln in sizes:
    n = 1 << ln
    pts = torch.zeros(n * 12, dtype=torch.int64, device=dev)
    zkp.g1_fixed_base_mul_dev(bench.rand_fr_tensor(torch, n, 1, dev), n, pts)
    enc = torch.zeros(n * 48, dtype=torch.uint8, device=dev)
    zkp.g1_compress_dev(pts, n, enc)
    out = torch.zeros(n * 12, dtype=torch.int64, device=dev)
    inf = torch.zeros(n, dtype=torch.uint8, device=dev)
    rep = zkp.g1_decompress_dev(enc, n, out, inf, check_subgroup=True)
    assert rep["bad"] == 0 and rep["checked"] == n and torch.equal(out, pts) and not inf.any(), rep
    t_dec = median_ms(lambda: zkp.g1_decompress_dev(enc, n, out, inf, check_subgroup=False))
    t_sub = median_ms(lambda: zkp.g1_decompress_dev(enc, n, out, inf, check_subgroup=True))
    t_val = median_ms(lambda: zkp.g1_validate_dev(out, n))
    t_enc = median_ms(lambda: zkp.g1_compress_dev(pts, n, enc))
    fr = bench.rand_fr_tensor(torch, n, 2, dev)
    raw = torch.zeros(n * 32, dtype=torch.uint8, device=dev)
    t_to = median_ms(lambda: zkp.fr_to_bytes_dev(fr, n, raw))
    back = torch.zeros_like(fr)
    assert zkp.fr_from_bytes_dev(raw, n, back) == (0, n) and torch.equal(back, fr)
    t_from = median_ms(lambda: zkp.fr_from_bytes_dev(raw, n, back))
    print(f"| 2^{ln} | {t_dec:.3f} ms | {t_sub:.3f} ms | {t_val:.3f} ms | {t_enc:.3f} ms | {t_from:.3f} ms | {t_to:.3f} ms "
          f"| {t_dec * 1e3 / (n >> 10):.2f} | {t_sub / t_val:.2f} |", flush=True)
    del pts, enc, out, inf, fr, raw, back
