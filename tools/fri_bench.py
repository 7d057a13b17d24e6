"""FRI generate_proof timing: python3 tools/fri_bench.py [LOG_D_COEFFS] [BLOWUP] [QUERIES] [--field gl|fr]
(default Goldilocks; for either field: best / median of five warm calls with profiling off, one profiled call with its phases,
the SHA-256 of the proof words, verify, and the 2^(LOG_D+1)-leaf Merkle tree)"""
import hashlib
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "zkp-implementation_amd"))
import numpy as np
import torch
import zkp_hip as zkp

field = "gl"
if "--field" in sys.argv:
    i = sys.argv.index("--field")
    field = sys.argv[i + 1]
    del sys.argv[i:i + 2]
ld = int(sys.argv[1]) if len(sys.argv) > 1 else 20
blow = int(sys.argv[2]) if len(sys.argv) > 2 else 2
nq = int(sys.argv[3]) if len(sys.argv) > 3 else 32
zkp.init()

rnd = np.random.default_rng(1)
if field == "fr":
    W, suffix, prove, verify, tree = 4, "_fr", zkp.fri_prove_fr, zkp.fri_verify_fr, zkp.fri_merkle_tree_fr_dev
    phases = ("fri_merkle", "ntt_fr_pass", "fri_fold", "fri_transcript", "fri_tail", "fri_gather")
    coeffs = rnd.integers(0, 2 ** 63, (1 << ld, 4), dtype=np.uint64)
    coeffs[:, 3] %= np.uint64(0x73eda753299d7d48)  # < r
    leaves = rnd.integers(0, 2 ** 63, (1 << (ld + 1), 4), dtype=np.uint64) >> np.uint64(2)
else:
    W, suffix, prove, verify, tree = 1, "", zkp.fri_prove, zkp.fri_verify, zkp.fri_merkle_tree_dev
    phases = ("fri_merkle", "ntt_gl_pass")  # the driver's own phases are not recorded for this field
    coeffs = rnd.integers(1, 2 ** 63, 1 << ld, dtype=np.uint64)
    leaves = rnd.integers(0, 2 ** 62, 1 << (ld + 1), dtype=np.uint64)

prove(coeffs, blow, nq)  # warm-up
times = []
for rep in range(6):
    zkp.profile_reset()
    zkp.profile_enable(rep == 5)
    t0 = time.perf_counter()
    proof = prove(coeffs, blow, nq)
    times.append(time.perf_counter() - t0)
    zkp.profile_enable(False)
ph = {k: zkp.profile_read(k) for k in phases}
_, mhz, _ = zkp.probe_mad_rate(5)  # shader clock right after the timed calls
warm = sorted(times[:5])
print(f"fri_prove{suffix} 2^{ld} coeffs x{blow} q{nq}: best {warm[0] * 1e3:.2f} ms, median {warm[2] * 1e3:.2f} ms (5 warm calls), "
      f"profiled call {times[5] * 1e3:.2f} ms, proof {proof.size * 8 / 1024:.1f} KiB, clock {mhz:.0f} MHz, phases (ms, records) {ph}")
print(f"proof{suffix} sha256 {hashlib.sha256(np.ascontiguousarray(proof).tobytes()).hexdigest()}")
t0 = time.perf_counter()
ok = verify(proof)
print(f"verify{suffix}", ok, f"{(time.perf_counter() - t0) * 1e3:.2f} ms")
n = 1 << (ld + 1)
d_leaves = torch.from_numpy(np.ascontiguousarray(leaves).view(np.int64)).cuda()
d_nodes = torch.zeros(zkp.fri_merkle_node_count(n) * W, dtype=torch.int64, device="cuda")
for _ in range(2):
    tree(d_leaves, n, d_nodes)
torch.cuda.synchronize()
ts = []
for _ in range(5):
    t0 = time.perf_counter()
    tree(d_leaves, n, d_nodes)
    torch.cuda.synchronize()
    ts.append(time.perf_counter() - t0)
ts.sort()
print(f"merkle tree{suffix} 2^{ld + 1} leaves: best {ts[0] * 1e3:.3f} ms, median {ts[2] * 1e3:.3f} ms = "
      f"{(2 * n - 1) / ts[0] / 1e9:.3f} G hashes/s")
