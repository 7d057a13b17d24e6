"""Worker of tests/test_gpu_kzg_recover_batch.py (own process: the device slots are set before the library starts).
python tests/kzg_recover_batch_worker.py   -- two slots on GPU 0; a recoverer for a batch made after zkp_set_device(1) lives on slot 1
and recovers a batch through both entries, in both layouts, while the thread has gone back to slot 0.  Prints OK kzg recover batch
slots."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zkp-implementation_amd"), os.path.join(ROOT, "tests", "model")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import zkp_hip as zkp  # noqa: E402
from oracle import oracle as orc  # noqa: E402

orc.build()
zkp.init_devices([0, 0])
assert zkp.device_count() == 2
log_n, log_l = 6, 2
n, l, r = 64, 4, 16
polys, length = 3, 29
zkp.set_device(1)
rc = zkp.KzgRecoverer(log_n, log_l, polys)
zkp.set_device(0)
f = orc.rand_fr(0x79F8, polys * length).reshape(polys, length, 4)
ev = np.zeros((polys, n, 4), dtype=np.uint64)
for p in range(polys):
    padded = np.zeros((n, 4), dtype=np.uint64)
    padded[:length] = f[p]
    ev[p] = orc.ntt_fr(padded)
present = np.ones(r, dtype=np.uint8)
present[[1, 2, 3, 5, 8, 13, 15]] = 0
sent = ev.copy()
sent[:, np.tile(present == 0, n // r)] = np.uint64(0xFFFFFFFFFFFFFFFF)
cells = lambda a: np.ascontiguousarray(a.reshape(polys, l, r, 4).transpose(0, 2, 1, 3))  # noqa: E731
coeffs, out_ev, ok = rc.recover_batch(cells(sent), present, length, want_evals=True, cells=True)
assert ok.all() and np.array_equal(coeffs, f) and np.array_equal(out_ev, cells(ev))
d_out = torch.zeros(polys * length * 4, dtype=torch.int64, device="cuda")
d_flags = torch.full((polys,), 7, dtype=torch.int32, device="cuda")
rc.recover_batch_dev(torch.from_numpy(sent.view(np.int64)).cuda(), polys, present, length, length, d_out, d_flags)
torch.cuda.synchronize()
assert d_flags.cpu().tolist() == [0] * polys and np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(polys, length, 4), f)
rc.close()
print("OK kzg recover batch slots")
