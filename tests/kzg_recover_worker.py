"""Worker of tests/test_gpu_kzg_recover.py (own process: the device slots are set before the library starts).
python tests/kzg_recover_worker.py   -- two slots on GPU 0; a recoverer made after zkp_set_device(1) lives on slot 1 and recovers
through both entries while the thread has gone back to slot 0.  Prints OK kzg recover slots."""
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
n, r = 64, 16
zkp.set_device(1)
rc = zkp.KzgRecoverer(log_n, log_l)
zkp.set_device(0)
length = 29
f = orc.rand_fr(0x79F0, length)
padded = np.zeros((n, 4), dtype=np.uint64)
padded[:length] = f
ev = orc.ntt_fr(padded)
present = np.ones(r, dtype=np.uint8)
present[[1, 2, 3, 5, 8, 13, 15]] = 0
sent = ev.copy()
sent[np.tile(present == 0, n // r)] = np.uint64(0xFFFFFFFFFFFFFFFF)
coeffs, out_ev, ok = rc.recover(sent, present, length, want_evals=True)
assert ok and np.array_equal(coeffs, f) and np.array_equal(out_ev, ev)
d_out = torch.zeros(length * 4, dtype=torch.int64, device="cuda")
d_flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
rc.recover_dev(torch.from_numpy(sent.view(np.int64)).cuda(), present, length, d_out, d_flag)
torch.cuda.synchronize()
assert int(d_flag.item()) == 0 and np.array_equal(d_out.cpu().numpy().view(np.uint64).reshape(length, 4), f)
rc.close()
print("OK kzg recover slots")
