"""Worker of tests/test_gpu_kzg_open_evals.py (own process: the device slots are set before the library starts).
python tests/kzg_open_evals_worker.py   -- two slots on GPU 0; a sharded bases handle is refused by zkp_kzg_eval_opener_create with
ZKP_E_ARG, and an opener made over a Lagrange basis on the second slot afterwards works there.  Prints OK kzg open evals slots."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zkp-implementation_amd"), os.path.join(ROOT, "tests", "model")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401

import zkp_hip as zkp  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from zkp_hip import kzg_evals  # noqa: E402

orc.build()
zkp.init_devices([0, 0])
assert zkp.device_count() == 2
log_n, n, secret = 3, 8, 0x1F2E3D4C5B6A7988
xy = zkp.srs_g1(orc.fr_from_ints([secret])[0], n)
sharded = zkp.G1Bases.from_host(xy)
assert len(sharded.shards()) == 2
try:
    kzg_evals.KzgEvalOpener(sharded, log_n, 2)
except zkp.ZkpError as e:
    assert e.code == zkp.ZKP_E_ARG and "sharded" in str(e), e
else:
    raise AssertionError("a sharded handle was accepted")

zkp.set_device(1)
mono = zkp.G1Bases.from_host(xy)
assert [s[0] for s in mono.shards()] == [1]
lag = mono.lagrange(log_n)
assert [s[0] for s in lag.shards()] == [1]
rows = orc.rand_fr(0x82F0, 2 * n).reshape(2, n, 4)
zs = orc.rand_fr(0x82F1, 2)
zkp.set_device(0)  # the opener lives on the slot of its bases, whatever the calling thread's
op = kzg_evals.KzgEvalOpener(lag, log_n, 2)
(pxy, pinf), y = op.open_batch(rows, zs)
cxy, cinf = op.commit_batch(rows)
for p in range(2):
    coeffs = orc.ntt_fr(rows[p], inverse=True)
    (exy, einf), ev = zkp.kzg_open(mono, coeffs, zs[p])
    assert pxy[p].tobytes() == exy.tobytes() and pinf[p] == einf and np.array_equal(y[p], ev), p
    ecxy, ecinf = zkp.kzg_commit(mono, coeffs)
    assert cxy[p].tobytes() == ecxy.tobytes() and cinf[p] == ecinf, p
op.close()
print("OK kzg open evals slots")
