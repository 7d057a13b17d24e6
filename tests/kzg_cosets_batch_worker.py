"""Worker of tests/test_gpu_kzg_cosets_batch.py (own process: the device slots are set before the library starts).
python tests/kzg_cosets_batch_worker.py   -- two slots on GPU 0; a sharded SRS handle is refused by zkp_kzg_opener_create_cosets_batch
with ZKP_E_ARG, and a batch opener made from a handle on the second slot afterwards works.  Prints OK kzg cosets batch slots."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zkp-implementation_amd"), os.path.join(ROOT, "tests", "model")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401

import g1_coset_model as cm  # noqa: E402
import zkp_hip as zkp  # noqa: E402
from oracle import oracle as orc  # noqa: E402

orc.build()
zkp.init_devices([0, 0])
assert zkp.device_count() == 2
n, l, secret = 8, 2, 0x1F2E3D4C5B6A7988
xy = zkp.srs_g1(orc.fr_from_ints([secret])[0], n)
sharded = zkp.G1Bases.from_host(xy)
assert len(sharded.shards()) == 2
try:
    zkp.KzgOpener(sharded, 3, 1, 2)
except zkp.ZkpError as e:
    assert e.code == zkp.ZKP_E_ARG and "sharded" in str(e), e
else:
    raise AssertionError("a sharded source was accepted")

zkp.set_device(1)
single = zkp.G1Bases.from_host(xy)
assert [s[0] for s in single.shards()] == [1]
rows = [orc.fr_to_ints(orc.rand_fr(0x82F0 + p, n)) for p in range(2)]
(proofs, inf), _ = zkp.KzgOpener(single, 3, 1, 2).open_cosets_batch(np.stack([orc.fr_from_ints(f) for f in rows]))
for p, f in enumerate(rows):
    for k in range(n // l):
        got = zkp.kzg_commit(single, orc.fr_from_ints(cm.quotient(f, n, l, k)))
        assert got[1] == inf[p][k] == 0 and np.array_equal(got[0], proofs[p][k]), (p, k)
print("OK kzg cosets batch slots")
