"""Worker of tests/test_gpu_g1_ntt.py (own process: the device slots are set before the library starts).
python tests/g1_ntt_worker.py   -- two slots on GPU 0; a sharded SRS handle is refused by zkp_g1_bases_lagrange and
zkp_kzg_opener_create with ZKP_E_ARG, and a handle made on one slot afterwards works.  Prints OK g1_ntt slots."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zkp-implementation_amd"), os.path.join(ROOT, "tests", "model")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401

import zkp_hip as zkp  # noqa: E402
from oracle import oracle as orc  # noqa: E402

orc.build()
zkp.init_devices([0, 0])
assert zkp.device_count() == 2
n, secret = 8, 0x1F2E3D4C5B6A7988
xy = zkp.srs_g1(orc.fr_from_ints([secret])[0], n)
sharded = zkp.G1Bases.from_host(xy)
assert len(sharded.shards()) == 2
for call in (lambda: sharded.lagrange(3), lambda: zkp.KzgOpener(sharded, 3)):
    try:
        call()
    except zkp.ZkpError as e:
        assert e.code == zkp.ZKP_E_ARG and "sharded" in str(e), e
    else:
        raise AssertionError("a sharded source was accepted")

zkp.set_device(1)
single = zkp.G1Bases.from_host(xy)
assert [s[0] for s in single.shards()] == [1]
lag = single.lagrange(3)  # [L_i(s)]G: its MSM with the evaluations of f commits to f
coeffs = orc.rand_fr(0x61F0, n)
got, exp = zkp.kzg_commit(lag, orc.ntt_fr(coeffs)), zkp.kzg_commit(single, coeffs)
assert got[1] == exp[1] == 0 and np.array_equal(got[0], exp[0])
(proofs, inf), ev = zkp.KzgOpener(single, 3).open_all(coeffs)
w = orc.fr_root_of_unity(3)
(p1, i1), e1 = zkp.kzg_open(single, coeffs, w)
assert i1 == inf[1] and np.array_equal(p1, proofs[1]) and np.array_equal(e1, ev[1])
print("OK g1_ntt slots")
