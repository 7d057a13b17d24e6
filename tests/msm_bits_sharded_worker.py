"""Worker of tests/test_gpu_msm_bits.py (own process: it initialises the library with two device slots, which share GPU 0 when the box
has one): the bounded MSM entries refuse a handle sharded over several slots, and the unbounded entry still serves it.  Prints OK."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zkp-implementation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import zkp_hip as zkp  # noqa: E402
from oracle import oracle as orc  # noqa: E402

ngpu = torch.cuda.device_count()
zkp.init_devices([i % ngpu for i in range(2)])
assert zkp.device_count() == 2
n = 256
xy = zkp.srs_g1(orc.fr_from_ints([0x1F2E3D4C5B6A7988])[0], n)
sharded = zkp.G1Bases.from_host(xy)  # default thread slot: sharded over both slots
assert len(sharded.shards()) == 2
sc = orc.fr_from_ints(list(range(1, n + 1)))
want = zkp.msm_g1(sharded, sc)
for bits in (9, 64, 128, 254):
    try:
        zkp.msm_g1(sharded, sc, bits=bits)
        raise SystemExit(f"bits={bits}: a sharded handle was accepted")
    except zkp.ZkpError as e:
        assert e.code == zkp.ZKP_E_ARG and "sharded" in str(e), e
t = torch.from_numpy(sc.view(np.int64)).to("cuda:0")
for call in (lambda: zkp.msm_g1_dev(sharded, t, n, bits=64), lambda: zkp.msm_g1_batch_dev(sharded, [t], n, bits=64),
             lambda: zkp.selftest_msm_sort_dev(sharded, [t], n, bits=64)):
    try:
        call()
        raise SystemExit("a device-pointer entry accepted a sharded handle")
    except zkp.ZkpError as e:
        assert e.code == zkp.ZKP_E_ARG and "sharded" in str(e), e
got = zkp.msm_g1(sharded, sc)  # the handle still serves the unbounded entry
assert got[1] == want[1] and np.array_equal(got[0], want[0])
zkp.set_device(0)
single = zkp.G1Bases.from_host(xy)  # one slot: the bounded entry takes it and agrees
assert len(single.shards()) == 1
got = zkp.msm_g1(single, sc, bits=9)
assert got[1] == want[1] and np.array_equal(got[0], want[0])
print("OK sharded refusal")
