"""Worker of tests/test_gpu_g1_validate.py (own process: the device slots are set before the library starts).
python tests/g1_validate_worker.py   -- two slots on GPU 0, a sharded handle of 130 points with one point outside G1 at index 100
Prints OK g1_validate slots."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zkp-implementation_amd"), os.path.join(ROOT, "tests", "model")):
    sys.path.insert(0, p)
import torch  # noqa: E402,F401

import bigmodel as bm  # noqa: E402
import zkp_hip as zkp  # noqa: E402
from oracle import oracle as orc  # noqa: E402

orc.build()
zkp.init_devices([0, 0])
assert zkp.device_count() == 2
n = 130
ks = orc.rand_fr(0x61CB, n)
ks[17] = 0  # an infinity base in the first chunk
pts, inf = orc.g1_fixed_base_mul(ks)
h = zkp.G1Bases.from_host(pts, inf)
assert [(off, ln) for (_, _, off, ln) in h.shards()] == [(0, 65), (65, 65)]
rep, status = h.validate(want_status=True)
assert rep == dict(checked=n, bad=0, non_canonical=0, off_curve=0, outside_subgroup=0, first_bad=n, first_status=0), rep
assert not status.any()

q = (4, pow(4 ** 3 + 4, (bm.P + 1) // 4, bm.P))  # on the curve, outside G1
assert bm.g1_on_curve(q)
bad = pts.copy()
bad[100] = orc.points_from_ints([q])[0][0]
for expand in (None, False, True):
    h = zkp.G1Bases.from_host(bad, inf)
    assert len(h.shards()) == 2
    if expand is not None:
        h.precompute(12, glv=expand)
    rep, status = h.validate(want_status=True)
    assert rep == dict(checked=n, bad=1, non_canonical=0, off_curve=0, outside_subgroup=1, first_bad=100, first_status=3), (expand, rep)
    assert status[100] == 3 and status.sum() == 3
bad[30] = bad[100]  # one in each chunk: the lowest index wins, the counters add up
rep = zkp.G1Bases.from_host(bad, inf).validate()
assert rep["bad"] == 2 and rep["outside_subgroup"] == 2 and rep["first_bad"] == 30 and rep["first_status"] == 3, rep
print("OK g1_validate slots")
