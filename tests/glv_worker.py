"""Worker of tests/test_gpu_glv.py (own process: the knob or the device slots are set before the library starts).
python tests/glv_worker.py ranges   -- ZKP_MSM_RANGE_LOG=10 comes with the environment: 4096 scalars in four ranges over split planes
python tests/glv_worker.py slots    -- two slots on GPU 0, a sharded split handle
Prints OK glv <mode>."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zkp-implementation_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402

import zkp_hip as zkp  # noqa: E402
from oracle import oracle as orc  # noqa: E402

LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF
mode = sys.argv[1]
orc.build()


def case(n, seed):
    ks = orc.rand_fr(0x61C0 + seed, n)
    ks[min(17, n - 1)] = 0  # an infinity base
    pts, inf = orc.g1_fixed_base_mul(ks)
    sc = orc.rand_fr(0x61D0 + seed, n)
    sc[:4] = orc.fr_from_ints([LAMBDA, LAMBDA + 1, orc.R_MOD - 1, 0])
    sc[40:90] = sc[39]  # a crowded bucket in every slice
    return pts, inf, sc, orc.msm_naive(pts, inf, sc)


if mode == "ranges":
    assert os.environ.get("ZKP_MSM_RANGE_LOG") == "10"
    zkp.init()
    n = 4096
    pts, inf, sc, (exp, einf) = case(n, 1)
    split = zkp.G1Bases.from_host(pts, inf).precompute(16, glv=True)
    plain = zkp.G1Bases.from_host(pts, inf).precompute(16)
    d_sc = torch.from_numpy(sc.view(np.int64)).cuda()
    for h in (split, plain):
        for got in (zkp.msm_g1_dev(h, d_sc, n), zkp.msm_g1(h, sc)):  # resident scalars; host scalars
            assert got[1] == einf and np.array_equal(got[0], exp), (h is split, got)
    # an uneven walk: the last range is shorter than the others
    m = n - 1023
    expm = orc.msm_naive(pts[:m], inf[:m], sc[:m])
    for h in (split, plain):
        got = zkp.msm_g1_dev(h, d_sc, m)
        assert got[1] == expm[1] and np.array_equal(got[0], expm[0])
elif mode == "slots":
    zkp.init_devices([0, 0])
    assert zkp.device_count() == 2
    n = 300
    pts, inf, sc, (exp, einf) = case(n, 2)
    sharded = zkp.G1Bases.from_host(pts, inf)
    assert len(sharded.shards()) == 2
    sharded.precompute(12, glv=True)
    e = sharded.expansion()
    assert (e["glv"], e["planes"], e["slices"], e["bytes"]) == (1, 11, 22, 128 * 11 * n), e
    try:
        sharded.precompute(12)
        raise SystemExit("a split handle was expanded again the other way")
    except zkp.ZkpError as err:
        assert err.code == zkp.ZKP_E_ARG
    got = zkp.msm_g1(sharded, sc)
    assert got[1] == einf and np.array_equal(got[0], exp)
    chunks = sharded.shards()
    resident = [torch.from_numpy(sc[off:off + ln].copy().view(np.int64)).cuda() for (_, _, off, ln) in chunks]
    torch.cuda.synchronize()
    got = zkp.msm_g1_sharded_dev(sharded, resident, n)
    assert got[1] == einf and np.array_equal(got[0], exp)
else:
    raise SystemExit("unknown mode")
print("OK glv", mode)
