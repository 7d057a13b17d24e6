"""The host pairing check through the x-chain final exponentiation of csrc/pairing_tower.hpp (ZKP_PAIRING_FINAL_EXP=chain, the
default) and through the plain 4314-bit power (=plain): the verdicts of the cases of tests/test_pairing_cpu.py, restated, are the
same under both, and zkp_pairing's value -- pinned bit for bit to the plain model -- does not depend on the knob.  CPU only."""
import os

import numpy as np
import pytest

import bigmodel as M
import pairing_model as PM

P, R = M.P, M.R
KNOB = "ZKP_PAIRING_FINAL_EXP"
RQ_INV = pow(2 ** 384, -1, P)


@pytest.fixture(scope="module")
def zkp():
    import zkp_hip
    zkp_hip.lib()
    return zkp_hip


@pytest.fixture(params=["chain", "plain", None, "nonsense"])
def mode(request):
    old = os.environ.pop(KNOB, None)
    if request.param is not None:
        os.environ[KNOB] = request.param
    yield request.param
    os.environ.pop(KNOB, None)
    if old is not None:
        os.environ[KNOB] = old


def g2_from_ints(pt):
    out = np.zeros(24, dtype=np.uint64)
    for i, v in enumerate([pt[0][0], pt[0][1], pt[1][0], pt[1][1]]):
        out[6 * i:6 * i + 6] = M.to_limbs(v * 2 ** 384 % P, 6)
    return out


def fq_canon(limbs):
    return sum(int(l) << (64 * i) for i, l in enumerate(limbs)) * RQ_INV % P


def test_the_knob_chooses_the_exponentiation(zkp, orc, mode):
    """zkp_selftest_final_exp_counts: which of the two ended a host check.  Anything but the word "plain" is the chain."""
    import zkp_hip.pairing as zp
    g2s = g2_from_ints(PM.g2_mul(PM.G2, 2))
    cxy, _ = orc.points_from_ints([M.g1_mul(M.G1, 2)])              # f = X: C = [s]G, at z = 1: y = 1, W = G
    wxy, _ = orc.points_from_ints([M.G1])
    one = orc.fr_from_ints([1])[0]
    before = zp.final_exp_counts()
    assert zkp.kzg_verify(g2s, (cxy[0], 0), (wxy[0], 0), one, one)
    after = zp.final_exp_counts()
    want = (0, 1) if mode == "plain" else (1, 0)
    assert (after[0] - before[0], after[1] - before[1]) == want


def test_kzg_verify_reference_cases(zkp, orc, mode):
    # kzg/src/commitment.rs:36-53: secret 2, 1 + 2X + 3X^2 at z = 1
    s = 2
    g2s = g2_from_ints(PM.g2_mul(PM.G2, s))
    pts = M.srs(s, 13)
    w, y = M.kzg_open([1, 2, 3], 1, pts)
    cxy, _ = orc.points_from_ints([M.msm_naive([1, 2, 3], pts)])
    wxy, winf = orc.points_from_ints([w])
    f = lambda v: orc.fr_from_ints([v])[0]
    assert y == 6 and zkp.kzg_verify(g2s, (cxy[0], 0), (wxy[0], int(winf[0])), f(y), f(1))
    assert not zkp.kzg_verify(g2s, (cxy[0], 0), (wxy[0], int(winf[0])), f(y + 1), f(1))
    assert not zkp.kzg_verify(g2s, (cxy[0], 0), (wxy[0], int(winf[0])), f(y), f(2))
    assert not zkp.kzg_verify(g2_from_ints(PM.g2_mul(PM.G2, 3)), (cxy[0], 0), (wxy[0], int(winf[0])), f(y), f(1))
    assert not zkp.kzg_verify(g2s, (cxy[0], 1), (wxy[0], 0), f(y), f(1))          # the identity as the commitment


def test_kzg_batch_verify(zkp, orc, mode):
    # kzg/src/commitment.rs:95-119
    s = 0xABCDEF
    g2s = g2_from_ints(PM.g2_mul(PM.G2, s))
    pts = M.srs(s, 11)
    cms, ws, zs, ys = [], [], [], []
    for k in range(3):
        coeffs = M.rand_fr_list(900 + k, 8)
        z = M.rand_fr_list(950 + k, 1)[0]
        w, y = M.kzg_open(coeffs, z, pts)
        cms.append(M.msm_naive(coeffs, pts)); ws.append(w); zs.append(z); ys.append(y)
    cxy, _ = orc.points_from_ints(cms)
    wxy, _ = orc.points_from_ints(ws)
    rp = orc.fr_from_ints([3, 2 ** 100 + 7, 2 ** 127 - 1])
    assert zkp.kzg_batch_verify(g2s, cxy, orc.fr_from_ints(zs), wxy, orc.fr_from_ints(ys), rp)
    ys[1] = (ys[1] + 1) % R
    assert not zkp.kzg_batch_verify(g2s, cxy, orc.fr_from_ints(zs), wxy, orc.fr_from_ints(ys), rp)


def test_pairing_value_is_the_plain_one_whatever_the_knob(zkp, orc, mode):
    g1xy, _ = orc.points_from_ints([M.G1])
    got = zkp.pairing(g1xy[0], zkp.g2_generator())
    assert [fq_canon(row) for row in got] == PM.f12_flat(PM.pairing(M.G1, PM.G2))
