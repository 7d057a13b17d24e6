"""GPU: many pairing-product checks per launch (zkp_pairing_checker_*, zkp_pairing_check_batch*).  Expected verdicts come from discrete
logs, not from model pairings: Q_j = [b_j]G_2 and P_j = [a_j]G (made by zkp_g1_fixed_base_mul_dev), so the product of a check is 1
iff sum a_j b_j = 0 mod r; a_k is chosen to make it so, and a_k + 1 to break it.  In every run exactly the checks
{0, 31, 63, 64, n - 1} (those that exist) are broken and the verdict bytes must match index by index: an all-ones or all-zeros
kernel fails, and so does a lane or wave mix-up.  No test provokes a fault: bad input here is an error code or a rejected check."""
import random

import numpy as np
import pytest

import bigmodel as M
import pairing_model as PM

pytestmark = pytest.mark.gpu
R, P = M.R, M.P
B = [1, 0x5EC2E7, 0xD15C0, 0x1234567]     # the discrete logs of the fixed G2 points
MAX_CHECKS = 130


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def pairing_module():
    import zkp_hip.pairing
    return zkp_hip.pairing


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).cuda()


_cache = {}


def g2_points(zkp, orc, k):
    if ("g2", k) not in _cache:
        _cache[("g2", k)] = np.stack([zkp.g2_mul(zkp.g2_generator(), orc.fr_from_ints([b])[0])[0] for b in B[:k]])
    return _cache[("g2", k)]


def checker(zkp, orc, k):
    if ("checker", k) not in _cache:
        _cache[("checker", k)] = pairing_module().PairingChecker(g2_points(zkp, orc, k), MAX_CHECKS)
    return _cache[("checker", k)]


def fixed_base(zkp, orc, scalars):
    """[a]G for every a, resident: (n x 12 limbs, n flags); a = 0 gives the identity flag"""
    import torch
    n = len(scalars)
    xy = torch.zeros(n * 12, dtype=torch.int64, device="cuda")
    inf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    zkp.g1_fixed_base_mul_dev(dev(orc.fr_from_ints(scalars)), n, xy, inf)
    torch.cuda.synchronize()
    return xy, inf


def broken_set(n):
    return sorted({i for i in (0, 31, 63, 64, n - 1) if 0 <= i < n})


def scalars_for(n, k, seed, logs=None):
    """n x k discrete logs a with sum_j a_j b_j = 0, except in the broken checks, where the last is one more"""
    logs = logs or B[:k]
    rng = random.Random(seed)
    bad = set(broken_set(n))
    out = []
    for c in range(n):
        a = [rng.randrange(1, R) for _ in range(k - 1)]
        last = (-sum(x * b for x, b in zip(a, logs)) * pow(logs[k - 1], -1, R)) % R
        out += a + [(last + 1) % R if c in bad else last]
    return out


@pytest.mark.parametrize("k", [1, 2, 3])
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 130])
def test_verdict_per_check(zkp, orc, n, k):
    """k = 1: sum = a_1, so only the identity P is accepted (the fixed-base entry flags it)"""
    import torch
    xy, inf = fixed_base(zkp, orc, scalars_for(n, k, 1000 * k + n))
    ok = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
    checker(zkp, orc, k).check_batch_dev(xy, n, ok_tensor=ok, p_inf_tensor=inf)
    torch.cuda.synchronize()
    want = [0 if c in broken_set(n) else 1 for c in range(n)]
    assert ok.cpu().numpy().tolist() == want


def test_host_entry_agrees_with_dev_entry_and_validates(zkp, orc):
    import torch
    n, k = 65, 2
    xy, inf = fixed_base(zkp, orc, scalars_for(n, k, 77))
    ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    val = torch.zeros(n * 72, dtype=torch.int64, device="cuda")
    c = checker(zkp, orc, k)
    c.check_batch_dev(xy, n, ok_tensor=ok, p_inf_tensor=inf, validate=True, out_tensor=val)
    torch.cuda.synchronize()
    h_ok, h_val = c.check_batch(xy.cpu().numpy().view(np.uint64).reshape(n, k, 12), inf.cpu().numpy().reshape(n, k), validate=True, values=True)
    assert h_ok.tolist() == ok.cpu().numpy().tolist() == [0 if i in broken_set(n) else 1 for i in range(n)]
    assert np.array_equal(h_val.reshape(n, 72), val.cpu().numpy().view(np.uint64).reshape(n, 72))
    one = np.zeros(72, dtype=np.uint64)
    one[:6] = M.to_limbs(M.fq_to_mont(1), 6)
    for i in range(n):
        assert np.array_equal(h_val.reshape(n, 72)[i], one) == bool(h_ok[i])     # the verdict is E == 1
    # values alone, verdicts alone
    only = torch.zeros(n * 72, dtype=torch.int64, device="cuda")
    c.check_batch_dev(xy, n, p_inf_tensor=inf, out_tensor=only)
    torch.cuda.synchronize()
    assert torch.equal(only, val)


def test_identity_p_is_skipped_not_multiplied_in(zkp, orc):
    """k = 3 with P_2 flagged as the identity over whatever coordinates: the check is a_1 b_1 + a_3 b_3"""
    import torch
    k, rng = 3, random.Random(5)
    rows, flags, want = [], [], []
    for c in range(6):
        a1, a2 = rng.randrange(1, R), rng.randrange(1, R)
        a3 = (-a1 * B[0] * pow(B[2], -1, R)) % R
        good = c % 2 == 0
        rows += [a1, a2, a3 if good else (a3 + 1) % R]
        flags += [0, 1, 0]
        want.append(1 if good else 0)
    xy, _ = fixed_base(zkp, orc, rows)
    ok = torch.zeros(6, dtype=torch.uint8, device="cuda")
    checker(zkp, orc, k).check_batch_dev(xy, 6, ok_tensor=ok, p_inf_tensor=dev(np.array(flags, dtype=np.uint8)))
    torch.cuda.synchronize()
    assert ok.cpu().numpy().tolist() == want
    # without the flags the middle pair counts and nothing verifies
    checker(zkp, orc, k).check_batch_dev(xy, 6, ok_tensor=ok)
    torch.cuda.synchronize()
    assert ok.cpu().numpy().tolist() == [0] * 6
    # every pair the identity: the empty product
    checker(zkp, orc, k).check_batch_dev(xy, 6, ok_tensor=ok, p_inf_tensor=dev(np.ones(18, dtype=np.uint8)))
    torch.cuda.synchronize()
    assert ok.cpu().numpy().tolist() == [1] * 6


def test_identity_q_slot_is_skipped(zkp, orc):
    import torch
    k = 3
    c = pairing_module().PairingChecker(g2_points(zkp, orc, k), 8, g2_is_inf=[0, 1, 0])
    rng = random.Random(6)
    rows, want = [], []
    for i in range(5):
        a1, a2 = rng.randrange(1, R), rng.randrange(1, R)
        a3 = (-a1 * B[0] * pow(B[2], -1, R)) % R
        rows += [a1, a2, a3 if i != 3 else (a3 + 1) % R]
        want.append(1 if i != 3 else 0)
    xy, inf = fixed_base(zkp, orc, rows)
    ok = torch.zeros(5, dtype=torch.uint8, device="cuda")
    c.check_batch_dev(xy, 5, ok_tensor=ok, p_inf_tensor=inf)
    torch.cuda.synchronize()
    assert ok.cpu().numpy().tolist() == want
    c.close()


def _bad_points(orc):
    g = M.g1_mul(M.G1, 9)
    off, _ = orc.points_from_ints([(g[0], (g[1] + 1) % P)])
    good, _ = orc.points_from_ints([g])
    noncanon = good[0].copy()
    xm = sum(int(v) << (64 * i) for i, v in enumerate(good[0][:6])) + P
    assert xm < 1 << 384
    noncanon[:6] = [(xm >> (64 * i)) & (2 ** 64 - 1) for i in range(6)]
    x = 1
    while True:   # on the curve, outside the r-torsion (the cofactor of G1 is ~2^126)
        rhs = (x * x * x + 4) % P
        yy = pow(rhs, (P + 1) // 4, P)
        if yy * yy % P == rhs:
            break
        x += 1
    outside, _ = orc.points_from_ints([(x, yy)])
    return {"curve": off[0], "canonical": noncanon, "subgroup": outside[0]}


def test_validation_names_the_bad_point(zkp, orc):
    n, k = 5, 2
    xy, inf = fixed_base(zkp, orc, scalars_for(n, k, 9))
    pts = xy.cpu().numpy().view(np.uint64).reshape(n, k, 12).copy()
    flags = inf.cpu().numpy().reshape(n, k)
    c = checker(zkp, orc, k)
    assert c.check_batch(pts, flags, validate=True).tolist() == [0, 1, 1, 1, 0]
    for word, pt in _bad_points(orc).items():
        bad = pts.copy()
        bad[3, 1] = pt
        bad[4, 0] = pt
        for call in (lambda: c.check_batch(bad, flags, validate=True),
                     lambda: c.check_batch_dev(dev(bad.reshape(-1)), n, ok_tensor=dev(np.zeros(n, dtype=np.uint8)), validate=True)):
            with pytest.raises(zkp.ZkpError) as ei:
                call()
            assert ei.value.code == zkp.ZKP_E_ARG
            assert "p[7]" in str(ei.value) and "check 3, pair 1" in str(ei.value) and word in str(ei.value)
        # unvalidated: a verdict, whatever it is, and no error
        assert c.check_batch(bad, flags, validate=False).shape == (n,)


def test_refusals(zkp, orc):
    pm = pairing_module()
    c = checker(zkp, orc, 2)
    with pytest.raises(zkp.ZkpError) as ei:
        c.check_batch(np.zeros((MAX_CHECKS + 1, 2, 12), dtype=np.uint64), np.ones((MAX_CHECKS + 1, 2), dtype=np.uint8))
    assert ei.value.code == zkp.ZKP_E_SIZE
    assert c.check_batch(np.zeros((0, 2, 12), dtype=np.uint64)).shape == (0,)
    g2 = g2_points(zkp, orc, 2)
    for make in (lambda: pm.PairingChecker(np.zeros((9, 24), dtype=np.uint64), 4, g2_is_inf=[1] * 9), lambda: pm.PairingChecker(g2, 0)):
        with pytest.raises(zkp.ZkpError) as ei:
            make()
        assert ei.value.code == zkp.ZKP_E_ARG
    off = g2.copy()
    off[1, 0] ^= np.uint64(1)
    with pytest.raises(zkp.ZkpError) as ei:
        pm.PairingChecker(off, 4)
    assert ei.value.code == zkp.ZKP_E_ARG and "g2[1]" in str(ei.value)


def test_agrees_with_kzg_verify_on_the_reference_case(zkp, orc):
    """kzg/src/commitment.rs:36-53: secret 2, 1 + 2X + 3X^2 at z = 1 gives y = 6; y = 7 is rejected.  The check of one opening is
    e(C + [z]W - [y]G, G_2) e(-W, [s]_2) == 1."""
    s, coeffs, z = 2, [1, 2, 3], 1
    pts = M.srs(s, 13)
    w, y = M.kzg_open(coeffs, z, pts)
    commit = M.msm_naive(coeffs, pts)
    g2s = zkp.g2_mul(zkp.g2_generator(), orc.fr_from_ints([s])[0])[0]
    c = pairing_module().PairingChecker(np.stack([zkp.g2_generator(), g2s]), 2)
    cxy, _ = orc.points_from_ints([commit])
    wxy, _ = orc.points_from_ints([w])
    f = lambda v: orc.fr_from_ints([v])[0]
    rows, want = [], []
    for value in (y, y + 1):
        left = M.g1_add(M.g1_add(commit, M.g1_mul(w, z)), M.g1_neg(M.g1_mul(M.G1, value)))
        pxy, _ = orc.points_from_ints([left, M.g1_neg(w)])
        rows.append(pxy)
        want.append(1 if zkp.kzg_verify(g2s, (cxy[0], 0), (wxy[0], 0), f(value), f(z)) else 0)
    assert y == 6 and want == [1, 0]
    assert c.check_batch(np.stack(rows)).tolist() == want
    c.close()
