"""GPU: the transform over G1 points (zkp_g1_ntt*, zkp_g1_scale_dev), the Lagrange-basis SRS (zkp_g1_bases_lagrange) and all openings
of a polynomial at once (zkp_kzg_opener_*, zkp_kzg_open_all*).  Expected values come from the trapdoor: inputs are [a_i]G with known
a_i, expected points are the oracle's fixed-base products of scalars computed with the oracle's Fr transform and big integers; the
smallest transforms are also checked straight from the definition with the oracle's naive MSM over powers of the root.  Everything
is compared bit for bit on the affine limbs and the flag byte (the limbs of an identity are zeros)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bigmodel as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R
LAMBDA = 0xAC45A4010001A40200000000FFFFFFFF
EDGES = [0, 1] + [m * LAMBDA + d for m in (1, 2, 1 << 64, LAMBDA - 1, LAMBDA, LAMBDA + 1) for d in (-1, 0, 1) if m * LAMBDA + d < R] + [R - 1, R - 2]
SECRET = 0x1F2E3D4C5B6A7988


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).cuda()


def host(t, shape):
    return t.cpu().numpy().view(np.uint64 if len(shape) == 2 else np.uint8).reshape(shape)


def points_of(orc, ints):
    """[a]G for every a, identities as zero limbs with the flag set"""
    return orc.g1_fixed_base_mul(orc.fr_from_ints([a % R for a in ints]))


def same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(np.asarray(got[1], dtype=np.uint8), np.asarray(exp[1], dtype=np.uint8))


def root(orc, log_n):
    return orc.fr_to_ints(orc.fr_root_of_unity(log_n).reshape(1, 4))[0]


def ntt_ints(orc, ints, inverse=False):
    return orc.fr_to_ints(orc.ntt_fr(orc.fr_from_ints([a % R for a in ints]), inverse=inverse))


def rand_ints(orc, seed, n):
    return orc.fr_to_ints(orc.rand_fr(seed, n))


def g1_ntt_dev(zkp, pts, inverse=False):
    import torch
    xy, inf = dev(pts[0]), dev(pts[1])
    n = pts[0].shape[0]
    zkp.g1_ntt_dev(xy, inf, n.bit_length() - 1, inverse=inverse)
    torch.cuda.synchronize()
    return host(xy, (n, 12)), host(inf, (n,))


# ------------------------------------------------------------------------------------------------------------ scale
def test_scale_edge_scalars_and_points(zkp, orc):
    import torch
    special = [0, 1, 2, R - 1, R - 2] + EDGES
    n = 300
    a = rand_ints(orc, 0x6171, n)
    k = special + rand_ints(orc, 0x6172, n - len(special))
    for i in (40, 41, 150, n - 1):
        a[i] = 0                      # P = O, next to each other and at the end
    a[60:70] = [a[60]] * 10           # equal points in neighbouring lanes
    k[64] = k[63]                     # ... and two lanes that are equal altogether
    k[200] = 0                        # k = 0 on a finite point among random ones
    pts = points_of(orc, a)
    xy, inf = dev(pts[0]), dev(pts[1])
    zkp.g1_scale_dev(xy, dev(orc.fr_from_ints(k)), n, is_inf_tensor=inf)
    torch.cuda.synchronize()
    exp = points_of(orc, [x * y for x, y in zip(a, k)])
    got = host(xy, (n, 12)), host(inf, (n,))
    bad = [i for i in range(n) if not (np.array_equal(got[0][i], exp[0][i]) and got[1][i] == exp[1][i])]
    assert not bad, [(i, hex(k[i])) for i in bad[:8]]
    assert exp[1].sum() >= 6


def test_scale_without_flags_and_of_nothing(zkp, orc):
    """d_is_inf == NULL: every point is read as finite and an identity product is written as zero limbs only; n == 0 touches nothing"""
    import torch
    n = 70
    a = rand_ints(orc, 0x6173, n)
    k = rand_ints(orc, 0x6174, n)
    k[3] = k[69] = 0
    xy = dev(points_of(orc, a)[0])
    zkp.g1_scale_dev(xy, dev(orc.fr_from_ints(k)), n)
    torch.cuda.synchronize()
    exp = points_of(orc, [x * y for x, y in zip(a, k)])
    assert exp[1].tolist() == [1 if i in (3, 69) else 0 for i in range(n)]
    assert np.array_equal(host(xy, (n, 12)), exp[0])
    before = host(xy, (n, 12)).copy()
    zkp.g1_scale_dev(xy, dev(orc.fr_from_ints(k)), 0)
    assert zkp.lib().zkp_g1_scale_dev(None, None, None, 0, None) == zkp.ZKP_OK
    torch.cuda.synchronize()
    assert np.array_equal(host(xy, (n, 12)), before)


# ------------------------------------------------------------------------------------------------------------ transform
_vectors = {}


def vector(orc, log_n):
    """(a, points, forward, inverse) of one size, computed once: identities scattered and at both ends from n = 8 on"""
    if log_n not in _vectors:
        n = 1 << log_n
        a = rand_ints(orc, 0x6180 + log_n, n)
        if n >= 8:
            for i in (0, 5, n // 2, n - 1):
                a[i] = 0
        _vectors[log_n] = (a, points_of(orc, a), points_of(orc, ntt_ints(orc, a)), points_of(orc, ntt_ints(orc, a, inverse=True)))
    return _vectors[log_n]


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 6, 7, 10, 13])
def test_transform_against_the_trapdoor(zkp, orc, log_n):
    a, pts, fwd, inv = vector(orc, log_n)
    got_f, got_i = g1_ntt_dev(zkp, pts), g1_ntt_dev(zkp, pts, inverse=True)
    assert same(got_f, fwd), log_n
    assert same(got_i, inv), log_n
    assert same(g1_ntt_dev(zkp, got_f, inverse=True), pts), "round trip"
    assert same(zkp.g1_ntt(pts[0], pts[1]), fwd), "host entry, forward"
    assert same(zkp.g1_ntt(pts[0], pts[1], inverse=True), inv), "host entry, inverse"


@pytest.mark.parametrize("log_n", [0, 1, 2, 3])
def test_transform_against_the_definition(zkp, orc, log_n):
    n = 1 << log_n
    a, pts, _, _ = vector(orc, log_n)
    for inverse in (False, True):
        w = pow(root(orc, log_n), -1 if inverse else 1, R)
        c = pow(n, -1, R) if inverse else 1
        rows = [orc.msm_naive(pts[0], pts[1], orc.fr_from_ints([c * pow(w, i * j, R) % R for j in range(n)])) for i in range(n)]
        exp = np.stack([r[0] for r in rows]), np.array([r[1] for r in rows], dtype=np.uint8)
        exp[0][exp[1] != 0] = 0
        assert same(g1_ntt_dev(zkp, pts, inverse=inverse), exp), (log_n, inverse)


@pytest.mark.parametrize("log_n", [3, 7, 10])
def test_transform_constant_and_padded_vectors(zkp, orc, log_n):
    n = 1 << log_n
    c = 0x123456789ABCDEF0123456789
    got = g1_ntt_dev(zkp, points_of(orc, [c] * n))       # every butterfly adds equal or opposite points
    assert same(got, points_of(orc, [n * c] + [0] * (n - 1)))
    assert got[1].tolist() == [0] + [1] * (n - 1)
    d = n // 2 - 1
    a = rand_ints(orc, 0x6190 + log_n, d) + [0] * (n - d)  # the shape of an opener's vector: d finite points, then identities
    for inverse in (False, True):
        assert same(g1_ntt_dev(zkp, points_of(orc, a), inverse=inverse), points_of(orc, ntt_ints(orc, a, inverse=inverse))), inverse


# ------------------------------------------------------------------------------------------------------------ Lagrange
_srs = {}


def srs(zkp, orc, count):
    """(points, handle) of [s^i]G, i < count"""
    if count not in _srs:
        xy = zkp.srs_g1(orc.fr_from_ints([SECRET])[0], count)
        _srs[count] = (xy, zkp.G1Bases.from_host(xy))
    return _srs[count]


@pytest.mark.parametrize("n", [1, 8, 64, 1024])
def test_lagrange_srs(zkp, orc, n):
    log_n = n.bit_length() - 1
    xy, h = srs(zkp, orc, n)
    lag = h.lagrange(log_n)
    assert len(lag) == n and lag.info() == (0, 0)
    w = root(orc, log_n)
    ninv = pow(n, -1, R)
    L = lambda i: pow(w, i, R) * (pow(SECRET, n, R) - 1) % R * ninv % R * pow(SECRET - pow(w, i, R), -1, R) % R
    for i in sorted({0, 1 % n, n // 2, n - 1}):
        e = np.zeros((n, 4), dtype=np.uint64)
        e[i] = orc.fr_from_ints([1])[0]
        exp = points_of(orc, [L(i)])
        got = zkp.msm_g1(lag, e)
        assert got[1] == exp[1][0] and np.array_equal(got[0], exp[0][0]), (n, i)
    got = zkp.msm_g1(lag, orc.fr_from_ints([1] * n))
    assert got[1] == 0 and np.array_equal(got[0], xy[0]), "the Lagrange points sum to S_0"
    rep = lag.validate()
    assert rep["checked"] == n and rep["bad"] == 0
    others = [h.lagrange(log_n).precompute(12), h.lagrange(log_n).precompute(12, glv=True)]
    for length in sorted({n, max(1, n - 3)}):
        coeffs = orc.rand_fr(0x61A0 + length, length)
        padded = np.zeros((n, 4), dtype=np.uint64)
        padded[:length] = coeffs
        evals = orc.ntt_fr(padded)
        exp = zkp.kzg_commit(h, coeffs)
        for handle in [lag] + others:
            got = zkp.kzg_commit(handle, evals)
            assert got[1] == exp[1] and np.array_equal(got[0], exp[0]), (n, length, handle.expansion())


def test_lagrange_errors(zkp, orc):
    xy, _ = srs(zkp, orc, 8)
    short = zkp.G1Bases.from_host(xy[:7])
    with pytest.raises(zkp.ZkpError) as ei:
        short.lagrange(3)
    assert ei.value.code == zkp.ZKP_E_SIZE
    with pytest.raises(zkp.ZkpError) as ei:
        short.lagrange(25)
    assert ei.value.code == zkp.ZKP_E_ARG
    t = dev(xy[:1].copy())
    assert zkp.lib().zkp_g1_ntt_dev(t.data_ptr(), dev(np.zeros(1, dtype=np.uint8)).data_ptr(), 25, 0, None) == zkp.ZKP_E_ARG
    assert zkp.lib().zkp_g1_ntt(xy.ctypes.data, np.zeros(8, dtype=np.uint8).ctypes.data, 25, 0) == zkp.ZKP_E_ARG


# ------------------------------------------------------------------------------------------------------------ all openings
def expected_openings(orc, f_ints, n):
    log_n = n.bit_length() - 1
    w = root(orc, log_n)
    evals = ntt_ints(orc, f_ints + [0] * (n - len(f_ints)))
    fs = 0
    for c in reversed(f_ints):
        fs = (fs * SECRET + c) % R
    return points_of(orc, [(fs - evals[m]) * pow(SECRET - pow(w, m, R), -1, R) for m in range(n)]), orc.fr_from_ints(evals)


_openers = {}


def opener(zkp, orc, n):
    if n not in _openers:
        _openers[n] = zkp.KzgOpener(srs(zkp, orc, n - 1)[1], n.bit_length() - 1)
    return _openers[n]


@pytest.mark.parametrize("n", [2, 4, 8, 64, 128, 1024, 4096])
def test_open_all_against_the_trapdoor_and_kzg_open(zkp, orc, n):
    log_n = n.bit_length() - 1
    _, h = srs(zkp, orc, n - 1)
    op = opener(zkp, orc, n)
    lengths = [n] if n == 4096 else [n, max(1, n - 3)]  # a non-zero top coefficient; fewer coefficients than points
    for length in lengths:
        f = rand_ints(orc, 0x61B0 + n + length, length)
        coeffs = orc.fr_from_ints(f)
        exp, exp_ev = expected_openings(orc, f, n)
        got, ev = op.open_all(coeffs)
        assert np.array_equal(ev, exp_ev), (n, length)
        assert same(got, exp), (n, length)
        w = root(orc, log_n)
        for m in sorted({0, 1, n // 2, n - 1}):
            z = orc.fr_from_ints([pow(w, m, R)])[0]
            (xy, inf), e = zkp.kzg_open(h, coeffs, z)
            assert inf == got[1][m] and np.array_equal(xy, got[0][m]) and np.array_equal(e, ev[m]), (n, length, m)


def test_open_all_two_launches(zkp, orc):
    """n = 2^18: the smallest n whose 2n pointwise products take two launches of G1_NTT_LAUNCH = 2^18 lanes.  The evaluations are compared
    in full with the oracle's Fr transform; proofs 0, 1, n/2 - 1, n/2, n - 2, n - 1 limb for limb with zkp_kzg_open at w^m -- every proof
    depends on all 2n products through the inverse transform, so a sample checks both launches."""
    log_n = 18
    n = 1 << log_n
    h = zkp.G1Bases.from_host(zkp.srs_g1(orc.fr_from_ints([SECRET])[0], n - 1))
    op = zkp.KzgOpener(h, log_n)  # about 0.4 GB, released below
    try:
        coeffs = orc.rand_fr(0x61B8, n)
        got, ev = op.open_all(coeffs)
    finally:
        op.close()
    assert np.array_equal(ev, orc.ntt_fr(coeffs))
    w = root(orc, log_n)
    for m in (0, 1, n // 2 - 1, n // 2, n - 2, n - 1):
        z = orc.fr_from_ints([pow(w, m, R)])[0]
        (xy, inf), e = zkp.kzg_open(h, coeffs, z)
        assert inf == got[1][m] and np.array_equal(xy, got[0][m]) and np.array_equal(e, ev[m]), m
    h.close()


def test_open_all_proof_verifies(zkp, orc):
    import pairing_model as PairM
    from test_pairing_cpu import g2_from_ints
    n = 8
    _, h = srs(zkp, orc, n)  # (the commitment of n coefficients takes n points, the opener n - 1)
    coeffs = orc.rand_fr(0x61C0, n)
    (xy, inf), ev = opener(zkp, orc, n).open_all(coeffs)
    g2s = g2_from_ints(PairM.g2_mul(PairM.G2, SECRET))
    z = orc.fr_from_ints([pow(root(orc, 3), 5, R)])[0]
    assert zkp.kzg_verify(g2s, zkp.kzg_commit(h, coeffs), (xy[5], int(inf[5])), ev[5], z)
    assert not zkp.kzg_verify(g2s, zkp.kzg_commit(h, coeffs), (xy[4], int(inf[4])), ev[5], z)


@pytest.mark.parametrize("n", [8, 64])
def test_open_all_special_polynomials(zkp, orc, n):
    xy, _ = srs(zkp, orc, n - 1)
    op = opener(zkp, orc, n)
    zeros = np.zeros((n, 12), dtype=np.uint64), np.ones(n, dtype=np.uint8)
    got, ev = op.open_all(orc.fr_from_ints([77]))                     # a constant: every quotient is zero
    assert same(got, zeros) and np.array_equal(ev, orc.fr_from_ints([77] * n))
    got, ev = op.open_all(np.zeros((n, 4), dtype=np.uint64))          # the zero vector, full length
    assert same(got, zeros) and not ev.any()
    got, ev = op.open_all(orc.fr_from_ints([0, 1]))                   # f = X: every quotient is 1
    assert same(got, (np.tile(xy[0], (n, 1)), np.zeros(n, dtype=np.uint8)))
    f = rand_ints(orc, 0x61D0 + n, n - 1) + [0]                       # a zero top coefficient is used as given
    assert same(op.open_all(orc.fr_from_ints(f))[0], expected_openings(orc, f, n)[0])
    assert op.open_all(orc.fr_from_ints(f), want_evals=False)[1] is None


def test_open_all_source_forms_and_device_entry(zkp, orc):
    import torch
    n = 64
    xy, h = srs(zkp, orc, n - 1)
    coeffs = orc.rand_fr(0x61E0, n)
    ref, ref_ev = opener(zkp, orc, n).open_all(coeffs)
    for glv in (False, True):
        src = zkp.G1Bases.from_host(xy).precompute(12, glv=glv)
        op = zkp.KzgOpener(src, 6)
        src.close()                                                   # the opener keeps nothing of its source
        got, ev = op.open_all(coeffs)
        assert same(got, ref) and np.array_equal(ev, ref_ev), glv
        op.close()
    op = opener(zkp, orc, n)
    for length in (n, 17):
        d_xy = torch.zeros(n * 12, dtype=torch.int64, device="cuda")
        d_inf = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        d_ev = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
        op.open_all_dev(dev(coeffs[:length]), length, d_xy, d_inf, d_ev)
        torch.cuda.synchronize()
        exp, exp_ev = op.open_all(coeffs[:length])
        assert same((host(d_xy, (n, 12)), host(d_inf, (n,))), exp) and np.array_equal(host(d_ev, (n, 4)), exp_ev), length
    op.open_all_dev(dev(coeffs), n, d_xy, d_inf)                      # evaluations not asked for
    torch.cuda.synchronize()
    assert same((host(d_xy, (n, 12)), host(d_inf, (n,))), ref)


def test_opener_errors(zkp, orc):
    xy, h = srs(zkp, orc, 7)
    for log_n in (0, 24):
        with pytest.raises(zkp.ZkpError) as ei:
            zkp.KzgOpener(h, log_n)
        assert ei.value.code == zkp.ZKP_E_ARG
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.KzgOpener(zkp.G1Bases.from_host(xy[:6]), 3)
    assert ei.value.code == zkp.ZKP_E_SIZE
    op = opener(zkp, orc, 8)
    with pytest.raises(zkp.ZkpError) as ei:
        op.open_all(np.zeros((0, 4), dtype=np.uint64))
    assert ei.value.code == zkp.ZKP_E_ARG
    with pytest.raises(zkp.ZkpError) as ei:
        op.open_all(orc.rand_fr(1, 9))
    assert ei.value.code == zkp.ZKP_E_SIZE
    assert same(op.open_all(orc.fr_from_ints([1, 2, 3]))[0], expected_openings(orc, [1, 2, 3], 8)[0])  # still usable


def test_kzg_scheme_open_all(zkp, orc):
    s = zkp.Srs.new_from_secret(orc.fr_from_ints([SECRET])[0], 8)
    scheme = zkp.KzgScheme(s, expand_bases=False)
    f = [3, 1, 4, 1, 5, 9, 2, 6]
    got, ev = scheme.open_all(orc.fr_from_ints(f), 3)
    exp, exp_ev = expected_openings(orc, f, 8)
    assert same(got, exp) and np.array_equal(ev, exp_ev)
    assert same(scheme.open_all(orc.fr_from_ints(f[:5]), 3)[0], expected_openings(orc, f[:5], 8)[0])  # the same opener again
    assert list(scheme._openers) == [3]
    scheme.close()                                                    # releases the openers; the scheme still commits
    assert scheme._openers == {}
    assert scheme.commit(orc.fr_from_ints(f))[1] == 0


def test_sharded_source_is_refused_in_a_child_process():
    """two slots on one GPU, a sharded source handle: both entries are ZKP_E_ARG and a single-slot call still works afterwards"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "g1_ntt_worker.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "OK g1_ntt slots" in p.stdout
