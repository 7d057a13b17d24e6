"""GPU: the coset openings (zkp_kzg_opener_create_cosets, zkp_kzg_open_cosets*, zkp_kzg_verify_coset).  Expected values come from the
trapdoor as in tests/test_gpu_g1_ntt.py: the SRS is [s^i]G with a known s, the expected proof of coset k is the oracle's fixed-base
product of q_k(s), computed with big integers -- by the division recurrence up to n = 64, by the O(n) closed form of
tests/model/g1_coset_model.py (pinned against the recurrence in tests/test_g1_coset_model_cpu.py) above.  Everything is compared bit
for bit on the affine limbs and the flag byte.  ZKP_KZG_COSET_GROUP_LOG is set around the creation of an opener to run every group
size of the multiply-accumulate pass, whichever the plan header commits."""
import os
import subprocess
import sys

import numpy as np
import pytest

import g1_coset_model as cm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = cm.R
SECRET = 0x1F2E3D4C5B6A7988
KNOB = "ZKP_KZG_COSET_GROUP_LOG"


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
    return orc.g1_fixed_base_mul(orc.fr_from_ints([a % R for a in ints]))


def same(got, exp):
    return np.array_equal(got[0], exp[0]) and np.array_equal(np.asarray(got[1], dtype=np.uint8), np.asarray(exp[1], dtype=np.uint8))


def rand_ints(orc, seed, n):
    return orc.fr_to_ints(orc.rand_fr(seed, n))


_srs, _openers, _expected = {}, {}, {}


def srs(zkp, orc, count):
    """(points, handle) of [s^i]G, i < count"""
    if count not in _srs:
        xy = zkp.srs_g1(orc.fr_from_ints([SECRET])[0], count)
        _srs[count] = (xy, zkp.G1Bases.from_host(xy))
    return _srs[count]


def make_opener(zkp, source, log_n, log_l, group_log=None):
    old = os.environ.pop(KNOB, None)
    if group_log is not None:
        os.environ[KNOB] = str(group_log)
    try:
        return zkp.KzgOpener(source, log_n, log_l)
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


def opener(zkp, orc, log_n, log_l, group_log=None):
    key = (log_n, log_l, group_log)
    if key not in _openers:
        _openers[key] = make_opener(zkp, srs(zkp, orc, 1 << log_n)[1], log_n, log_l, group_log)
    return _openers[key]


def expected(orc, f, log_n, log_l):
    """(the r proof points, the n evaluations) of the coefficients f (integers)"""
    key = (tuple(f) if len(f) <= 64 else (len(f), f[0], f[-1]), log_n, log_l)
    if key not in _expected:
        n, l = 1 << log_n, 1 << log_l
        evals = orc.fr_to_ints(orc.ntt_fr(orc.fr_from_ints(list(f) + [0] * (n - len(f)))))
        if n <= 64:
            q = [cm.evaluate(cm.quotient(f, n, l, k), SECRET) for k in range(n // l)]
        else:
            q = cm.proofs_closed_form(f, evals, SECRET, n, l)
        _expected[key] = (points_of(orc, q), orc.fr_from_ints(evals))
    return _expected[key]


def lengths(n, l):
    return sorted({x for x in (1, l, l + 1, n - 3, n) if 1 <= x <= n})


# r = 2, l below / at / above the largest group, l > r, and the practical cell of 64 points
SHAPES = [(1, 0), (2, 1), (3, 1), (3, 2), (6, 0), (6, 2), (6, 3), (6, 5), (10, 6), (12, 6)]


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_proofs_and_evaluations_against_the_trapdoor(zkp, orc, log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    groups = [None, 0, 1, 2, 3] if log_n <= 10 else [None, 3]
    for length in lengths(n, l):
        f = rand_ints(orc, 0x6200 + 64 * log_n + length, length)
        exp, exp_ev = expected(orc, f, log_n, log_l)
        if length <= l:
            assert exp[1].all(), "len <= l: r identities"
        for group_log in groups:
            got, ev = opener(zkp, orc, log_n, log_l, group_log).open_cosets(orc.fr_from_ints(f), evals=True)
            assert np.array_equal(ev, exp_ev), (length, group_log)
            bad = [k for k in range(n // l) if not (np.array_equal(got[0][k], exp[0][k]) and got[1][k] == exp[1][k])]
            assert not bad, (length, group_log, bad[:8])


def test_cosets_of_one_point_are_open_all(zkp, orc):
    n = 64
    _, h = srs(zkp, orc, n)
    coeffs = orc.rand_fr(0x6210, n - 3)
    plain = zkp.KzgOpener(h, 6)
    ref, ref_ev = plain.open_all(coeffs)
    handle = zkp.C.c_void_p()  # the C entry itself with log_l = 0
    assert zkp.lib().zkp_kzg_opener_create_cosets(h._h, 6, 0, zkp.C.byref(handle)) == zkp.ZKP_OK
    zkp.lib().zkp_kzg_opener_destroy(handle)
    for op in (zkp.KzgOpener(h, 6, 0), plain):
        got, ev = op.open_cosets(coeffs, evals=True)
        assert got[0].tobytes() == ref[0].tobytes() and got[1].tobytes() == ref[1].tobytes() and ev.tobytes() == ref_ev.tobytes()
        assert same(op.open_all(coeffs)[0], ref)
    with pytest.raises(zkp.ZkpError) as ei:  # and the other way round it is refused
        opener(zkp, orc, 6, 3).open_all(coeffs)
    assert ei.value.code == zkp.ZKP_E_ARG


def test_proofs_are_commitments_of_the_quotients(zkp, orc):
    """no trapdoor on this route: zkp_kzg_commit of the model's quotient polynomial"""
    n, l = 64, 8
    _, h = srs(zkp, orc, n)
    f = rand_ints(orc, 0x6220, n)
    got, _ = opener(zkp, orc, 6, 3).open_cosets(orc.fr_from_ints(f))
    for k in range(n // l):
        c = zkp.kzg_commit(h, orc.fr_from_ints(cm.quotient(f, n, l, k)))
        assert c[1] == got[1][k] and np.array_equal(c[0], got[0][k]), k


@pytest.mark.parametrize("group_log", [0, 3])
def test_special_polynomials(zkp, orc, group_log):
    n, l, r = 64, 8, 8
    xy, _ = srs(zkp, orc, n)
    op = opener(zkp, orc, 6, 3, group_log)
    zeros = np.zeros((r, 12), dtype=np.uint64), np.ones(r, dtype=np.uint8)
    got, ev = op.open_cosets(np.zeros((n, 4), dtype=np.uint64), evals=True)            # the zero vector, full length
    assert same(got, zeros) and not ev.any()
    got, ev = op.open_cosets(orc.fr_from_ints([77]), evals=True)                       # a constant
    assert same(got, zeros) and np.array_equal(ev, orc.fr_from_ints([77] * n))
    got, _ = op.open_cosets(orc.fr_from_ints([R - 1] + [0] * (l - 1) + [1]))           # X^l - 1: every quotient is 1
    assert same(got, (np.tile(xy[0], (r, 1)), np.zeros(r, dtype=np.uint8)))
    f = rand_ints(orc, 0x6230, n)
    for i in range(5, n, l):
        f[i] = 0                                                                       # nothing of f on slice 5
    assert same(op.open_cosets(orc.fr_from_ints(f))[0], expected(orc, f, 6, 3)[0])
    assert op.open_cosets(orc.fr_from_ints(f))[1] is None


def test_expanded_source_handles(zkp, orc):
    n = 64
    xy, _ = srs(zkp, orc, n)
    f = rand_ints(orc, 0x6240, n)
    for glv in (False, True):
        src = zkp.G1Bases.from_host(xy).precompute(12, glv=glv)
        op = zkp.KzgOpener(src, 6, 3)
        src.close()                                                                    # the opener keeps nothing of its source
        assert same(op.open_cosets(orc.fr_from_ints(f))[0], expected(orc, f, 6, 3)[0]), glv
        op.close()


@pytest.mark.parametrize("group_log", [None, 3])
def test_two_launches(zkp, orc, group_log):
    """(18, 10): 2^19 terms, two launches of the multiply-accumulate pass; with groups of 8 the second launch begins a group"""
    log_n, log_l = 18, 10
    n = 1 << log_n
    coeffs = orc.rand_fr(0x6250, n)
    f = orc.fr_to_ints(coeffs)
    exp, exp_ev = expected(orc, f, log_n, log_l)
    op = opener(zkp, orc, log_n, log_l, group_log)
    got, ev = op.open_cosets(coeffs, evals=True)
    assert np.array_equal(ev, exp_ev)
    assert same(got, exp)
    _openers.pop((log_n, log_l, group_log)).close()                                    # (a quarter of a GiB)


def test_device_entry_and_a_second_call(zkp, orc):
    import torch
    log_n, log_l = 6, 3
    n, r = 64, 8
    op = opener(zkp, orc, log_n, log_l, 2)
    first, second = orc.rand_fr(0x6260, n), orc.rand_fr(0x6261, 17)
    for coeffs in (first, second, first):                                              # nothing of a call is left for the next
        length = coeffs.shape[0]
        d_xy = torch.zeros(r * 12, dtype=torch.int64, device="cuda")
        d_inf = torch.full((r,), 7, dtype=torch.uint8, device="cuda")
        d_ev = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
        op.open_cosets_dev(dev(coeffs), length, d_xy, d_inf, d_ev)
        torch.cuda.synchronize()
        ref, ref_ev = op.open_cosets(coeffs, evals=True)
        assert same((host(d_xy, (r, 12)), host(d_inf, (r,))), ref) and np.array_equal(host(d_ev, (n, 4)), ref_ev), length
        assert same(ref, expected(orc, orc.fr_to_ints(coeffs), log_n, log_l)[0]), length
    op.open_cosets_dev(dev(first), n, d_xy, d_inf)                                     # evaluations not asked for
    torch.cuda.synchronize()
    assert same((host(d_xy, (r, 12)), host(d_inf, (r,))), expected(orc, orc.fr_to_ints(first), log_n, log_l)[0])


@pytest.mark.parametrize("log_n,log_l", [(6, 3), (4, 1)])
def test_verify_coset(zkp, orc, log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    _, h = srs(zkp, orc, n)
    coeffs = orc.rand_fr(0x6270 + log_n, n)
    (xy, inf), ev = opener(zkp, orc, log_n, log_l).open_cosets(coeffs, evals=True)
    commitment = zkp.kzg_commit(h, coeffs)
    g2 = zkp.g2_generator()
    g2_sl, _ = zkp.g2_mul(g2, orc.fr_from_ints([pow(SECRET, l, R)])[0])
    g2_s, _ = zkp.g2_mul(g2, orc.fr_from_ints([SECRET])[0])
    w = cm.root(log_n)
    x = lambda k: orc.fr_from_ints([pow(w, k, R)])[0]
    for k in range(r):
        assert zkp.kzg_verify_coset(h, g2_sl, commitment, (xy[k], int(inf[k])), x(k), ev[k::r]), k
    k = 3
    wrong = ev[k::r].copy()
    wrong[l - 1] = ev[(k + 1) % n]
    assert not zkp.kzg_verify_coset(h, g2_sl, commitment, (xy[k], int(inf[k])), x(k), wrong), "one altered evaluation"
    assert not zkp.kzg_verify_coset(h, g2_sl, commitment, (xy[k + 1], int(inf[k + 1])), x(k), ev[k::r]), "the neighbouring coset's proof"
    assert not zkp.kzg_verify_coset(h, g2_s, commitment, (xy[k], int(inf[k])), x(k), ev[k::r]), "[s]_2 in place of [s^l]_2"
    off = xy[k].copy()
    off[0] ^= 1
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.kzg_verify_coset(h, g2_sl, commitment, (off, 0), x(k), ev[k::r])
    assert ei.value.code == zkp.ZKP_E_ARG and "curve" in str(ei.value)


def test_error_codes(zkp, orc):
    """ZKP_E_ARG and ZKP_E_SIZE of every entry (ZKP_E_NOMEM: test_creation_beyond_the_byte_budget_is_refused_and_leaves_nothing)"""
    xy, h = srs(zkp, orc, 64)
    for log_n, log_l in ((3, 3), (3, 4), (24, 6), (0, 0), (24, 0)):                      # log_l >= log_n, log_n > 23
        handle = zkp.C.c_void_p()
        assert zkp.lib().zkp_kzg_opener_create_cosets(h._h, log_n, log_l, zkp.C.byref(handle)) == zkp.ZKP_E_ARG, (log_n, log_l)
        assert not handle.value
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.KzgOpener(h, 3, 3)
    assert ei.value.code == zkp.ZKP_E_ARG
    short = zkp.G1Bases.from_host(xy[:64 - 8 - 1])                                     # n - l - 1 points
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.KzgOpener(short, 6, 3)
    assert ei.value.code == zkp.ZKP_E_SIZE
    zkp.KzgOpener(zkp.G1Bases.from_host(xy[:64 - 8]), 6, 3).close()                    # n - l are enough
    op = opener(zkp, orc, 6, 3)
    with pytest.raises(zkp.ZkpError) as ei:
        op.open_cosets(np.zeros((0, 4), dtype=np.uint64))
    assert ei.value.code == zkp.ZKP_E_ARG
    with pytest.raises(zkp.ZkpError) as ei:
        op.open_cosets(orc.rand_fr(1, 65))
    assert ei.value.code == zkp.ZKP_E_SIZE
    f = [1, 2, 3] + [0] * 20 + [5]
    assert same(op.open_cosets(orc.fr_from_ints(f))[0], expected(orc, f, 6, 3)[0])     # still usable
    with pytest.raises(zkp.ZkpError) as ei:                                            # the verifier: fewer than l points
        zkp.kzg_verify_coset(zkp.G1Bases.from_host(xy[:7]), zkp.g2_generator(), (xy[0], 0), (xy[1], 0), orc.fr_from_ints([1])[0],
                             orc.rand_fr(2, 8))
    assert ei.value.code == zkp.ZKP_E_SIZE
    with pytest.raises(zkp.ZkpError) as ei:                                            # x = 0 is the shift of no coset
        zkp.kzg_verify_coset(h, zkp.g2_generator(), (xy[0], 0), (xy[1], 0), np.zeros(4, dtype=np.uint64), orc.rand_fr(2, 8))
    assert ei.value.code == zkp.ZKP_E_ARG and "x = 0" in str(ei.value)
    acc, one, ev = zkp.C.c_int(7), orc.fr_from_ints([1]), orc.rand_fr(2, 8)            # log_l >= 23, refused before evals is read
    rc = zkp.lib().zkp_kzg_verify_coset(h._h, zkp.g2_generator().ctypes.data, xy[0].ctypes.data, 0, xy[1].ctypes.data, 0, one.ctypes.data, 23,
                                        ev.ctypes.data, zkp.C.byref(acc))
    assert rc == zkp.ZKP_E_ARG and acc.value == 7


def test_creation_beyond_the_byte_budget_is_refused_and_leaves_nothing(zkp, orc):
    """ZKP_E_NOMEM of zkp_kzg_opener_create_cosets through ZKP_KZG_OPENER_MAX_BYTES, the branch that also refuses what the device has
    not free: the sizes are in the message, the device has as much free memory afterwards as before, and one byte more is enough."""
    import torch
    n, l = 64, 8
    _, h = srs(zkp, orc, n)
    sz = cm.sizes(n, l, 0)
    total, kept = sz[-1], sz[0]
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    os.environ["ZKP_KZG_OPENER_MAX_BYTES"] = str(total - 1)
    try:
        with pytest.raises(zkp.ZkpError) as ei:
            make_opener(zkp, h, 6, 3, 0)
        after = torch.cuda.mem_get_info()[0]
        os.environ["ZKP_KZG_OPENER_MAX_BYTES"] = str(total)
        op = make_opener(zkp, h, 6, 3, 0)
    finally:
        del os.environ["ZKP_KZG_OPENER_MAX_BYTES"]
    msg = str(ei.value)
    assert ei.value.code == zkp.ZKP_E_NOMEM
    assert f"workspaces of {total} bytes" in msg and f"{kept} kept slices + {total - kept} per call" in msg and f"MAX_BYTES {total - 1}" in msg, msg
    assert after == before, (before, after)
    f = rand_ints(orc, 0x6280, n)
    assert same(op.open_cosets(orc.fr_from_ints(f))[0], expected(orc, f, 6, 3)[0])
    op.close()


def test_kzg_scheme_open_cosets(zkp, orc):
    s = zkp.Srs.new_from_secret(orc.fr_from_ints([SECRET])[0], 16)
    scheme = zkp.KzgScheme(s, expand_bases=False)
    f = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3]
    got, ev = scheme.open_cosets(orc.fr_from_ints(f), 4, 2, evals=True)
    exp, exp_ev = expected(orc, f, 4, 2)
    assert same(got, exp) and np.array_equal(ev, exp_ev)
    assert same(scheme.open_cosets(orc.fr_from_ints(f[:7]), 4, 2)[0], expected(orc, f[:7], 4, 2)[0])  # the same opener again
    assert list(scheme._coset_openers) == [(4, 2)] and scheme._openers == {}
    scheme.close()
    assert scheme._coset_openers == {}


def test_sharded_source_is_refused_in_a_child_process():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kzg_cosets_worker.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "OK kzg cosets slots" in p.stdout
