"""GPU: the coset openings of a batch of polynomials in one call (zkp_kzg_opener_create_cosets_batch, zkp_kzg_open_cosets_batch*).
Expected values come twice, as in tests/test_gpu_kzg_cosets.py: from the trapdoor (the SRS is [s^i]G with a known s, the expected proof
of coset k is the oracle's fixed-base product of q_k(s), by tests/model/g1_coset_model.py), and -- byte for byte -- from
zkp_kzg_open_cosets of each polynomial on an opener made for one.  ZKP_KZG_COSET_GROUP_LOG is set around the creation of an opener
to run other group sizes of the multiply-accumulate pass than the plan header commits."""
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
BUDGET = "ZKP_KZG_OPENER_MAX_BYTES"


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def last_error(zkp):
    return zkp.lib().zkp_last_error().decode()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).cuda()


def host(t, shape):
    return t.cpu().numpy().view(np.uint64 if shape[-1] in (4, 12) else np.uint8).reshape(shape)


_srs, _openers, _expected = {}, {}, {}


def srs(zkp, orc, count):
    """(points, handle) of [s^i]G, i < count"""
    if count not in _srs:
        xy = zkp.srs_g1(orc.fr_from_ints([SECRET])[0], count)
        _srs[count] = (xy, zkp.G1Bases.from_host(xy))
    return _srs[count]


def make_opener(zkp, source, log_n, log_l, max_polys, group_log=None):
    old = os.environ.pop(KNOB, None)
    if group_log is not None:
        os.environ[KNOB] = str(group_log)
    try:
        return zkp.KzgOpener(source, log_n, log_l, max_polys)
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


def opener(zkp, orc, log_n, log_l, max_polys, group_log=None):
    key = (log_n, log_l, max_polys, group_log)
    if key not in _openers:
        _openers[key] = make_opener(zkp, srs(zkp, orc, 1 << log_n)[1], log_n, log_l, max_polys, group_log)
    return _openers[key]


def expected(orc, f, log_n, log_l):
    """(the r proof points and flags, the n evaluations) of the coefficients f (integers) from the trapdoor"""
    while len(f) > 1 and f[-1] == 0:
        f = f[:-1]
    key = (tuple(f), log_n, log_l)
    if key not in _expected:
        n, l = 1 << log_n, 1 << log_l
        evals = orc.fr_to_ints(orc.ntt_fr(orc.fr_from_ints(list(f) + [0] * (n - len(f)))))
        if n <= 64:
            q = [cm.evaluate(cm.quotient(f, n, l, k), SECRET) for k in range(n // l)]
        else:
            q = cm.proofs_closed_form(f, evals, SECRET, n, l)
        _expected[key] = (orc.g1_fixed_base_mul(orc.fr_from_ints([a % R for a in q])), orc.fr_from_ints(evals))
    return _expected[key]


def row_ints(orc, seed, length, effective):
    """`length` coefficients of which the first `effective` are random, the rest zero"""
    return (orc.fr_to_ints(orc.rand_fr(seed, effective)) if effective else []) + [0] * (length - effective)


def check_rows(zkp, orc, got, ev, rows, log_n, log_l, single, where):
    """every row of a batch's outputs against the trapdoor and against open_cosets of that polynomial on `single`"""
    (xy, inf) = got
    for p, f in enumerate(rows):
        exp, exp_ev = expected(orc, f, log_n, log_l)
        assert np.array_equal(xy[p], exp[0]) and np.array_equal(inf[p], np.asarray(exp[1], dtype=np.uint8)), (where, p, "trapdoor")
        assert np.array_equal(ev[p], exp_ev), (where, p, "evaluations")
        (sxy, sinf), sev = single.open_cosets(orc.fr_from_ints(f), evals=True)
        assert xy[p].tobytes() == sxy.tobytes() and inf[p].tobytes() == sinf.tobytes() and ev[p].tobytes() == sev.tobytes(), (where, p, "single call")
        if max([i + 1 for i, c in enumerate(f) if c], default=0) <= (1 << log_l):       # the effective length
            assert inf[p].all() and not xy[p].any(), (where, p, "r identities")


# r = 2; no fold; a fold of several steps; one group per output with l > 1; a batch that is no power of two; the practical cell
SHAPES = [(1, 0, 3, None), (2, 1, 3, None), (3, 2, 2, None), (6, 0, 3, None), (6, 3, 5, None), (6, 3, 3, 3), (6, 5, 3, 3), (6, 5, 2, 0),
          (10, 6, 4, None)]


@pytest.mark.parametrize("log_n,log_l,n_polys,group_log", SHAPES)
def test_batch_equals_the_trapdoor_and_the_single_calls(zkp, orc, log_n, log_l, n_polys, group_log):
    n, l = 1 << log_n, 1 << log_l
    # effective lengths of the rows: full, all zero (r identities), len <= l (r identities), and two in between; a batch takes the
    # next n_polys of them, so two batches hold every kind (the first: a full row and an all-zero one, whose length 0 is below l)
    kinds = [n, 0, l, max(1, n - 3), min(n, l + 1)]
    batches = [[kinds[(i + j) % 5] for j in range(n_polys)] for i in (0, n_polys % 5)]
    single = opener(zkp, orc, log_n, log_l, 1, group_log)
    op = opener(zkp, orc, log_n, log_l, n_polys, group_log)
    for b, effs in enumerate(batches):
        length = max(max(effs), 1)                                                      # the call's len: the longest row
        rows = [row_ints(orc, 0x8100 + 256 * log_n + 16 * b + p, length, e) for p, e in enumerate(effs)]
        coeffs = np.stack([orc.fr_from_ints(f) for f in rows])
        got, ev = op.open_cosets_batch(coeffs, evals=True)
        assert got[0].shape == (n_polys, n // l, 12) and got[1].shape == (n_polys, n // l) and ev.shape == (n_polys, n, 4)
        check_rows(zkp, orc, got, ev, rows, log_n, log_l, single, (b, effs))
        assert op.open_cosets_batch(coeffs)[1] is None                                   # evaluations not asked for


@pytest.mark.parametrize("group_log", [None, 3])
def test_more_lanes_than_one_launch(zkp, orc, group_log):
    """(10, 6) x 129: 129 x 2^11 products, above the 2^18 a launch of the multiply-accumulate pass takes -- two launches, the second
    holds one polynomial (with groups of 8 terms: 2^15 lanes per launch, still 128 polynomials)"""
    log_n, log_l, n_polys = 10, 6, 129
    n = 1 << log_n
    three = [orc.rand_fr(0x8200 + i, n) for i in range(3)]
    single = opener(zkp, orc, log_n, log_l, 1, group_log)
    refs = [single.open_cosets(f, evals=True) for f in three]
    for i, f in enumerate(three):
        assert np.array_equal(refs[i][0][0], expected(orc, orc.fr_to_ints(f), log_n, log_l)[0][0]), i
    op = make_opener(zkp, srs(zkp, orc, n)[1], log_n, log_l, n_polys, group_log)
    (xy, inf), ev = op.open_cosets_batch(np.stack([three[p % 3] for p in range(n_polys)]), evals=True)
    op.close()
    bad = [p for p in range(n_polys) if not (xy[p].tobytes() == refs[p % 3][0][0].tobytes() and inf[p].tobytes() == refs[p % 3][0][1].tobytes() and
                                             ev[p].tobytes() == refs[p % 3][1].tobytes())]
    assert not bad, bad[:8]


def test_device_entry_stride_fewer_polynomials_and_a_second_call(zkp, orc):
    import torch
    log_n, log_l, max_polys, n_polys = 6, 3, 4, 3
    n, r, length = 64, 8, 41
    op = opener(zkp, orc, log_n, log_l, max_polys, 1)                                   # groups of 2: partial sums and a fold
    single = opener(zkp, orc, log_n, log_l, 1, 1)
    alone = orc.rand_fr(0x8300, n)
    d_xy1, d_inf1 = torch.zeros(r * 12, dtype=torch.int64, device="cuda"), torch.full((r,), 7, dtype=torch.uint8, device="cuda")
    op.open_cosets_dev(dev(alone), n, d_xy1, d_inf1)
    torch.cuda.synchronize()
    before = (host(d_xy1, (r, 12)).copy(), host(d_inf1, (r,)).copy())
    assert np.array_equal(before[0], expected(orc, orc.fr_to_ints(alone), log_n, log_l)[0][0])
    for call in range(2):                                                               # nothing of a call is left for the next
        rows = [row_ints(orc, 0x8310 + 8 * call + p, length, e) for p, e in enumerate((length, 9 + call, 30))]
        padded = np.full((n_polys, n, 4), 0xDEADBEEFDEADBEEF, dtype=np.uint64)           # stride = n > len, poison in the gap
        for p, f in enumerate(rows):
            padded[p, :length] = orc.fr_from_ints(f)
        d_xy = torch.zeros(n_polys * r * 12, dtype=torch.int64, device="cuda")
        d_inf = torch.full((n_polys * r,), 7, dtype=torch.uint8, device="cuda")
        d_ev = torch.full((n_polys * n * 4,), 5, dtype=torch.int64, device="cuda")
        op.open_cosets_batch_dev(dev(padded), n_polys, length, n, d_xy, d_inf, d_ev)
        torch.cuda.synchronize()
        got = (host(d_xy, (n_polys, r, 12)), host(d_inf, (n_polys, r)))
        check_rows(zkp, orc, got, host(d_ev, (n_polys, n, 4)), rows, log_n, log_l, single, call)
        op.open_cosets_batch_dev(dev(padded), n_polys, length, n, d_xy, d_inf)           # evaluations not asked for
        torch.cuda.synchronize()
        assert np.array_equal(host(d_xy, (n_polys, r, 12)), got[0])
    op.open_cosets_dev(dev(alone), n, d_xy1, d_inf1)                                    # one polynomial on the batch opener, as before
    torch.cuda.synchronize()
    assert host(d_xy1, (r, 12)).tobytes() == before[0].tobytes() and host(d_inf1, (r,)).tobytes() == before[1].tobytes()
    (sxy, sinf), _ = single.open_cosets(alone)
    assert sxy.tobytes() == before[0].tobytes() and sinf.tobytes() == before[1].tobytes()


def test_cells_of_a_batch_pass_the_cell_verifier_in_one_check(zkp, orc):
    log_n, log_l = 6, 3
    n, l, r = 64, 8, 8
    s = zkp.Srs.new_from_secret(orc.fr_from_ints([SECRET])[0], n)
    scheme = zkp.KzgScheme(s, expand_bases=False)
    polys = np.stack([orc.rand_fr(0x8400, n), orc.rand_fr(0x8401, n)])
    (pxy, pinf), ev = scheme.open_cosets_batch(polys, log_n, log_l, evals=True)
    assert list(scheme._coset_openers) == [(log_n, log_l)] and scheme._coset_openers[log_n, log_l].max_polys == 2
    again = scheme.open_cosets(polys[1], log_n, log_l)[0]                                # the kept opener serves one polynomial too
    assert again[0].tobytes() == pxy[1].tobytes()
    commits = [scheme.commit(polys[p]) for p in range(2)]
    commits = (np.stack([c[0] for c in commits]), np.array([c[1] for c in commits], dtype=np.uint8))
    g2_sl = zkp.g2_mul(zkp.g2_generator(), orc.fr_from_ints([pow(SECRET, l, R)])[0])[0]
    ci = np.repeat(np.arange(2, dtype=np.uint32), r)
    ki = np.tile(np.arange(r, dtype=np.uint32), 2)
    evals = np.stack([ev[p][k::r] for p in range(2) for k in range(r)])
    proofs = (pxy.reshape(2 * r, 12), pinf.reshape(2 * r))
    assert scheme.verify_cells(g2_sl, commits, ci, ki, evals, proofs, log_n, log_l)
    bad = evals.copy()
    bad[r + 2, 5] = orc.fr_add(bad[r + 2, 5][None], orc.fr_from_ints([1]))[0]
    assert not scheme.verify_cells(g2_sl, commits, ci, ki, bad, proofs, log_n, log_l), "one altered evaluation of the second polynomial"
    scheme.close()


def test_refusals(zkp, orc):
    """every refusal of the three entries, before anything is launched"""
    import torch
    E_ARG, E_SIZE, OK = zkp.ZKP_E_ARG, zkp.ZKP_E_SIZE, zkp.ZKP_OK
    xy, h = srs(zkp, orc, 64)
    create, handle = zkp.lib().zkp_kzg_opener_create_cosets_batch, zkp.C.c_void_p()
    assert create(None, 6, 3, 2, zkp.C.byref(handle)) == E_ARG and create(h._h, 6, 3, 2, None) == E_ARG                  # null
    for max_polys in (0, 4097, 1 << 40):
        assert create(h._h, 6, 3, max_polys, zkp.C.byref(handle)) == E_ARG and not handle.value, max_polys
        assert "max_polys" in last_error(zkp)
    for log_n, log_l in ((3, 3), (3, 4), (24, 6), (0, 0)):                                                                 # shape limits
        assert create(h._h, log_n, log_l, 2, zkp.C.byref(handle)) == E_ARG and not handle.value, (log_n, log_l)
    short = zkp.G1Bases.from_host(xy[:64 - 8 - 1])                                                                         # too few points
    assert create(short._h, 6, 3, 2, zkp.C.byref(handle)) == E_SIZE and not handle.value
    short.close()
    assert create(h._h, 6, 3, 4096, zkp.C.byref(handle)) == OK and handle.value                                            # the largest
    zkp.lib().zkp_kzg_opener_destroy(handle)

    op, single = opener(zkp, orc, 6, 3, 2), opener(zkp, orc, 6, 3, 1)
    coeffs = np.stack([orc.rand_fr(0x8500, 64), orc.rand_fr(0x8501, 64)])
    out_xy, out_inf = np.full((3, 8, 12), 9, dtype=np.uint64), np.full((3, 8), 9, dtype=np.uint8)
    fn = zkp.lib().zkp_kzg_open_cosets_batch
    args = lambda o=op, c=coeffs, polys=2, length=64, stride=64, x=out_xy, i=out_inf: (
        o._h if o is not None else None, c.ctypes.data if c is not None else None, polys, length, stride, x.ctypes.data if x is not None else None,
        i.ctypes.data if i is not None else None, None)
    for hole in ("o", "c", "x", "i"):
        assert fn(*args(**{hole: None})) == E_ARG, hole
    assert fn(*args(length=0, stride=0)) == E_ARG and fn(*args(length=0)) == E_ARG                                         # len == 0
    assert fn(*args(length=65, stride=65)) == E_SIZE                                                                       # len > n
    assert fn(*args(length=64, stride=63)) == E_ARG and "stride" in last_error(zkp)                                       # stride < len
    assert fn(*args(polys=3)) == E_SIZE and "3 polynomials" in last_error(zkp) and "made for 2" in last_error(zkp)       # n_polys > max_polys
    assert fn(*args(o=single, polys=2)) == E_SIZE and "made for 1" in last_error(zkp)
    assert (out_xy == 9).all() and (out_inf == 9).all(), "a refused call wrote its outputs"
    assert fn(*args(polys=0)) == OK and (out_xy == 9).all() and (out_inf == 9).all()                                       # an empty batch
    d = torch.zeros(8, dtype=torch.int64, device="cuda")                                                                   # the device entry
    dfn = zkp.lib().zkp_kzg_open_cosets_batch_dev
    p = zkp.C.c_void_p(d.data_ptr())
    assert dfn(None, p, 1, 1, 1, p, p, None, None) == E_ARG and dfn(op._h, None, 1, 1, 1, p, p, None, None) == E_ARG
    assert dfn(op._h, p, 1, 1, 1, None, p, None, None) == E_ARG and dfn(op._h, p, 1, 1, 1, p, None, None, None) == E_ARG
    assert dfn(op._h, p, 1, 0, 0, p, p, None, None) == E_ARG and dfn(op._h, p, 1, 65, 65, p, p, None, None) == E_SIZE
    assert dfn(op._h, p, 1, 2, 1, p, p, None, None) == E_ARG and dfn(op._h, p, 3, 1, 1, p, p, None, None) == E_SIZE
    assert dfn(op._h, p, 0, 1, 1, p, p, None, None) == OK
    torch.cuda.synchronize()
    assert not d.any().item()
    with pytest.raises(zkp.ZkpError) as ei:
        op.open_cosets_batch(np.zeros((3, 64, 4), dtype=np.uint64))
    assert ei.value.code == E_SIZE
    got, ev = op.open_cosets_batch(coeffs, evals=True)                                                                     # still usable
    check_rows(zkp, orc, got, ev, [orc.fr_to_ints(c) for c in coeffs], 6, 3, single, "after the refusals")
    got1, _ = op.open_cosets_batch(coeffs[:1])                                                                             # n_polys < max_polys
    assert got1[0][0].tobytes() == got[0][0].tobytes()


def test_creation_beyond_the_byte_budget_is_refused_and_leaves_nothing(zkp, orc):
    """ZKP_E_NOMEM through ZKP_KZG_OPENER_MAX_BYTES: a max_polys whose workspaces exceed the budget that max_polys - 1 fits in; the
    message names the kept slices, the per-call bytes and max_polys, and the device has as much free memory afterwards as before"""
    import torch
    n, l, r, max_polys = 64, 8, 8, 3
    _, h = srs(zkp, orc, n)
    kept = 512 * n
    per_poly = 512 * n + 768 * r + 64 * n                                                # group_log 0: partial sums, u and h, scalars
    total = lambda polys: kept + polys * per_poly + 256 * min(polys * 2 * n, 1 << 18)    # ... and the table
    assert total(1) == cm.sizes(n, l, 0)[-1]
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    os.environ[BUDGET] = str(total(max_polys) - 1)
    try:
        with pytest.raises(zkp.ZkpError) as ei:
            make_opener(zkp, h, 6, 3, max_polys, 0)
        after = torch.cuda.mem_get_info()[0]
        smaller = make_opener(zkp, h, 6, 3, max_polys - 1, 0)                            # the same budget holds a smaller batch
        os.environ[BUDGET] = str(total(max_polys))
        op = make_opener(zkp, h, 6, 3, max_polys, 0)
    finally:
        del os.environ[BUDGET]
    msg = str(ei.value)
    assert ei.value.code == zkp.ZKP_E_NOMEM
    assert f"workspaces of {total(max_polys)} bytes" in msg and f"{kept} kept slices + {total(max_polys) - kept} per call" in msg, msg
    assert f"max_polys {max_polys}" in msg and f"MAX_BYTES {total(max_polys) - 1}" in msg, msg
    assert after == before, (before, after)
    coeffs = np.stack([orc.rand_fr(0x8600 + p, n) for p in range(max_polys)])
    got = op.open_cosets_batch(coeffs)[0]
    for p in range(max_polys):
        assert np.array_equal(got[0][p], expected(orc, orc.fr_to_ints(coeffs[p]), 6, 3)[0][0]), p
    assert smaller.open_cosets_batch(coeffs[:2])[0][0].tobytes() == got[0][:2].tobytes()
    smaller.close()
    op.close()


def test_sharded_source_is_refused_in_a_child_process():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kzg_cosets_batch_worker.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "OK kzg cosets batch slots" in p.stdout
