"""GPU: evaluation-form KZG (zkp_kzg_eval_opener_*, zkp_kzg_commit_evals_batch*, zkp_kzg_open_evals_batch*,
zkp_kzg_open_evals_field_dev).  A row is a vector of values from orc.rand_fr; the reference is the coefficient-form opening the
library had before (kzg/src/scheme.rs:108-142): the oracle's inverse transform gives the coefficients, orc.poly_eval_fr and
orc.poly_div_linear_fr the value and the quotient, orc.ntt_fr the quotient's values, zkp.kzg_open / zkp.kzg_commit over the monomial
SRS the points.  Every comparison is exact: words of y and q, bytes of the points and their flags."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kzg_evals_model as em

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = em.R
SECRET = 0x1F2E3D4C5B6A7988
KNOB = "ZKP_KZG_EVALS_INVERSE"
BUDGET = "ZKP_KZG_EVALS_MAX_BYTES"

# n = 2 and n = 8 (short workgroups with idle lanes and partly filled chunks), then the edges of the plan: one size below the
# elements a workgroup inverts together, that number, two workgroups and two partial sums per row, four of them
SHAPES = [1, 3] + em.edge_log_ns()
BATCHES = [1, 2, 3, 5]
ROWS = max(BATCHES)
LARGER = 8  # a handle made for more rows than any batch of BATCHES


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, copy=True, order="C").view(np.int64 if a.dtype == np.uint64 else np.uint8)).cuda()


def host(t, shape):
    return t.cpu().numpy().view(np.uint64).reshape(shape)


def zeros(count):
    import torch
    return torch.zeros(4 * count, dtype=torch.int64, device="cuda")


def bitrev_rows(rows, log_n):
    """(P, n, 4) natural order -> the rows as a bit-reversed handle takes them"""
    idx = np.array([em.bitrev(i, log_n) for i in range(1 << log_n)])
    return np.ascontiguousarray(rows[:, idx])


_srs, _lagrange, _openers, _refs = {}, {}, {}, {}


def srs(zkp, orc, log_n):
    """the monomial SRS [s^i]G, i < n, as a handle, and [s]_2"""
    if log_n not in _srs:
        s = orc.fr_from_ints([SECRET])[0]
        _srs[log_n] = (zkp.G1Bases.from_host(zkp.srs_g1(s, 1 << log_n)), zkp.g2_mul(zkp.g2_generator(), s)[0])
    return _srs[log_n]


def lagrange(zkp, orc, log_n, mode="plain"):
    """the Lagrange basis of the domain: plain, expanded, or expanded for the endomorphism-split MSM"""
    if (log_n, mode) not in _lagrange:
        b = srs(zkp, orc, log_n)[0].lagrange(log_n)
        if mode != "plain":
            b.precompute(9, glv=mode == "split")
        _lagrange[log_n, mode] = b
    return _lagrange[log_n, mode]


def make_opener(zkp, bases, log_n, max_polys, bitrev):
    from zkp_hip import kzg_evals
    return kzg_evals.KzgEvalOpener(bases, log_n, max_polys, bitrev=bitrev)


def opener(zkp, orc, log_n, max_polys, bitrev, mode="plain"):
    key = (log_n, max_polys, bitrev, mode)
    if key not in _openers:
        _openers[key] = make_opener(zkp, lagrange(zkp, orc, log_n, mode), log_n, max_polys, bitrev)
    return _openers[key]


def with_knob(value, fn):
    old = os.environ.pop(KNOB, None)
    if value is not None:
        os.environ[KNOB] = str(value)
    try:
        return fn()
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


def reference(zkp, orc, values, z, log_n):
    """One row (canonical (n, 4) limbs in natural order) at one point: (y, the quotient's values, proof bytes, flag, commitment
    bytes, flag) by the coefficient form; computed once per (row, point)"""
    key = (values.tobytes(), z.tobytes())
    if key not in _refs:
        n = 1 << log_n
        mono = srs(zkp, orc, log_n)[0]
        coeffs = orc.ntt_fr(values, inverse=True)
        y = orc.poly_eval_fr(coeffs, z)
        quot = np.zeros((n, 4), dtype=np.uint64)
        quot[:n - 1] = orc.poly_div_linear_fr(coeffs, z)
        (pxy, pinf), ev = zkp.kzg_open(mono, coeffs, z)
        assert np.array_equal(ev, y)
        cxy, cinf = zkp.kzg_commit(mono, coeffs)
        _refs[key] = (y, orc.ntt_fr(quot), pxy.tobytes(), pinf, cxy.tobytes(), cinf)
    return _refs[key]


def standard_rows(orc, log_n):
    """ROWS random rows and a point outside the domain for each, never changed"""
    n = 1 << log_n
    rows = orc.rand_fr(0xE7A0 + log_n, ROWS * n).reshape(ROWS, n, 4)
    zs = orc.rand_fr(0xE7B0 + log_n, ROWS)
    rows.setflags(write=False)
    zs.setflags(write=False)
    return rows, zs


def check_open(zkp, orc, got, rows, zs, log_n, where):
    """(proofs, flags), y of a call against the reference of every row (rows canonical, natural order)"""
    (xy, inf), y = got
    for p in range(rows.shape[0]):
        ry, _, pxy, pinf, _, _ = reference(zkp, orc, rows[p], zs[p], log_n)
        assert np.array_equal(y[p], ry), (where, p, "y")
        assert xy[p].tobytes() == pxy and inf[p] == pinf, (where, p, "proof")
        if pinf:
            assert not xy[p].any(), (where, p, "the identity has zero limbs")


def check_field(zkp, orc, op, sent, rows, zs, log_n, where):
    polys, n = rows.shape[0], 1 << log_n
    d_y, d_q = zeros(polys), zeros(polys * n)
    op.field_dev(dev(sent), polys, dev(zs), d_y, d_q)
    y, q = host(d_y, (polys, 4)), host(d_q, (polys, n, 4))
    for p in range(polys):
        ry, rq = reference(zkp, orc, rows[p], zs[p], log_n)[:2]
        assert np.array_equal(y[p], ry), (where, p, "y")
        assert np.array_equal(q[p], rq), (where, p, "q", np.nonzero((q[p] != rq).any(axis=1))[0][:8])


@pytest.mark.parametrize("log_n", SHAPES)
def test_field_half_proofs_and_commitments_are_exact(zkp, orc, log_n):
    rows, zs = standard_rows(orc, log_n)
    for polys in BATCHES:
        for bitrev in (False, True):
            sent = bitrev_rows(rows[:polys], log_n) if bitrev else rows[:polys]
            for max_polys in (polys, LARGER):
                where = (log_n, polys, bitrev, max_polys)
                op = opener(zkp, orc, log_n, max_polys, bitrev)
                check_field(zkp, orc, op, sent, rows[:polys], zs[:polys], log_n, where)
                check_open(zkp, orc, op.open_batch(sent, zs[:polys]), rows[:polys], zs[:polys], log_n, where)
                cxy, cinf = op.commit_batch(sent)
                for p in range(polys):
                    ref = reference(zkp, orc, rows[p], zs[p], log_n)
                    assert cxy[p].tobytes() == ref[4] and cinf[p] == ref[5], (where, p, "commitment")
            # the same bytes with the rows resident
            op = opener(zkp, orc, log_n, LARGER, bitrev)
            check_open(zkp, orc, op.open_batch_dev(dev(sent), polys, dev(zs[:polys])), rows[:polys], zs[:polys], log_n, (log_n, polys, bitrev, "dev"))
            dxy, dinf = op.commit_batch_dev(dev(sent), polys)
            assert dxy.tobytes() == cxy.tobytes() and dinf.tobytes() == cinf.tobytes()


def edge_batch(orc, log_n):
    """Ordinary rows mixed with: z = w^0, w^(n-1), w^(n/2), z = 0, two rows with the same z, the all-zero row, a constant row, and a
    row whose limbs are not canonical -> (the rows as sent, their canonical values, the points)"""
    n = 1 << log_n
    w = em.root(log_n)
    base, zs = standard_rows(orc, log_n)
    rnd = orc.rand_fr(0xE7C0 + log_n, 4 * n).reshape(4, n, 4)
    const = np.repeat(orc.rand_fr(0xE7D0 + log_n, 1), n, axis=0)
    rows = np.stack([base[0], rnd[0], rnd[1], base[1], rnd[2], rnd[3], base[2], np.zeros((n, 4), dtype=np.uint64), const, base[3], base[4]])
    in_domain = orc.fr_from_ints([1, pow(w, n - 1, R), pow(w, n // 2, R), 0])
    points = np.stack([zs[0], in_domain[0], in_domain[1], zs[1], in_domain[2], in_domain[3], zs[1], zs[2], in_domain[2], zs[3], zs[4]])
    sent = rows.copy()
    r_limbs = np.array([(R >> (64 * k)) & 0xffffffffffffffff for k in range(4)], dtype=object)
    bumped = []
    for v in rows[9]:  # base[3] + r in every element: below 2^256, not canonical
        total = sum(int(v[k]) << (64 * k) for k in range(4)) + sum(int(r_limbs[k]) << (64 * k) for k in range(4))
        assert total < 1 << 256
        bumped.append([(total >> (64 * k)) & 0xffffffffffffffff for k in range(4)])
    sent[9] = np.array(bumped, dtype=np.uint64)
    return sent, rows, points


@pytest.mark.parametrize("log_n", [3, em.edge_log_ns()[2]])
@pytest.mark.parametrize("bitrev", [False, True])
def test_edge_rows_mixed_with_ordinary_ones(zkp, orc, log_n, bitrev):
    sent, rows, points = edge_batch(orc, log_n)
    polys = rows.shape[0]
    if bitrev:
        sent = bitrev_rows(sent, log_n)
    op = opener(zkp, orc, log_n, polys, bitrev)
    check_field(zkp, orc, op, sent, rows, points, log_n, (log_n, bitrev, "edges"))
    got = op.open_batch(sent, points)
    check_open(zkp, orc, got, rows, points, log_n, (log_n, bitrev, "edges"))
    (xy, inf), y = got
    assert inf[7] == 1 and inf[8] == 1 and not xy[7].any() and not xy[8].any()  # the zero and the constant row: the identity
    assert not y[7].any() and np.array_equal(y[8], rows[8][0])
    assert np.array_equal(y[1], rows[1][0]) and np.array_equal(y[4], rows[4][(1 << log_n) // 2])  # f at w^0, at w^(n/2)
    cxy, cinf = op.commit_batch(sent)
    for p in range(polys):
        ref = reference(zkp, orc, rows[p], points[p], log_n)
        assert cxy[p].tobytes() == ref[4] and cinf[p] == ref[5], (p, "commitment")
    assert cinf[7] == 1 and not cxy[7].any()


def test_both_inversions_give_identical_bytes(zkp, orc):
    log_n = em.edge_log_ns()[2]
    sent, rows, points = edge_batch(orc, log_n)
    op = opener(zkp, orc, log_n, rows.shape[0], False)
    got = [with_knob(v, lambda: op.open_batch(sent, points)) for v in (0, 1, None)]
    for (xy, inf), y in got:
        check_open(zkp, orc, ((xy, inf), y), rows, points, log_n, "knob")
    for v in (0, 1):
        with_knob(v, lambda: check_field(zkp, orc, op, sent, rows, points, log_n, ("knob", v)))


@pytest.mark.parametrize("mode,polys", [("plain", 65), ("split", 33), ("expanded", 65)])
def test_msm_group_boundary(zkp, orc, mode, polys):
    """One row more than a pass of the batched MSM takes: 64 rows over a plain or expanded handle, 32 over an endomorphism-split one"""
    c = em.plan_constants()
    assert polys == (c["msm_group_split"] if mode == "split" else c["msm_group"]) + 1
    log_n, n = 4, 16
    rows = orc.rand_fr(0xE7E0, polys * n).reshape(polys, n, 4)
    zs = orc.rand_fr(0xE7E1, polys)
    zs[polys - 1] = orc.fr_from_ints([pow(em.root(log_n), 5, R)])[0]  # the row alone in the last group has its z in the domain
    op = opener(zkp, orc, log_n, polys, False, mode)
    check_open(zkp, orc, op.open_batch(rows, zs), rows, zs, log_n, mode)
    cxy, cinf = op.commit_batch(rows)
    for p in range(polys):
        ref = reference(zkp, orc, rows[p], zs[p], log_n)
        assert cxy[p].tobytes() == ref[4] and cinf[p] == ref[5], (mode, p)


def test_round_trips_through_the_verifiers(zkp, orc):
    log_n = 3
    sent, rows, points = edge_batch(orc, log_n)
    op = opener(zkp, orc, log_n, rows.shape[0], False)
    g2s = srs(zkp, orc, log_n)[1]
    (pxy, pinf), y = op.open_batch(sent, points)
    cxy, cinf = op.commit_batch(sent)
    one = orc.fr_from_ints([1])
    for p in range(rows.shape[0]):
        assert zkp.kzg_verify(g2s, (cxy[p], cinf[p]), (pxy[p], pinf[p]), y[p], points[p]), p
        assert not zkp.kzg_verify(g2s, (cxy[p], cinf[p]), (pxy[p], pinf[p]), orc.fr_add(y[p].reshape(1, 4), one)[0], points[p]), p
    finite = [p for p in range(rows.shape[0]) if not pinf[p] and not cinf[p]]
    assert len(finite) >= 8
    weights = orc.rand_fr(0xE7F0, len(finite))
    assert zkp.kzg_batch_verify(g2s, cxy[finite], points[finite], pxy[finite], y[finite], weights)


def test_device_calls_queued_back_to_back(zkp, orc):
    """Field calls with different P on one handle and one stream, read afterwards: a later call reuses the handle's workspace"""
    import torch
    log_n = em.edge_log_ns()[2]
    n = 1 << log_n
    rows, zs = standard_rows(orc, log_n)
    op = opener(zkp, orc, log_n, LARGER, True)
    sent = bitrev_rows(rows, log_n)
    outs = []
    for polys in (5, 2, 3, 1):
        d_y, d_q = zeros(polys), zeros(polys * n)
        op.field_dev(dev(sent[ROWS - polys:]), polys, dev(zs[ROWS - polys:]), d_y, d_q)
        outs.append((polys, d_y, d_q))
    torch.cuda.synchronize()
    for polys, d_y, d_q in outs:
        y, q = host(d_y, (polys, 4)), host(d_q, (polys, n, 4))
        for k in range(polys):
            p = ROWS - polys + k
            ry, rq = reference(zkp, orc, rows[p], zs[p], log_n)[:2]
            assert np.array_equal(y[k], ry) and np.array_equal(q[k], rq), (polys, k)


def test_refusals_launch_nothing_and_leave_the_handle_usable(zkp, orc):
    import torch
    log_n, n = 3, 8
    lag = lagrange(zkp, orc, log_n)
    C, L = zkp.C, zkp.lib()
    h = C.c_void_p()

    def refused(code, text, *args):
        assert L.zkp_kzg_eval_opener_create(*args, C.byref(h)) == code and not h.value
        assert text in L.zkp_last_error().decode(), L.zkp_last_error().decode()

    refused(zkp.ZKP_E_ARG, "null argument", None, log_n, 0, 1)
    assert L.zkp_kzg_eval_opener_create(lag._h, log_n, 0, 1, None) == zkp.ZKP_E_ARG
    refused(zkp.ZKP_E_ARG, "1 <= log_n <= 24", lag._h, 0, 0, 1)
    refused(zkp.ZKP_E_ARG, "1 <= log_n <= 24", lag._h, 25, 0, 1)
    refused(zkp.ZKP_E_ARG, "order 2 is neither", lag._h, log_n, 2, 1)
    refused(zkp.ZKP_E_ARG, "1 .. 4096 polynomials", lag._h, log_n, 0, 0)
    refused(zkp.ZKP_E_ARG, "1 .. 4096 polynomials", lag._h, log_n, 0, 4097)
    refused(zkp.ZKP_E_SIZE, "8 points, fewer than 2^log_n = 16", lag._h, 4, 0, 1)

    rows, zs = standard_rows(orc, log_n)
    op = opener(zkp, orc, log_n, 3, False)
    xy, inf, y = np.full((4, 12), 7, dtype=np.uint64), np.full(4, 7, dtype=np.uint8), np.full((4, 4), 7, dtype=np.uint64)
    d_rows, d_zs = dev(rows[:4]), dev(zs[:4])
    d_y, d_q = torch.full((16,), 7, dtype=torch.int64, device="cuda"), torch.full((4 * n * 4,), 7, dtype=torch.int64, device="cuda")
    p = lambda a: a.ctypes.data
    t = lambda x: C.c_void_p(x.data_ptr())
    rows4 = rows[:4].copy()
    calls = {
        "open": lambda k: L.zkp_kzg_open_evals_batch(op._h, p(rows4), k, p(zs), p(xy), p(inf), p(y)),
        "open_dev": lambda k: L.zkp_kzg_open_evals_batch_dev(op._h, t(d_rows), k, t(d_zs), None, p(xy), p(inf), p(y)),
        "commit": lambda k: L.zkp_kzg_commit_evals_batch(op._h, p(rows4), k, p(xy), p(inf)),
        "commit_dev": lambda k: L.zkp_kzg_commit_evals_batch_dev(op._h, t(d_rows), k, None, p(xy), p(inf)),
        "field": lambda k: L.zkp_kzg_open_evals_field_dev(op._h, t(d_rows), k, t(d_zs), t(d_y), t(d_q), None),
    }
    for name, call in calls.items():
        assert call(4) == zkp.ZKP_E_SIZE, name
        msg = L.zkp_last_error().decode()
        assert "a batch of 4 polynomials on an opener made for 3" in msg, (name, msg)
        assert call(0) == zkp.ZKP_OK, name  # an empty batch: nothing to do
    assert L.zkp_kzg_open_evals_batch(op._h, None, 2, p(zs), p(xy), p(inf), p(y)) == zkp.ZKP_E_ARG
    assert L.zkp_kzg_open_evals_batch_dev(op._h, t(d_rows), 2, None, None, p(xy), p(inf), p(y)) == zkp.ZKP_E_ARG
    assert L.zkp_kzg_commit_evals_batch(op._h, None, 2, p(xy), p(inf)) == zkp.ZKP_E_ARG
    assert L.zkp_kzg_commit_evals_batch_dev(op._h, t(d_rows), 2, None, None, p(inf)) == zkp.ZKP_E_ARG
    assert L.zkp_kzg_open_evals_field_dev(op._h, t(d_rows), 2, t(d_zs), None, t(d_q), None) == zkp.ZKP_E_ARG
    assert L.zkp_last_error().decode() == "null argument"
    torch.cuda.synchronize()
    assert (xy == 7).all() and (inf == 7).all() and (y == 7).all() and (d_y.cpu() == 7).all() and (d_q.cpu() == 7).all()
    check_open(zkp, orc, op.open_batch(rows[:3], zs[:3]), rows[:3], zs[:3], log_n, "after the refusals")


def test_creation_beyond_the_byte_budget_is_refused_and_leaves_nothing(zkp, orc):
    import torch
    log_n, max_polys = 6, 5
    n = 1 << log_n
    opener(zkp, orc, log_n, max_polys, False)  # (whatever the slot builds once for this shape is built)
    blocks = 1  # n is below a workgroup's span
    total = 32 * n + 2 * 32 * n * max_polys + 2 * 32 * blocks * max_polys + 32 * max_polys + 4 * max_polys
    total = (total + 31) // 32 * 32
    bases = lagrange(zkp, orc, log_n)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    os.environ[BUDGET] = str(total - 1)
    try:
        with pytest.raises(zkp.ZkpError) as ei:
            make_opener(zkp, bases, log_n, max_polys, False)
        after = torch.cuda.mem_get_info()[0]
        os.environ[BUDGET] = str(total)
        op = make_opener(zkp, bases, log_n, max_polys, False)
    finally:
        del os.environ[BUDGET]
    msg = str(ei.value)
    assert ei.value.code == zkp.ZKP_E_NOMEM
    assert f"workspace of {total} bytes" in msg and f"max_polys {max_polys}" in msg and f"MAX_BYTES {total - 1}" in msg and "bytes free" in msg, msg
    assert after == before, (before, after)
    rows, zs = standard_rows(orc, log_n)
    check_open(zkp, orc, op.open_batch(rows, zs), rows, zs, log_n, "at the budget")
    op.close()
    op.close()


def test_kzg_scheme_commit_and_open_evals_batch(zkp, orc):
    log_n, n = 4, 16
    s = zkp.Srs.new_from_secret(orc.fr_from_ints([SECRET])[0], n)
    scheme = zkp.KzgScheme(s, expand_bases=False)
    rows, zs = standard_rows(orc, log_n)

    def check(polys, bitrev):
        sent = bitrev_rows(rows[:polys], log_n) if bitrev else rows[:polys]
        (pxy, pinf), y = scheme.open_evals_batch(sent, zs[:polys], log_n, bitrev=bitrev)
        cxy, cinf = scheme.commit_evals_batch(sent, log_n, bitrev=bitrev)
        for p in range(polys):
            coeffs = orc.ntt_fr(rows[p], inverse=True)
            (exy, einf), ev = scheme.open(coeffs, zs[p])
            assert pxy[p].tobytes() == exy.tobytes() and pinf[p] == einf and np.array_equal(y[p], ev), (polys, bitrev, p)
            ecxy, ecinf = scheme.commit(coeffs)
            assert cxy[p].tobytes() == ecxy.tobytes() and cinf[p] == ecinf

    check(2, False)
    first = scheme._eval_openers[log_n, False]
    assert first.max_polys == 2
    check(1, False)
    assert scheme._eval_openers[log_n, False] is first
    check(3, False)  # a batch that outgrows the kept opener replaces it
    assert scheme._eval_openers[log_n, False].max_polys == 3 and scheme._eval_openers[log_n, False] is not first and first._h is None
    check(2, True)
    assert sorted(scheme._eval_openers) == [(log_n, False), (log_n, True)] and list(scheme._lagrange) == [log_n]
    kept = list(scheme._eval_openers.values()) + list(scheme._lagrange.values())
    scheme.close()
    assert scheme._eval_openers == {} and scheme._lagrange == {} and all(k._h is None for k in kept)
    scheme.close()


def test_opener_on_the_second_slot_in_a_child_process():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kzg_open_evals_worker.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "OK kzg open evals slots" in p.stdout
