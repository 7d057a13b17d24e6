"""GPU: cell recovery of a batch (zkp_kzg_recoverer_create_batch, zkp_kzg_recover_cosets_batch*).  Row p is a polynomial f_p from
orc.rand_fr with its evaluations from orc.ntt_fr; all rows miss the same cosets, and the missing positions hold bytes that are no
field element and differ between rows.  Every result is exact: the coefficients equal f_p, the evaluations the oracle's in the
requested layout, and every row is byte for byte what zkp_kzg_recover_cosets returns for it on a recoverer made for one."""
import os
import random
import subprocess
import sys

import numpy as np
import pytest

import kzg_recover_model as km

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNOB = "ZKP_KZG_RECOVER_LEAF_LOG"
BUDGET = "ZKP_KZG_RECOVER_MAX_BYTES"
SECRET = 0x1F2E3D4C5B6A7988
NATURAL, CELLS = 0, 1

# r = 2; l = 1 (the transposition is the identity); small; the practical cell at small n; r = 1024 with a two-pass transform of n
SHAPES = [(2, 1), (6, 0), (6, 3), (10, 6), (12, 2)]
LARGER = 8  # a handle made for more rows than any batch of BATCHES: two groups of rows, vec larger than the call uses
BATCHES = [1, 2, 3, 5]


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
    return t.cpu().numpy().view(np.uint64).reshape(shape)


def make_recoverer(zkp, log_n, log_l, max_polys, leaf_log=None):
    old = os.environ.pop(KNOB, None)
    if leaf_log is not None:
        os.environ[KNOB] = str(leaf_log)
    try:
        return zkp.KzgRecoverer(log_n, log_l, max_polys)
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


_recoverers, _polys, _single = {}, {}, {}


def recoverer(zkp, log_n, log_l, max_polys=1, leaf_log=None):
    key = (log_n, log_l, max_polys, leaf_log)
    if key not in _recoverers:
        _recoverers[key] = make_recoverer(zkp, log_n, log_l, max_polys, leaf_log)
    return _recoverers[key]


def poly(orc, log_n, length, p):
    """(f_p, its evaluations on the domain): computed once, never changed"""
    key = (log_n, length, p)
    if key not in _polys:
        n = 1 << log_n
        f = orc.rand_fr(0x7A00 + 65536 * p + 4096 * log_n + length, length)
        padded = np.zeros((n, 4), dtype=np.uint64)
        padded[:length] = f
        ev = orc.ntt_fr(padded)
        f.setflags(write=False)
        ev.setflags(write=False)
        _polys[key] = (f, ev)
    return _polys[key]


def rows_of(orc, log_n, length, polys):
    """((P, length, 4) coefficients, (P, n, 4) evaluations in natural order) of the rows 0 .. P - 1"""
    got = [poly(orc, log_n, length, p) for p in range(polys)]
    return np.stack([f for f, _ in got]), np.stack([ev for _, ev in got])


def mask_of(r, missing):
    present = np.ones(r, dtype=np.uint8)
    present[list(missing)] = 0
    return present


def given(ev, present):
    """natural-order rows with bytes 0xFF - p (no field element) at the positions of row p's missing cosets"""
    r = present.shape[0]
    out = ev.copy()
    gone = np.tile(present == 0, ev.shape[1] // r)
    for p in range(out.shape[0]):
        out[p][gone] = np.frombuffer(bytes([0xFF - p % 16]) * 8, dtype=np.uint64)[0]
    return out


def to_cells(rows, r):
    """(P, n, 4) natural order -> (P, r, l, 4): cell k of a row holds the values k + j r"""
    polys, n = rows.shape[0], rows.shape[1]
    return np.ascontiguousarray(rows.reshape(polys, n // r, r, 4).transpose(0, 2, 1, 3))


def lengths(n, l, r, m):
    return sorted({x for x in (1, l + 1, n // 2, (r - m) * l) if 1 <= x <= (r - m) * l})


def missing_sets(r, rng):
    return {"none": set(), "first": {0}, "first half": set(range(r // 2)), "every other": set(range(0, r, 2)),
            "random": set(rng.sample(range(r), rng.randint(1, r - 1)))}


def single_rows(zkp, orc, log_n, log_l, name, missing, length, polys):
    """what zkp_kzg_recover_cosets returns for each row, on a recoverer made for one: [(coefficients, evaluations)], kept"""
    r = 1 << (log_n - log_l)
    present = mask_of(r, missing)
    _, ev = rows_of(orc, log_n, length, polys)
    sent = given(ev, present)
    out = []
    for p in range(polys):
        key = (log_n, log_l, name, length, p)
        if key not in _single:
            coeffs, out_ev, ok = recoverer(zkp, log_n, log_l).recover(sent[p], present, length, want_evals=True)
            assert ok, key
            _single[key] = (coeffs.tobytes(), out_ev.tobytes())
        out.append(_single[key])
    return out


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_rows_equal_the_single_entry_and_the_oracle(zkp, orc, log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    rng = random.Random(0x7B00 + 64 * log_n + log_l)
    sets = missing_sets(r, rng)
    calls = layouts = 0
    for polys in BATCHES:
        # (the larger handle's tree has levels at every shape with r >= 4: leaves of two factors)
        for rc in (recoverer(zkp, log_n, log_l, polys), recoverer(zkp, log_n, log_l, LARGER, 1)):
            todo = [(name, missing, length) for name, missing in sets.items() for length in lengths(n, l, r, len(missing))]
            for length in (1, l + 1, n // 2):  # "most": the largest admissible m for the length
                most = r - (length + l - 1) // l
                if 1 <= most and length <= n:
                    todo.append(("most of %d" % length, set(random.Random(length).sample(range(r), most)), length))
            for name, missing, length in todo:
                present = mask_of(r, missing)
                f, ev = rows_of(orc, log_n, length, polys)
                ref = single_rows(zkp, orc, log_n, log_l, name, missing, length, polys)
                sent = given(ev, present)
                # both layouts on the handle made for exactly this batch, alternating on the larger one
                for layout in ((NATURAL, CELLS) if rc.max_polys == polys else (calls % 2,)):
                    cells = layout == CELLS
                    coeffs, out_ev, ok = rc.recover_batch(to_cells(sent, r) if cells else sent, present, length, want_evals=True, cells=cells)
                    where = (name, length, polys, rc.max_polys, layout)
                    assert ok.shape == (polys,) and ok.all(), where
                    assert np.array_equal(coeffs, f), where
                    assert np.array_equal(out_ev, to_cells(ev, r) if cells else ev), where
                    back = out_ev.transpose(0, 2, 1, 3).reshape(polys, n, 4) if cells else out_ev
                    for p in range(polys):
                        assert coeffs[p].tobytes() == ref[p][0] and np.ascontiguousarray(back[p]).tobytes() == ref[p][1], (where, p)
                    calls += 1
                    layouts |= 1 << layout
    assert calls >= 100 and layouts == 3


def test_both_sides_of_the_plan_switch_on_one_handle(zkp, orc):
    """512 rows of 2^10 are 2^19 elements, where the transforms of n take the other plan; 511 stay below it"""
    log_n, log_l = 10, 6
    n, l, r = 1024, 64, 16
    rc = recoverer(zkp, log_n, log_l, 512)
    single = recoverer(zkp, log_n, log_l)
    present = mask_of(r, set(range(0, r, 2)))
    length = n // 2  # exactly enough: any row of field elements is consistent
    rows = orc.rand_fr(0x7C00, 512 * n).reshape(512, n, 4)
    for p in (0, 255, 510, 511):
        rows[p] = poly(orc, log_n, length, p)[1]
    sent = given(rows, present)
    for polys, cells in ((512, False), (511, True)):
        coeffs, out_ev, ok = rc.recover_batch(to_cells(sent[:polys], r) if cells else sent[:polys], present, length, want_evals=True, cells=cells)
        assert ok.all()
        back = out_ev.transpose(0, 2, 1, 3).reshape(polys, n, 4) if cells else out_ev
        for p in (0, 255, polys - 1):
            ref, ref_ev, ref_ok = single.recover(sent[p], present, length, want_evals=True)
            assert ref_ok and coeffs[p].tobytes() == ref.tobytes() and np.ascontiguousarray(back[p]).tobytes() == ref_ev.tobytes(), (polys, p)
            assert np.array_equal(coeffs[p], poly(orc, log_n, length, p)[0]), (polys, p)


@pytest.mark.parametrize("log_n,log_l", [(6, 3), (10, 6)])
def test_one_bad_row_does_not_taint_its_neighbours(zkp, orc, log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    rng = random.Random(0x7D00 + log_n)
    rc = recoverer(zkp, log_n, log_l, 3)
    missing = set(rng.sample(range(r), r // 4))
    present = mask_of(r, missing)
    length = (r - len(missing)) * l - l  # one cell more than needed
    f, ev = rows_of(orc, log_n, length, 3)
    good = given(ev, present)
    at = rng.choice([i for i in range(n) if present[i % r]])
    for bad_row, cells in ((1, False), (0, False), (2, False), (1, True)):
        sent = good.copy()
        sent[bad_row][at] = ev[bad_row][(at + 1) % n]
        assert not np.array_equal(sent[bad_row][at], ev[bad_row][at])
        coeffs, out_ev, ok = rc.recover_batch(to_cells(sent, r) if cells else sent, present, length, want_evals=True, cells=cells)
        assert ok.tolist() == [p != bad_row for p in range(3)], (bad_row, cells)
        for p in range(3):
            if p != bad_row:
                assert np.array_equal(coeffs[p], f[p]) and np.array_equal(out_ev[p], to_cells(ev, r)[p] if cells else ev[p]), (bad_row, cells, p)


def test_stride_feeds_the_batched_opener_and_the_cell_verifier(zkp, orc):
    import torch
    log_n, log_l = 4, 2
    n, l, r = 16, 4, 4
    polys, length = 3, 7
    stride = length + 3
    s = zkp.Srs.new_from_secret(orc.fr_from_ints([SECRET])[0], n)
    rc = recoverer(zkp, log_n, log_l, polys)
    op = zkp.KzgOpener(s.bases, log_n, log_l, polys)
    f, ev = rows_of(orc, log_n, length, polys)
    present = mask_of(r, {1, 2})
    sentinel = -0x0123456789ABCDEF
    d_coeffs = torch.full(((polys * stride + 5) * 4,), sentinel, dtype=torch.int64, device="cuda")
    d_ev = torch.zeros(polys * n * 4, dtype=torch.int64, device="cuda")
    d_flags = torch.full((polys,), 7, dtype=torch.int32, device="cuda")
    rc.recover_batch_dev(dev(to_cells(given(ev, present), r)), polys, present, length, stride, d_coeffs, d_flags, d_ev, cells=True)
    d_xy = torch.zeros(polys * r * 12, dtype=torch.int64, device="cuda")
    d_inf = torch.zeros(polys * r, dtype=torch.uint8, device="cuda")
    op.open_cosets_batch_dev(d_coeffs, polys, length, stride, d_xy, d_inf)  # the same buffer, the same stride
    torch.cuda.synchronize()
    assert d_flags.cpu().tolist() == [0, 0, 0]
    got = d_coeffs.cpu().numpy().view(np.uint64).reshape(-1, 4)
    want = np.full_like(got, np.int64(sentinel).astype(np.uint64))
    for p in range(polys):
        want[p * stride:p * stride + length] = f[p]
    assert np.array_equal(got, want)  # the gaps and what lies behind the last row keep the sentinel
    (exp_xy, exp_inf), _ = op.open_cosets_batch(f)
    xy, inf = host(d_xy, (polys, r, 12)), d_inf.cpu().numpy().reshape(polys, r)
    assert np.array_equal(xy, exp_xy) and np.array_equal(inf, exp_inf)
    cell_ev = host(d_ev, (polys, r, l, 4))
    assert np.array_equal(cell_ev, to_cells(ev, r))
    # every recovered cell with its proof, as the verifier takes them
    commits = [zkp.kzg_commit(s.bases, f[p]) for p in range(polys)]
    commitments = (np.stack([c for c, _ in commits]), np.array([i for _, i in commits], dtype=np.uint8))
    g2_sl, _ = zkp.g2_mul(zkp.g2_generator(), orc.fr_from_ints([pow(SECRET, l, km.R)])[0])
    ver = zkp.KzgCellVerifier(s.bases, g2_sl, log_n, log_l, polys * r, polys)
    ci = np.repeat(np.arange(polys, dtype=np.uint32), r)
    ki = np.tile(np.arange(r, dtype=np.uint32), polys)
    wt = orc.fr_from_ints([random.Random(0x7E00 + i).randrange(1 << 128) for i in range(polys * r)])
    flat = cell_ev.reshape(polys * r, l, 4)
    assert ver.verify(commitments, ci, ki, flat, (xy.reshape(-1, 12), inf.reshape(-1)), wt)
    swapped = flat.copy()
    swapped[[1, 2]] = swapped[[2, 1]]
    assert not ver.verify(commitments, ci, ki, swapped, (xy.reshape(-1, 12), inf.reshape(-1)), wt)
    ver.close()
    op.close()


def test_device_calls_queued_back_to_back(zkp, orc):
    import torch
    log_n, log_l = 10, 6
    n, r = 1 << log_n, 1 << (log_n - log_l)
    rc = recoverer(zkp, log_n, log_l, LARGER, 1)
    rng = random.Random(0x7F00)
    plans = [(5, set(rng.sample(range(r), 8)), n // 2, CELLS), (2, set(), n, NATURAL), (8, {3}, 65, CELLS), (3, set(rng.sample(range(r), 5)), 100, NATURAL)]
    queued = []
    for polys, missing, length, layout in plans:  # queued back to back, read afterwards: nothing of one call is left for the next
        present = mask_of(r, missing)
        f, ev = rows_of(orc, log_n, length, polys)
        sent = given(ev, present)
        d_out = torch.zeros(polys * length * 4, dtype=torch.int64, device="cuda")
        d_ev = torch.zeros(polys * n * 4, dtype=torch.int64, device="cuda")
        d_flags = torch.full((polys,), 7, dtype=torch.int32, device="cuda")
        rc.recover_batch_dev(dev(to_cells(sent, r) if layout == CELLS else sent), polys, present, length, length, d_out, d_flags, d_ev, cells=layout)
        present[:] = 0  # read before the call returned
        queued.append((f, to_cells(ev, r) if layout == CELLS else ev, d_out, d_ev, d_flags, polys, length))
    torch.cuda.synchronize()
    for f, ev, d_out, d_ev, d_flags, polys, length in queued:
        assert d_flags.cpu().tolist() == [0] * polys
        assert np.array_equal(host(d_out, (polys, length, 4)), f) and np.array_equal(host(d_ev, ev.shape), ev), (polys, length)
    polys, missing, length, _ = plans[0]
    present = mask_of(r, missing)
    f, ev = poly(orc, log_n, length, 0)
    d_out, d_flag = torch.zeros(length * 4, dtype=torch.int64, device="cuda"), torch.full((1,), 7, dtype=torch.int32, device="cuda")
    rc.recover_dev(dev(given(ev[None], present)[0]), present, length, d_out, d_flag)  # a single call on the handle of a batch
    torch.cuda.synchronize()
    assert int(d_flag.item()) == 0 and np.array_equal(host(d_out, (length, 4)), f)


def test_refusals(zkp, orc):
    import torch
    log_n, log_l = 6, 3
    n, l, r = 64, 8, 8
    for max_polys in (0, 4097):
        handle = zkp.C.c_void_p()
        assert zkp.lib().zkp_kzg_recoverer_create_batch(log_n, log_l, max_polys, zkp.C.byref(handle)) == zkp.ZKP_E_ARG, max_polys
        assert not handle.value
    handle = zkp.C.c_void_p()
    assert zkp.lib().zkp_kzg_recoverer_create_batch(3, 3, 2, zkp.C.byref(handle)) == zkp.ZKP_E_ARG and not handle.value
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.KzgRecoverer(log_n, log_l, 4097)
    assert ei.value.code == zkp.ZKP_E_ARG
    rc = recoverer(zkp, log_n, log_l, 3)
    f, ev = rows_of(orc, log_n, 17, 3)
    present = mask_of(r, {0, 5})
    sent = given(ev, present)

    def still_usable():
        coeffs, _, ok = rc.recover_batch(sent, present, 17)
        assert ok.all() and np.array_equal(coeffs, f)
        one, _, ok1 = rc.recover(sent[1], present, 17)  # a handle of any max_polys serves the single entries
        assert ok1 and np.array_equal(one, f[1])

    still_usable()
    four = np.concatenate([sent, sent[:1]])
    with pytest.raises(zkp.ZkpError) as ei:
        rc.recover_batch(four, present, 17)
    assert ei.value.code == zkp.ZKP_E_SIZE and "4 polynomials" in str(ei.value) and "made for 3" in str(ei.value), str(ei.value)
    still_usable()
    # the single entry's own refusals, through the batch entry
    with pytest.raises(zkp.ZkpError) as ei:
        rc.recover_batch(sent, present, 0)
    assert ei.value.code == zkp.ZKP_E_ARG
    with pytest.raises(zkp.ZkpError) as ei:
        rc.recover_batch(sent, present, n + 1)
    assert ei.value.code == zkp.ZKP_E_SIZE
    with pytest.raises(zkp.ZkpError) as ei:  # 6 cells of 8 points do not give 49 coefficients
        rc.recover_batch(sent, present, 6 * l + 1)
    assert ei.value.code == zkp.ZKP_E_SIZE
    assert "6 present cells" in str(ei.value) and "l = 8" in str(ei.value) and "len = 49" in str(ei.value), str(ei.value)
    still_usable()
    out = np.zeros((3, 17, 4), dtype=np.uint64)
    flags = np.full(3, 7, dtype=np.uint8)
    args = [rc._h, sent.ctypes.data, 3, present.ctypes.data, 17, NATURAL, out.ctypes.data, None, flags.ctypes.data]
    for hole in (0, 1, 3, 6, 8):
        a = list(args)
        a[hole] = None
        assert zkp.lib().zkp_kzg_recover_cosets_batch(*a) == zkp.ZKP_E_ARG, hole
    for layout in (2, -1):
        a = list(args)
        a[5] = layout
        assert zkp.lib().zkp_kzg_recover_cosets_batch(*a) == zkp.ZKP_E_ARG, layout
        assert "layout" in zkp.lib().zkp_last_error().decode()
    assert flags.tolist() == [7, 7, 7] and not out.any()
    still_usable()
    # the device entry: stride < len; nothing was launched (the words keep their 7)
    d_in, d_out = dev(sent), torch.zeros(3 * 20 * 4, dtype=torch.int64, device="cuda")
    d_flags = torch.full((3,), 7, dtype=torch.int32, device="cuda")
    with pytest.raises(zkp.ZkpError) as ei:
        rc.recover_batch_dev(d_in, 3, present, 17, 16, d_out, d_flags)
    assert ei.value.code == zkp.ZKP_E_ARG and "stride" in str(ei.value)
    with pytest.raises(zkp.ZkpError) as ei:
        rc.recover_batch_dev(d_in, 3, present, 17, 17, d_out, d_flags, cells=5)
    assert ei.value.code == zkp.ZKP_E_ARG
    rc.recover_batch_dev(d_in, 0, present, 17, 17, d_out, d_flags)  # an empty batch: OK, nothing touched
    torch.cuda.synchronize()
    assert d_flags.cpu().tolist() == [7, 7, 7] and not d_out.cpu().numpy().any()
    a = list(args)
    a[2] = 0
    assert zkp.lib().zkp_kzg_recover_cosets_batch(*a) == zkp.ZKP_OK and flags.tolist() == [7, 7, 7]
    rc.recover_batch_dev(d_in, 3, present, 17, 20, d_out, d_flags)
    torch.cuda.synchronize()
    assert d_flags.cpu().tolist() == [0, 0, 0] and np.array_equal(host(d_out, (3, 20, 4))[:, :17], f)
    still_usable()


def test_creation_beyond_the_byte_budget_is_refused_and_leaves_nothing(zkp, orc):
    import torch
    log_n, log_l, max_polys = 6, 3, 5
    recoverer(zkp, log_n, log_l, max_polys)  # (whatever the slot builds once for this shape and batch is built)
    single, pinned = km.workspace_bytes(log_n, log_l)
    total = single + 32 * (1 << log_n) * (max_polys - 1)  # only the n-element vector grows
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    os.environ[BUDGET] = str(total - 1)
    try:
        with pytest.raises(zkp.ZkpError) as ei:
            make_recoverer(zkp, log_n, log_l, max_polys)
        after = torch.cuda.mem_get_info()[0]
        os.environ[BUDGET] = str(total)
        rc = make_recoverer(zkp, log_n, log_l, max_polys)
    finally:
        del os.environ[BUDGET]
    msg = str(ei.value)
    assert ei.value.code == zkp.ZKP_E_NOMEM
    assert f"workspace of {total} bytes" in msg and f"{pinned} pinned" in msg and f"max_polys {max_polys}" in msg and f"MAX_BYTES {total - 1}" in msg, msg
    assert after == before, (before, after)
    f, ev = rows_of(orc, log_n, 17, max_polys)
    present = mask_of(8, {2})
    coeffs, _, ok = rc.recover_batch(given(ev, present), present, 17)
    assert ok.all() and np.array_equal(coeffs, f)
    rc.close()


def test_kzg_scheme_recover_cosets_batch(zkp, orc):
    log_n, log_l = 4, 2
    n, l, r = 16, 4, 4
    s = zkp.Srs.new_from_secret(orc.fr_from_ints([SECRET])[0], n)
    scheme = zkp.KzgScheme(s, expand_bases=False)
    present = mask_of(r, {0, 3})
    f, ev = rows_of(orc, log_n, 7, 2)
    coeffs, out_ev, ok = scheme.recover_cosets_batch(given(ev, present), present, 7, log_n, log_l)
    assert ok.all() and np.array_equal(coeffs, f) and np.array_equal(out_ev, ev)
    first = scheme._recoverers[4, 2]
    assert first.max_polys == 2
    f, ev = rows_of(orc, log_n, 7, 3)  # a batch that outgrows the kept recoverer replaces it
    coeffs, out_ev, ok, proofs = scheme.recover_cosets_batch(to_cells(given(ev, present), r), present, 7, log_n, log_l, proofs=True, cells=True)
    assert ok.all() and np.array_equal(coeffs, f) and np.array_equal(out_ev, to_cells(ev, r))
    assert scheme._recoverers[4, 2].max_polys == 3 and scheme._recoverers[4, 2] is not first
    exp = scheme.open_cosets_batch(f, log_n, log_l)[0]
    assert np.array_equal(proofs[0], exp[0]) and np.array_equal(proofs[1], exp[1])
    assert len(scheme.recover_cosets(given(ev, present)[0], present, 7, log_n, log_l)) == 3  # the single entry on the same recoverer
    assert list(scheme._recoverers) == [(4, 2)]
    scheme.close()
    assert scheme._recoverers == {} and scheme._coset_openers == {}


def test_batch_on_the_second_slot_in_a_child_process():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kzg_recover_batch_worker.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "OK kzg recover batch slots" in p.stdout
