"""GPU: cell recovery (zkp_kzg_recoverer_create, zkp_kzg_recover_cosets*).  f comes from orc.rand_fr, its evaluations from orc.ntt_fr;
the recovered coefficients must equal f bit for bit, and the returned evaluations those of the oracle.  Missing positions hold
all-ones bytes.  ZKP_KZG_RECOVER_LEAF_LOG is set around the creation of a recoverer so that the leaf kernel alone, and at least
three transform levels of the product tree at every shape with r >= 16, run whatever default the plan header commits."""
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
DEFAULT_LEAF_LOG = 5  # KZG_RECOVER_LEAF_LOG of csrc/kzg_recover_plan.hpp: the sets below put m around 2^this as well
SECRET = 0x1F2E3D4C5B6A7988

# r = 2; small; l = 1; cosets of 8; the practical cell; r = 1024 with a two-pass transform of n; r = 2^14: the deepest tree
SHAPES = [(2, 1), (3, 1), (6, 0), (6, 3), (10, 6), (12, 2), (14, 0)]
LEAVES = [1, 2, None]


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


def make_recoverer(zkp, log_n, log_l, leaf_log=None):
    old = os.environ.pop(KNOB, None)
    if leaf_log is not None:
        os.environ[KNOB] = str(leaf_log)
    try:
        return zkp.KzgRecoverer(log_n, log_l)
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


_recoverers, _polys = {}, {}


def recoverer(zkp, log_n, log_l, leaf_log=None):
    key = (log_n, log_l, leaf_log)
    if key not in _recoverers:
        _recoverers[key] = make_recoverer(zkp, log_n, log_l, leaf_log)
    return _recoverers[key]


def poly(orc, log_n, length):
    """(f, its evaluations on the domain): computed once, never changed"""
    key = (log_n, length)
    if key not in _polys:
        n = 1 << log_n
        f = orc.rand_fr(0x7400 + 4096 * log_n + length, length)
        padded = np.zeros((n, 4), dtype=np.uint64)
        padded[:length] = f
        ev = orc.ntt_fr(padded)
        f.setflags(write=False)
        ev.setflags(write=False)
        _polys[key] = (f, ev)
    return _polys[key]


def mask_of(r, missing):
    present = np.ones(r, dtype=np.uint8)
    present[list(missing)] = 0
    return present


def given(ev, present, fill=0xFF):
    """the evaluations with `fill` bytes at the positions of the missing cosets"""
    r = present.shape[0]
    out = ev.copy()
    gone = np.tile(present == 0, ev.shape[0] // r)
    out[gone] = np.frombuffer(bytes([fill]) * 8, dtype=np.uint64)[0]
    return out


def lengths(n, l):
    return sorted({x for x in (1, l, l + 1, n // 2, n - l) if 1 <= x <= n})


def missing_sets(log_n, log_l, leaf_log, rng):
    """name -> set of missing cosets, every one leaving at least one coset"""
    r = 1 << (log_n - log_l)
    t = leaf_log if leaf_log is not None else DEFAULT_LEAF_LOG
    sets = {"none": set(), "first": {0}, "last": {r - 1}, "first half": set(range(r // 2)), "second half": set(range(r // 2, r)),
            "every other": set(range(0, r, 2)), "random": set(rng.sample(range(r), rng.randint(1, r - 1)))}
    for m in ((1 << t) - 1, 1 << t, (1 << t) + 1):
        if 1 <= m < r:
            sets["m = %d" % m] = set(rng.sample(range(r), m))
    lr = log_n - log_l
    if lr >= 3:
        m = (1 << (lr - 1)) + (1 << (lr - 3)) + 1  # 2^a + 2^b + 1
        sets["m = %d" % m] = set(rng.sample(range(r), m))
    return sets


@pytest.mark.parametrize("leaf_log", LEAVES)
@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_recovered_coefficients_and_evaluations(zkp, orc, log_n, log_l, leaf_log):
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    rng = random.Random(0x7500 + 64 * log_n + log_l)
    rc = recoverer(zkp, log_n, log_l, leaf_log)
    sets = missing_sets(log_n, log_l, leaf_log, rng)
    calls = 0
    for length in lengths(n, l) + [n]:
        f, ev = poly(orc, log_n, length)
        todo = dict(sets) if length < n else {"none": set()}  # (n coefficients: m = 0 only)
        most = r - (length + l - 1) // l  # the largest admissible m for the length
        if most >= 1:
            todo["most"] = set(rng.sample(range(r), most))
        for name, missing in todo.items():
            if (r - len(missing)) * l < length:
                continue
            present = mask_of(r, missing)
            coeffs, out_ev, ok = rc.recover(given(ev, present), present, length, want_evals=True)
            assert ok, (name, length)
            assert np.array_equal(coeffs, f), (name, length)
            assert np.array_equal(out_ev, ev), (name, length)
            calls += 1
            if length in (1, n // 2):  # what stands at a missing position does not matter: zeros give the same
                again, _, ok = rc.recover(given(ev, present, 0), present, length)
                assert ok and again.tobytes() == coeffs.tobytes(), (name, length)
    assert calls >= 8


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_inconsistent_input_with_surplus_cells(zkp, orc, log_n, log_l):
    import torch
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    rng = random.Random(0x7600 + 64 * log_n + log_l)
    rc = recoverer(zkp, log_n, log_l)
    missing = set(rng.sample(range(r), r // 4))
    present = mask_of(r, missing)
    length = (r - len(missing)) * l - l  # one cell more than needed
    assert length >= 1
    f, ev = poly(orc, log_n, length)
    good = given(ev, present)
    at = rng.choice([i for i in range(n) if present[i % r]])
    bad = good.copy()
    bad[at] = ev[(at + 1) % n] if not np.array_equal(ev[(at + 1) % n], ev[at]) else ev[at] ^ np.uint64(1)
    _, _, ok = rc.recover(bad, present, length)
    assert not ok
    d_out, d_flag = torch.zeros(length * 4, dtype=torch.int64, device="cuda"), torch.full((1,), 7, dtype=torch.int32, device="cuda")
    rc.recover_dev(dev(bad), present, length, d_out, d_flag)
    torch.cuda.synchronize()
    assert int(d_flag.item()) == 1
    rc.recover_dev(dev(good), present, length, d_out, d_flag)
    torch.cuda.synchronize()
    assert int(d_flag.item()) == 0 and np.array_equal(host(d_out, (length, 4)), f)


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_exactly_enough_cells_are_always_consistent(zkp, orc, log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    rng = random.Random(0x7700 + 64 * log_n + log_l)
    rc = recoverer(zkp, log_n, log_l)
    missing = set(rng.sample(range(r), r // 2))
    present = mask_of(r, missing)
    length = (r - len(missing)) * l
    _, ev = poly(orc, log_n, length)
    bad = given(ev, present)
    at = rng.choice([i for i in range(n) if present[i % r]])
    bad[at] = ev[(at + 1) % n]
    coeffs, _, ok = rc.recover(bad, present, length)
    assert ok
    padded = np.zeros((n, 4), dtype=np.uint64)
    padded[:length] = coeffs
    back = orc.ntt_fr(padded)
    keep = np.tile(present == 1, l)
    assert np.array_equal(back[keep], bad[keep])  # the interpolant through what was given


def test_device_entry_three_calls_in_a_row(zkp, orc):
    import torch
    log_n, log_l = 10, 6
    n, r = 1 << log_n, 1 << (log_n - log_l)
    rc = recoverer(zkp, log_n, log_l, 2)
    rng = random.Random(0x7800)
    plans = [(set(rng.sample(range(r), 8)), n // 2), (set(), n), ({3}, 65), (set(rng.sample(range(r), 8)), n // 2)]
    queued = []
    for missing, length in plans:  # queued back to back, read afterwards: nothing of one call is left for the next
        present = mask_of(r, missing)
        f, ev = poly(orc, log_n, length)
        d_out = torch.zeros(length * 4, dtype=torch.int64, device="cuda")
        d_ev = torch.zeros(n * 4, dtype=torch.int64, device="cuda")
        d_flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
        rc.recover_dev(dev(given(ev, present)), present, length, d_out, d_flag, d_ev)
        present[:] = 0  # read before the call returned
        queued.append((f, ev, d_out, d_ev, d_flag, length))
    torch.cuda.synchronize()
    for f, ev, d_out, d_ev, d_flag, length in queued:
        assert int(d_flag.item()) == 0
        assert np.array_equal(host(d_out, (length, 4)), f) and np.array_equal(host(d_ev, (n, 4)), ev), length
    missing, length = plans[0]
    present = mask_of(r, missing)
    f, ev = poly(orc, log_n, length)
    d_out, d_flag = torch.zeros(length * 4, dtype=torch.int64, device="cuda"), torch.full((1,), 7, dtype=torch.int32, device="cuda")
    rc.recover_dev(dev(given(ev, present)), present, length, d_out, d_flag)  # evaluations not asked for
    torch.cuda.synchronize()
    ref, _, ok = rc.recover(given(ev, present), present, length)
    assert ok and int(d_flag.item()) == 0 and host(d_out, (length, 4)).tobytes() == ref.tobytes() == f.tobytes()


def test_kzg_scheme_recover_cosets_with_proofs(zkp, orc):
    log_n, log_l = 4, 2
    n, l, r = 16, 4, 4
    s = zkp.Srs.new_from_secret(orc.fr_from_ints([SECRET])[0], n)
    scheme = zkp.KzgScheme(s, expand_bases=False)
    f, ev = poly(orc, log_n, 7)
    present = mask_of(r, {1, 2})
    coeffs, out_ev, ok, proofs = scheme.recover_cosets(given(ev, present), present, 7, log_n, log_l, proofs=True)
    assert ok and np.array_equal(coeffs, f) and np.array_equal(out_ev, ev)
    exp = scheme.open_cosets(f, log_n, log_l)[0]
    assert np.array_equal(proofs[0], exp[0]) and np.array_equal(proofs[1], exp[1])
    assert len(scheme.recover_cosets(given(ev, present), present, 7, log_n, log_l)) == 3  # the same recoverer again
    assert list(scheme._recoverers) == [(4, 2)] and list(scheme._coset_openers) == [(4, 2)] and scheme._openers == {}
    # a recovered cell (coset 1 was missing) passes the verifier
    commitment = zkp.kzg_commit(s.bases, f)
    g2_sl, _ = zkp.g2_mul(zkp.g2_generator(), orc.fr_from_ints([pow(SECRET, l, km.R)])[0])
    k = 1
    x = orc.fr_from_ints([pow(km.root(log_n), k, km.R)])[0]
    assert zkp.kzg_verify_coset(s.bases, g2_sl, commitment, (proofs[0][k], int(proofs[1][k])), x, out_ev[k::r])
    assert not zkp.kzg_verify_coset(s.bases, g2_sl, commitment, (proofs[0][k], int(proofs[1][k])), x, out_ev[k + 1::r])
    scheme.close()
    assert scheme._recoverers == {} and scheme._coset_openers == {}


def test_error_codes(zkp, orc):
    log_n, log_l = 6, 3
    n, l, r = 64, 8, 8
    for a, b in ((3, 3), (3, 4), (24, 6), (0, 0), (24, 0)):  # log_l >= log_n, log_n > 23
        handle = zkp.C.c_void_p()
        assert zkp.lib().zkp_kzg_recoverer_create(a, b, zkp.C.byref(handle)) == zkp.ZKP_E_ARG, (a, b)
        assert not handle.value
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.KzgRecoverer(3, 3)
    assert ei.value.code == zkp.ZKP_E_ARG
    rc = recoverer(zkp, log_n, log_l)
    f, ev = poly(orc, log_n, 17)
    present = mask_of(r, {0, 5})

    def still_usable():
        coeffs, _, ok = rc.recover(given(ev, present), present, 17)
        assert ok and np.array_equal(coeffs, f)

    with pytest.raises(zkp.ZkpError) as ei:
        rc.recover(ev, present, 0)
    assert ei.value.code == zkp.ZKP_E_ARG
    still_usable()
    with pytest.raises(zkp.ZkpError) as ei:
        rc.recover(ev, present, n + 1)
    assert ei.value.code == zkp.ZKP_E_SIZE
    still_usable()
    with pytest.raises(zkp.ZkpError) as ei:  # 6 cells of 8 points do not give 49 coefficients
        rc.recover(ev, present, 6 * l + 1)
    assert ei.value.code == zkp.ZKP_E_SIZE
    assert "6 present cells" in str(ei.value) and "l = 8" in str(ei.value) and "len = 49" in str(ei.value), str(ei.value)
    still_usable()
    ok = zkp.C.c_int(7)
    out = np.zeros((17, 4), dtype=np.uint64)
    assert zkp.lib().zkp_kzg_recover_cosets(rc._h, None, present.ctypes.data, 17, out.ctypes.data, None, zkp.C.byref(ok)) == zkp.ZKP_E_ARG
    assert zkp.lib().zkp_kzg_recover_cosets(None, ev.ctypes.data, present.ctypes.data, 17, out.ctypes.data, None, zkp.C.byref(ok)) == zkp.ZKP_E_ARG
    assert ok.value == 7
    still_usable()


def test_creation_beyond_the_byte_budget_is_refused_and_leaves_nothing(zkp, orc):
    import torch
    log_n, log_l = 6, 3
    recoverer(zkp, log_n, log_l)  # (whatever the slot builds once for this shape is built)
    total, pinned = km.workspace_bytes(log_n, log_l)
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    os.environ["ZKP_KZG_RECOVER_MAX_BYTES"] = str(total - 1)
    try:
        with pytest.raises(zkp.ZkpError) as ei:
            make_recoverer(zkp, log_n, log_l)
        after = torch.cuda.mem_get_info()[0]
        os.environ["ZKP_KZG_RECOVER_MAX_BYTES"] = str(total)
        rc = make_recoverer(zkp, log_n, log_l)
    finally:
        del os.environ["ZKP_KZG_RECOVER_MAX_BYTES"]
    msg = str(ei.value)
    assert ei.value.code == zkp.ZKP_E_NOMEM
    assert f"workspace of {total} bytes" in msg and f"{pinned} pinned" in msg and f"MAX_BYTES {total - 1}" in msg, msg
    assert after == before, (before, after)
    f, ev = poly(orc, log_n, 17)
    present = mask_of(8, {2})
    coeffs, _, ok = rc.recover(given(ev, present), present, 17)
    assert ok and np.array_equal(coeffs, f)
    still = recoverer(zkp, log_n, log_l).recover(given(ev, present), present, 17)  # and the handle made before the refusal
    assert still[2] and np.array_equal(still[0], f)
    rc.close()


def test_recoverer_on_the_second_slot_in_a_child_process():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "kzg_recover_worker.py")], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-3000:])
    assert "OK kzg recover slots" in p.stdout
