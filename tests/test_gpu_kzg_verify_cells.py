"""GPU: batched cell verification (zkp_kzg_cell_verifier_*, zkp_kzg_verify_cells*, zkp_kzg_cells_aggregate_dev).  The SRS is [s^i]G
with a known s; cells and proofs come from KzgOpener.open_cosets, commitments from kzg_commit, [s^l]_2 from g2_mul -- the entries
that were there before.  Three polynomials per shape: one of full length, one of length <= l (every proof of it is the identity) and
the zero polynomial (its commitment is the identity).  The field half is compared bit for bit with tests/model/kzg_cells_model.py on
every limb of its three outputs; the two MSM results are not exposed, so the group half is judged by its verdicts: honest batches,
tampered ones, and zkp_kzg_verify_coset cell by cell as the yardstick.  ZKP_KZG_CELLS_CHUNK_LOG is set around the creation of a
verifier so that one chunk per cell, two cells per chunk and the default all run.  No test provokes a fault: bad input here is an
error code or a rejected batch."""
import os
import random

import numpy as np
import pytest

import bigmodel as bm
import g1_coset_model as cm
import kzg_cells_model as km

pytestmark = pytest.mark.gpu
R, P = km.R, bm.P
SECRET = 0x1F2E3D4C5B6A7988
KNOB = "ZKP_KZG_CELLS_CHUNK_LOG"
# r = 8 with l = 2; l below a workgroup's width; l = 1; l = 64, the practical cell
SHAPES = [(4, 1), (6, 3), (6, 0), (10, 6)]
CHUNK_LOGS = [0, 1, None]
COMMITS = 3
DEFAULT_CHUNK_LOG = 4  # KZG_CELLS_CHUNK_LOG of csrc/kzg_cells_plan.hpp


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


_srs, _data, _verifiers = {}, {}, {}


def srs(zkp, orc, count):
    if count not in _srs:
        xy = zkp.srs_g1(orc.fr_from_ints([SECRET])[0], count)
        _srs[count] = (xy, zkp.G1Bases.from_host(xy))
    return _srs[count]


class Data:
    """everything of one shape, computed once: the three polynomials, their commitments, cells and proofs"""

    def __init__(self, zkp, orc, log_n, log_l):
        self.log_n, self.log_l, self.n, self.l = log_n, log_l, 1 << log_n, 1 << log_l
        self.r = self.n // self.l
        self.bases = srs(zkp, orc, self.n)[1]
        lengths = [self.n, self.l, 1]
        polys = [orc.rand_fr(0x7300 + 16 * log_n + log_l, self.n), orc.rand_fr(0x7301 + 16 * log_n + log_l, self.l), np.zeros((1, 4), dtype=np.uint64)]
        opener = zkp.KzgOpener(self.bases, log_n, log_l)
        self.proofs, self.evals, self.evals_int = [], [], []
        self.commits = np.zeros((COMMITS, 12), dtype=np.uint64)
        self.commits_inf = np.zeros(COMMITS, dtype=np.uint8)
        for m, f in enumerate(polys):
            assert f.shape[0] == lengths[m]
            (xy, inf), ev = opener.open_cosets(f, evals=True)
            self.proofs.append((xy, inf))
            self.evals.append(ev)
            self.evals_int.append(orc.fr_to_ints(ev))
            c, cinf = zkp.kzg_commit(self.bases, f)
            self.commits[m], self.commits_inf[m] = c, cinf
        opener.close()
        assert self.proofs[1][1].all() and self.proofs[2][1].all() and self.commits_inf[2] == 1 and not self.commits_inf[:2].any()
        g2 = zkp.g2_generator()
        self.g2_sl = zkp.g2_mul(g2, orc.fr_from_ints([pow(SECRET, self.l, R)])[0])[0]
        self.g2_s = zkp.g2_mul(g2, orc.fr_from_ints([SECRET])[0])[0]

    def batch(self, cells):
        """cells: [(m, k)] -> commit_index, coset_index, evals (N, l, 4), (proofs xy, flags), evaluations as integers"""
        ci = np.array([m for m, _ in cells], dtype=np.uint32)
        ki = np.array([k for _, k in cells], dtype=np.uint32)
        ev = np.stack([self.evals[m][k::self.r] for m, k in cells]) if cells else np.zeros((0, self.l, 4), dtype=np.uint64)
        pxy = np.stack([self.proofs[m][0][k] for m, k in cells]) if cells else np.zeros((0, 12), dtype=np.uint64)
        pinf = np.array([self.proofs[m][1][k] for m, k in cells], dtype=np.uint8)
        return ci, ki, ev, (pxy, pinf), [self.evals_int[m][k::self.r] for m, k in cells]

    def batches(self):
        """name -> cells: one cell; all M r cells shuffled; a subset with duplicates and unused cosets; all cells of one coset"""
        rng = random.Random(0x7310 + self.log_n)
        every = [(m, k) for m in range(COMMITS) for k in range(self.r)]
        shuffled = every[:]
        rng.shuffle(shuffled)
        subset = [(m, k) for m, k in shuffled if k % 3 != 1][:9]
        subset += subset[:3]
        return {"one": [(0, self.r - 1)], "all": shuffled, "subset": subset, "coset": [(m, self.r // 2) for m in range(COMMITS)] * 2}


def data(zkp, orc, shape):
    if shape not in _data:
        _data[shape] = Data(zkp, orc, *shape)
    return _data[shape]


def make_verifier(zkp, bases, g2, log_n, log_l, max_cells, max_commits, chunk_log=None):
    old = os.environ.pop(KNOB, None)
    if chunk_log is not None:
        os.environ[KNOB] = str(chunk_log)
    try:
        return zkp.KzgCellVerifier(bases, g2, log_n, log_l, max_cells, max_commits)
    finally:
        os.environ.pop(KNOB, None)
        if old is not None:
            os.environ[KNOB] = old


def verifier(zkp, orc, shape, chunk_log=None):
    key = (shape, chunk_log)
    if key not in _verifiers:
        d = data(zkp, orc, shape)
        _verifiers[key] = make_verifier(zkp, d.bases, d.g2_sl, d.log_n, d.log_l, 2 * COMMITS * d.r, COMMITS, chunk_log)
    return _verifiers[key]


def weights_for(orc, seed, count):
    ints = [random.Random(seed + i).randrange(1 << 128) for i in range(count)]
    return orc.fr_from_ints(ints) if count else np.zeros((0, 4), dtype=np.uint64), ints


def run_aggregate(zkp, ver, d, ci, ki, ev, wt):
    import torch
    cells = len(ci)
    out_i = torch.full((d.l * 4,), -1, dtype=torch.int64, device="cuda")
    out_c = torch.full((COMMITS * 4,), -1, dtype=torch.int64, device="cuda")
    out_p = torch.full((max(cells, 1) * 4,), -1, dtype=torch.int64, device="cuda")
    ver.aggregate_dev(COMMITS, ci, ki, dev(ev) if cells else out_p, dev(wt) if cells else out_p, out_i, out_c, out_p)
    torch.cuda.synchronize()
    host = lambda t, rows: t.cpu().numpy().view(np.uint64).reshape(-1, 4)[:rows]
    return host(out_i, d.l), host(out_c, COMMITS), host(out_p, cells)


# ------------------------------------------------------------------------------------------------ the field half, bit for bit
@pytest.mark.parametrize("chunk_log", CHUNK_LOGS)
@pytest.mark.parametrize("shape", SHAPES)
def test_aggregate_is_the_model_bit_for_bit(zkp, orc, shape, chunk_log):
    d = data(zkp, orc, shape)
    ver = verifier(zkp, orc, shape, chunk_log)
    for at, (name, cells) in enumerate(d.batches().items()):
        ci, ki, ev, _, ev_int = d.batch(cells)
        wt, wt_int = weights_for(orc, 0x7320 + at, len(cells))
        if len(cells) > 2:
            wt[2], wt_int[2] = 0, 0  # a weight of 0 drops its cell
        exp = km.aggregate(d.log_n, d.log_l, COMMITS, ci.tolist(), ki.tolist(), ev_int, wt_int, DEFAULT_CHUNK_LOG if chunk_log is None else chunk_log)
        got = run_aggregate(zkp, ver, d, ci, ki, ev, wt)
        for what, g, e in zip(("interpolant", "commitment weights", "proof scalars"), got, exp):
            assert np.array_equal(g, orc.fr_from_ints(e)), (name, what)


@pytest.mark.parametrize("shape", SHAPES)
def test_a_second_smaller_batch_sees_nothing_of_the_first(zkp, orc, shape):
    d = data(zkp, orc, shape)
    ver = verifier(zkp, orc, shape, 1)
    b = d.batches()
    for at, name in enumerate(("all", "one", "subset", "one")):
        ci, ki, ev, _, ev_int = d.batch(b[name])
        wt, wt_int = weights_for(orc, 0x7330 + at, len(ci))
        exp = km.aggregate(d.log_n, d.log_l, COMMITS, ci.tolist(), ki.tolist(), ev_int, wt_int)
        got = run_aggregate(zkp, ver, d, ci, ki, ev, wt)
        assert all(np.array_equal(g, orc.fr_from_ints(e)) for g, e in zip(got, exp)), name
    got = run_aggregate(zkp, ver, d, *d.batch([])[:3], np.zeros((0, 4), dtype=np.uint64))  # no cell at all: zeros
    assert not got[0].any() and not got[1].any()


# ------------------------------------------------------------------------------------------------ verdicts
def verify(ver, d, ci, ki, ev, proofs, wt):
    return ver.verify((d.commits, d.commits_inf), ci, ki, ev, proofs, wt)


@pytest.mark.parametrize("shape", SHAPES)
def test_honest_batches_accept_on_both_entries(zkp, orc, shape):
    d = data(zkp, orc, shape)
    for at, (name, cells) in enumerate(d.batches().items()):
        ver = verifier(zkp, orc, shape, CHUNK_LOGS[at % 3])
        ci, ki, ev, proofs, _ = d.batch(cells)
        wt, _ = weights_for(orc, 0x7340 + at, len(cells))
        assert verify(ver, d, ci, ki, ev, proofs, wt), name
        assert ver.verify_dev(dev(d.commits), COMMITS, ci, ki, dev(ev), dev(proofs[0]), dev(wt), dev(d.commits_inf), dev(proofs[1])), name
    assert verify(verifier(zkp, orc, shape), d, *d.batch([])[:4], np.zeros((0, 4), dtype=np.uint64)), "an empty batch accepts"


@pytest.mark.parametrize("shape", SHAPES)
def test_tampered_batches_reject(zkp, orc, shape):
    d = data(zkp, orc, shape)
    l, r = d.l, d.r
    # polynomial 0 on every coset of the first half, then five cells of coset r / 2: with two cells per chunk that coset has three chunks
    cells = [(0, k) for k in range(r // 2)] + [(m, r // 2) for m in (0, 1, 2, 0, 0)]
    ci, ki, ev, (pxy, pinf), _ = d.batch(cells)
    wt, _ = weights_for(orc, 0x7350, len(cells))
    ver = verifier(zkp, orc, shape, 1)
    assert verify(ver, d, ci, ki, ev, (pxy, pinf), wt)
    one = orc.fr_from_ints([1])[0]
    first_of_coset, last_of_coset = r // 2, len(cells) - 1  # the first cell of coset r / 2 (its first chunk) and the last (its last chunk)
    for cell, pos in ((0, 0), (first_of_coset, 0), (last_of_coset, l - 1), (len(cells) - 2, l - 1)):
        bad = ev.copy()
        bad[cell, pos] = orc.fr_add(bad[cell, pos][None], one[None])[0]
        assert not verify(ver, d, ci, ki, bad, (pxy, pinf), wt), ("one altered evaluation", cell, pos)
    assert not ver.verify_dev(dev(d.commits), COMMITS, ci, ki, dev(bad), dev(pxy), dev(wt), dev(d.commits_inf), dev(pinf)), "the device entry too"
    bad = pxy.copy()
    bad[0] = d.proofs[0][0][1]
    assert not verify(ver, d, ci, ki, ev, (bad, pinf), wt), "a neighbouring coset's proof"
    bad = ci.copy()
    bad[0] = 1
    assert not verify(ver, d, bad, ki, ev, (pxy, pinf), wt), "a wrong commitment index"
    bad = ev.copy()
    bad[[0, 1]] = bad[[1, 0]]
    assert not verify(ver, d, ci, ki, bad, (pxy, pinf), wt), "the evaluations of two cells swapped"
    if d.log_l:
        wrong = make_verifier(zkp, d.bases, d.g2_s, d.log_n, d.log_l, len(cells), COMMITS)
        assert not verify(wrong, d, ci, ki, ev, (pxy, pinf), wt), "[s]_2 in place of [s^l]_2"
        wrong.close()
    assert verify(ver, d, ci, ki, ev, (pxy, pinf), wt), "and the verifier is as it was"


@pytest.mark.parametrize("shape", SHAPES)
def test_one_cell_batches_agree_with_verify_coset(zkp, orc, shape):
    """6 cells per shape, each as it is and with one altered evaluation: the batched verdict is zkp_kzg_verify_coset's"""
    d = data(zkp, orc, shape)
    ver = verifier(zkp, orc, shape)
    w = cm.root(d.log_n)
    one = orc.fr_from_ints([1])[0]
    for at, (m, k) in enumerate([(0, 0), (0, d.r - 1), (1, 1), (1, d.r // 2), (2, 0), (2, d.r - 2)]):
        ci, ki, ev, (pxy, pinf), _ = d.batch([(m, k)])
        wt, _ = weights_for(orc, 0x7360 + at, 1)
        x = orc.fr_from_ints([pow(w, k, R)])[0]
        for tamper in (False, True):
            if tamper:
                ev = ev.copy()
                ev[0, at % d.l] = orc.fr_add(ev[0, at % d.l][None], one[None])[0]
            single = zkp.kzg_verify_coset(d.bases, d.g2_sl, (d.commits[m], int(d.commits_inf[m])), (pxy[0], int(pinf[0])), x, ev[0])
            assert single == (not tamper)
            assert verify(ver, d, ci, ki, ev, (pxy, pinf), wt) == single, (m, k, tamper)


@pytest.mark.parametrize("shape", [(4, 1), (6, 3)])
def test_weights_enter_per_cell(zkp, orc, shape):
    """A cell twice, its copies with the errors +delta and -delta on one evaluation: equal weights let them cancel, distinct weights
    do not -- which is why the weights must be random.  A tampered cell of weight 0 is not checked at all."""
    d = data(zkp, orc, shape)
    ver = verifier(zkp, orc, shape, 0)
    cells = [(0, 1), (1, 2), (0, 1)]
    ci, ki, ev, proofs, _ = d.batch(cells)
    delta = orc.fr_from_ints([12345])
    ev[0, d.l - 1] = orc.fr_add(ev[0, d.l - 1][None], delta)[0]
    ev[2, d.l - 1] = orc.fr_sub(ev[2, d.l - 1][None], delta)[0]
    assert verify(ver, d, ci, ki, ev, proofs, orc.fr_from_ints([7, 9, 7])), "equal weights: the errors cancel"
    assert not verify(ver, d, ci, ki, ev, proofs, orc.fr_from_ints([7, 9, 8])), "distinct weights"
    ci, ki, ev, proofs, _ = d.batch([(0, 1), (1, 2)])
    ev[0, 0] = orc.fr_add(ev[0, 0][None], delta)[0]
    assert not verify(ver, d, ci, ki, ev, proofs, orc.fr_from_ints([5, 6]))
    assert verify(ver, d, ci, ki, ev, proofs, orc.fr_from_ints([0, 6])), "a weight of 0 drops its cell"


# ------------------------------------------------------------------------------------------------ refusals
def raw_ints(row):
    return (sum(int(v) << (64 * k) for k, v in enumerate(row[:6])), sum(int(v) << (64 * k) for k, v in enumerate(row[6:])))


def raw_row(x, y):
    return [(x >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)] + [(y >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(6)]


def test_bad_points_are_named(zkp, orc):
    shape = (6, 3)
    d = data(zkp, orc, shape)
    ver = verifier(zkp, orc, shape)
    cells = [(0, k) for k in range(d.r)] + [(1, 0)]
    ci, ki, ev, (pxy, pinf), _ = d.batch(cells)
    wt, _ = weights_for(orc, 0x7370, len(cells))
    mont = lambda v: v * (1 << 384) % P
    x, y = raw_ints(pxy[5])
    outside = raw_row(mont(4), mont(pow(4 ** 3 + 4, (P + 1) // 4, P)))  # on the curve, outside G1
    cases = [("proofs", 5, raw_row(x, y + 1), "curve"), ("proofs", 3, raw_row(x + P, y), "canonical"), ("commits", 1, outside, "subgroup")]
    for array, at, row, word in cases:
        commits, proofs = d.commits.copy(), pxy.copy()
        (proofs if array == "proofs" else commits)[at] = row
        if array == "proofs":
            proofs[at + 1] = row  # a second bad point behind it: the lowest index is named
        for entry in ("host", "dev"):
            with pytest.raises(zkp.ZkpError) as ei:
                if entry == "host":
                    ver.verify((commits, d.commits_inf), ci, ki, ev, (proofs, pinf), wt)
                else:
                    ver.verify_dev(dev(commits), COMMITS, ci, ki, dev(ev), dev(proofs), dev(wt), dev(d.commits_inf), dev(pinf))
            msg = str(ei.value)
            assert ei.value.code == zkp.ZKP_E_ARG and f"{array}[{at}]" in msg and word in msg, msg
    assert verify(ver, d, ci, ki, ev, (pxy, pinf), wt), "the verifier stays usable"
    # a bad point behind an infinity flag is no point at all
    commits = d.commits.copy()
    commits[2] = 0xFFFFFFFFFFFFFFFF
    assert ver.verify((commits, d.commits_inf), ci, ki, ev, (pxy, pinf), wt)


def test_call_refusals_come_before_any_launch(zkp, orc):
    shape = (6, 3)
    d = data(zkp, orc, shape)
    small = make_verifier(zkp, d.bases, d.g2_sl, 6, 3, 4, 2)
    ci, ki, ev, (pxy, pinf), _ = d.batch([(0, 1), (1, 2), (0, 3), (1, 4), (0, 5)])
    wt, _ = weights_for(orc, 0x7380, 5)
    two = (d.commits[:2], d.commits_inf[:2])

    def code(fn):
        with pytest.raises(zkp.ZkpError) as ei:
            fn()
        return ei.value.code, str(ei.value)

    assert code(lambda: small.verify(two, ci, ki, ev, (pxy, pinf), wt))[0] == zkp.ZKP_E_SIZE                      # 5 cells of 4
    four = slice(0, 4)
    assert small.verify(two, ci[four], ki[four], ev[four], (pxy[four], pinf[four]), wt[four])
    assert code(lambda: small.verify((d.commits, d.commits_inf), ci[four], ki[four], ev[four], (pxy[four], pinf[four]), wt[four]))[0] == zkp.ZKP_E_SIZE
    bad_k = ki[four].copy()
    bad_k[2] = d.r
    c, msg = code(lambda: small.verify(two, ci[four], bad_k, ev[four], (pxy[four], pinf[four]), wt[four]))
    assert c == zkp.ZKP_E_ARG and "cell 2" in msg and "coset" in msg, msg
    bad_c = ci[four].copy()
    bad_c[3] = 2
    c, msg = code(lambda: small.verify(two, bad_c, ki[four], ev[four], (pxy[four], pinf[four]), wt[four]))
    assert c == zkp.ZKP_E_ARG and "cell 3" in msg and "commitment" in msg, msg
    import torch
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    c, msg = code(lambda: small.aggregate_dev(2, ci[four], bad_k, dev(ev[four]), dev(wt[four]), out, out, out))
    assert c == zkp.ZKP_E_ARG and "cell 2" in msg
    c, msg = code(lambda: small.verify_dev(dev(d.commits), 2, bad_c, ki[four], dev(ev[four]), dev(pxy[four]), dev(wt[four])))
    assert c == zkp.ZKP_E_ARG and "cell 3" in msg
    acc = zkp.C.c_int(7)                                                                                              # null arguments
    args = [small._h, d.commits.ctypes.data, None, 2, 4, ci.ctypes.data, ki.ctypes.data, ev.ctypes.data, pxy.ctypes.data, None, wt.ctypes.data]
    for hole in (1, 5, 6, 7, 8, 10):
        a = list(args)
        a[hole] = None
        assert zkp.lib().zkp_kzg_verify_cells(*a, zkp.C.byref(acc)) == zkp.ZKP_E_ARG, hole
    assert zkp.lib().zkp_kzg_verify_cells(*args, None) == zkp.ZKP_E_ARG and acc.value == 7
    assert small.verify(two, ci[four], ki[four], ev[four], (pxy[four], pinf[four]), wt[four]), "still usable"
    small.close()


def test_creation_refusals(zkp, orc):
    import torch
    xy, bases = srs(zkp, orc, 64)
    g2 = zkp.g2_generator()
    create = zkp.lib().zkp_kzg_cell_verifier_create
    handle = zkp.C.c_void_p()
    for log_n, log_l in ((3, 3), (3, 4), (24, 6), (0, 0), (24, 0)):                         # 1 <= log_n - log_l, log_n <= 23
        assert create(bases._h, g2.ctypes.data, log_n, log_l, 8, 2, zkp.C.byref(handle)) == zkp.ZKP_E_ARG and not handle.value
    for max_cells, max_commits in ((0, 1), (1, 0), ((1 << 30) + 1, 1)):
        assert create(bases._h, g2.ctypes.data, 6, 3, max_cells, max_commits, zkp.C.byref(handle)) == zkp.ZKP_E_ARG and not handle.value
    off = g2.copy()
    off[0] ^= 1
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.KzgCellVerifier(bases, off, 6, 3, 8, 2)
    assert ei.value.code == zkp.ZKP_E_ARG and "[s^l]_2" in str(ei.value)
    short = zkp.G1Bases.from_host(xy[:7])
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.KzgCellVerifier(short, g2, 6, 3, 8, 2)
    assert ei.value.code == zkp.ZKP_E_SIZE
    zkp.KzgCellVerifier(zkp.G1Bases.from_host(xy[:8]), g2, 6, 3, 8, 2).close()               # l points are enough
    # a workspace that does not fit: the sizes are in the message and the device has as much free memory afterwards as before
    torch.cuda.synchronize()
    before = torch.cuda.mem_get_info()[0]
    big = srs(zkp, orc, 1024)[1]
    with pytest.raises(zkp.ZkpError) as ei:                                                # 2^30 chunk rows of 64 values: 2 TiB
        make_verifier(zkp, big, g2, 10, 6, 1 << 30, 4, 0)
    after = torch.cuda.mem_get_info()[0]
    chunks, cchunks = km.max_chunks(1 << 30, 16, 0), km.max_chunks(1 << 30, 4, 0)
    words = km.table_words(1 << 30, 4, 16, chunks, cchunks)
    total = 32 * 1024 + 32 * 64 * chunks + 32 * cchunks + 32 * 64 + 2 * 32 * (4 + (1 << 30)) + 64 + 4 * words
    total = (total + 31) // 32 * 32
    assert ei.value.code == zkp.ZKP_E_NOMEM and f"workspace of {total} bytes" in str(ei.value) and f"{4 * words} pinned" in str(ei.value), str(ei.value)
    assert after == before, (before, after)


# ------------------------------------------------------------------------------------------------ the wrapper
def test_kzg_scheme_verify_cells_draws_its_weights(zkp, orc):
    s = zkp.Srs.new_from_secret(orc.fr_from_ints([SECRET])[0], 16)
    scheme = zkp.KzgScheme(s, expand_bases=False)
    f = orc.rand_fr(0x7390, 16)
    (pxy, pinf), ev = scheme.open_cosets(f, 4, 2, evals=True)
    commitment = scheme.commit(f)
    g2_sl = zkp.g2_mul(zkp.g2_generator(), orc.fr_from_ints([pow(SECRET, 4, R)])[0])[0]
    cells = [3, 0, 2, 2]
    ci, ki = np.zeros(4, dtype=np.uint32), np.array(cells, dtype=np.uint32)
    evals = np.stack([ev[k::4] for k in cells])
    proofs = (pxy[cells], pinf[cells])
    commits = (commitment[0][None], np.array([commitment[1]], dtype=np.uint8))
    assert scheme.verify_cells(g2_sl, commits, ci, ki, evals, proofs, 4, 2)
    assert scheme.verify_cells(g2_sl, commitment[0][None], ci, ki, evals, proofs[0], 4, 2), "no flags: no identity among them"
    bad = evals.copy()
    bad[1, 3] = orc.fr_add(bad[1, 3][None], orc.fr_from_ints([1]))[0]
    assert not scheme.verify_cells(g2_sl, commits, ci, ki, bad, proofs, 4, 2)
    assert scheme.verify_cells(g2_sl, commits, ci, ki, evals, proofs, 4, 2, weights=orc.fr_from_ints([1, 2, 3, 4]))
    assert list(scheme._cell_verifiers) == [(4, 2)]
    scheme.close()
    assert scheme._cell_verifiers == {}
