"""GPU: batched verification of point openings (zkp_kzg_point_verifier_*, zkp_kzg_verify_points*, zkp_kzg_verify_points_find_bad*,
zkp_kzg_points_aggregate_dev, zkp_kzg_verify_evals_batch_dev).  The SRS is [s^i]G with a known s, so an honest opening of f at z is
made in scalars -- y = f(z), W = [(f(s) - y) / (s - z)]G by the fixed-base entry -- and checked against kzg_open / kzg_commit /
KzgEvalOpener.open_batch, the entries that were there before, where a test takes its openings from those.  The field half is compared
bit for bit with tests/model/kzg_points_model.py on every limb of its four outputs; the two MSM results are not exposed, so the group
half is judged by its verdicts: honest batches, tampered ones, and zkp_kzg_batch_verify as the yardstick.  ZKP_KZG_CELLS_CHUNK_LOG is
set around the creation of a verifier so that one opening per chunk and the default both run.  No test provokes a fault: bad input
here is an error code or a rejected batch.  No test runs more than about 40 pairing checks (about 31 ms each on the host)."""
import os
import random

import numpy as np
import pytest

import bigmodel as bm
import kzg_points_model as pm

pytestmark = pytest.mark.gpu
R, P = pm.R, bm.P
SECRET = 0x1F2E3D4C5B6A7988
KNOB = "ZKP_KZG_CELLS_CHUNK_LOG"
SIZES = [1, 2, 15, 16, 17, 255, 256, 257, 1025]
MAX_OPENINGS, MAX_COMMITS = 1025, 1026
MASK = (1 << 64) - 1


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available(), "no GPU"
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def points_module():
    import zkp_hip.kzg_points
    return zkp_hip.kzg_points


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else np.uint8)).cuda()


_cache = {}


def g2s(zkp, orc):
    if "g2s" not in _cache:
        _cache["g2s"] = zkp.g2_mul(zkp.g2_generator(), orc.fr_from_ints([SECRET])[0])[0]
    return _cache["g2s"]


def verifier(zkp, orc, chunk_log=None):
    """one verifier of MAX_OPENINGS x MAX_COMMITS per chunk log, kept"""
    key = ("verifier", chunk_log)
    if key not in _cache:
        old = os.environ.pop(KNOB, None)
        if chunk_log is not None:
            os.environ[KNOB] = str(chunk_log)
        try:
            _cache[key] = points_module().KzgPointVerifier(g2s(zkp, orc), MAX_OPENINGS, MAX_COMMITS)
        finally:
            os.environ.pop(KNOB, None)
            if old is not None:
                os.environ[KNOB] = old
    return _cache[key]


def evaluate(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def fixed_base(zkp, orc, scalars):
    """[k]G for every k -> ((n, 12) limbs, (n,) flags)"""
    import torch
    n = len(scalars)
    xy = torch.zeros(n * 12, dtype=torch.int64, device="cuda")
    inf = torch.zeros(n, dtype=torch.uint8, device="cuda")
    zkp.g1_fixed_base_mul_dev(dev(orc.fr_from_ints(scalars)), n, xy, inf)
    torch.cuda.synchronize()
    return xy.cpu().numpy().view(np.uint64).reshape(n, 12), inf.cpu().numpy()


class Batch:
    """Honest openings of `polys` (lists of integer coefficients) made in scalars: opening i is of polys[index[i]] at zs[i]"""

    def __init__(self, zkp, orc, polys, index, zs):
        self.polys, self.index, self.zs_int = polys, list(index), list(zs)
        self.at_s = [evaluate(f, SECRET) for f in polys]
        self.ys_int = [evaluate(polys[m], z) for m, z in zip(index, zs)]
        self.quot = [(self.at_s[m] - y) * pow(SECRET - z, -1, R) % R for m, z, y in zip(index, zs, self.ys_int)]
        self.commits, self.commits_inf = fixed_base(zkp, orc, self.at_s)
        self.proofs, self.proofs_inf = fixed_base(zkp, orc, self.quot)
        self.ci = np.array(index, dtype=np.uint32)
        self.zs, self.ys = orc.fr_from_ints(self.zs_int), orc.fr_from_ints(self.ys_int)
        self.count = len(index)

    def weights_int(self, seed):
        return [random.Random(seed + i).randrange(1, 1 << 128) for i in range(self.count)]

    def weights(self, orc, seed):
        return orc.fr_from_ints(self.weights_int(seed))

    def host(self, **over):
        a = dict(commitments=(self.commits, self.commits_inf), zs=self.zs, ys=self.ys, proofs=(self.proofs, self.proofs_inf), commit_index=self.ci)
        a.update(over)
        return a

    def on_device(self, wt, **over):
        a = dict(commits=self.commits, zs=self.zs, ys=self.ys, proofs=self.proofs, commit_index=self.ci)
        a.update(over)
        return dict(commits_tensor=dev(a["commits"]), n_commits=a["commits"].shape[0], n_openings=self.count, z_tensor=dev(a["zs"]),
                    y_tensor=dev(a["ys"]), proofs_tensor=dev(a["proofs"]), weights_tensor=dev(wt), commit_index=a["commit_index"],
                    commits_inf_tensor=dev(self.commits_inf), proofs_inf_tensor=dev(self.proofs_inf))


def rand_poly(seed, length):
    rng = random.Random(seed)
    return [rng.randrange(R) for _ in range(length)]


def batch(zkp, orc, name):
    """the batches the verdict tests share, made once"""
    key = ("batch", name)
    if key not in _cache:
        rng = random.Random(0x7500 + sum(map(ord, name)))
        polys = [rand_poly(0x7501, 16), rand_poly(0x7502, 9), rand_poly(0x7503, 3)]
        if name == "257 over 3":
            index = [rng.choice((0, 0, 0, 1, 2)) for _ in range(257)]
        elif name == "9 over 3":
            index = [0, 1, 2, 0, 0, 1, 2, 2, 0]
        elif name == "37 over 3":
            index = [rng.randrange(3) for _ in range(37)]
        elif name == "5 one each":
            polys, index = [rand_poly(0x7510 + m, 4 + m) for m in range(5)], list(range(5))
        elif name == "constant":  # every proof is the identity
            polys, index = [[12345], rand_poly(0x7504, 1)], [0, 1, 0]
        elif name == "zero":  # the commitment is the identity, and so is every proof
            polys, index = [[0], rand_poly(0x7505, 5)], [0, 1, 0, 1]
        _cache[key] = Batch(zkp, orc, polys, index, [rng.randrange(R) for _ in index])
    return _cache[key]


# ------------------------------------------------------------------------------------------------ the field half, bit for bit
def groupings(n, rng):
    """name -> (n_commits, index or None): identity, one commitment, one opening per commitment plus an unused one, a skewed split"""
    each = list(range(n))
    rng.shuffle(each)
    return {"identity": (n, None), "one": (1, [0] * n), "each": (n + 1, each),
            "skew": (6, [2 if rng.randrange(8) else rng.choice((0, 5)) for _ in range(n)])}


def raw(values):
    """integers below 2^256 as limbs, unchanged"""
    return np.array([[(v >> (64 * k)) & MASK for k in range(4)] for v in values], dtype=np.uint64).reshape(-1, 4)


def field_case(orc, n, seed):
    """-> integers zs, ys, ws and their limbs; the edge values of the issue where n leaves room, y not canonical in memory, one opening twice"""
    rng = random.Random(seed)
    zs, ys, ws = ([rng.randrange(R) for _ in range(n)] for _ in range(3))
    ws = [w >> 127 for w in ws]  # 128-bit weights, mostly
    if n >= 15:
        zs[3], ys[4], ws[5], ws[6] = 0, 0, 0, R - 1
        zs[9], ys[9], ws[9] = zs[8], ys[8], ws[8]  # one opening repeated
    zl, yl, wl = orc.fr_from_ints(zs), orc.fr_from_ints(ys), orc.fr_from_ints(ws)
    for at in range(0, n, 7):  # the same residue, limbs + r: not canonical
        v = sum(int(x) << (64 * k) for k, x in enumerate(yl[at]))
        if v + R < 1 << 256:
            yl[at] = raw([v + R])[0]
    return zs, ys, ws, zl, yl, wl


def run_aggregate(zkp, ver, n_commits, index, zl, yl, wl):
    import torch
    n = zl.shape[0]
    outs = [torch.full((max(rows, 1) * 4,), -1, dtype=torch.int64, device="cuda") for rows in (n_commits, n, n, 1)]
    ver.aggregate_dev(n_commits, n, dev(zl) if n else outs[1], dev(yl) if n else outs[1], dev(wl) if n else outs[1], *outs,
                      commit_index=None if index is None else np.array(index, dtype=np.uint32))
    torch.cuda.synchronize()
    return [t.cpu().numpy().view(np.uint64).reshape(-1, 4)[:rows] for t, rows in zip(outs, (n_commits, n, n, 1))]


def check_aggregate(zkp, orc, ver, n, name, n_commits, index, chunk_log, seed):
    zs, ys, ws, zl, yl, wl = field_case(orc, n, seed)
    cw, rz, r, neg = pm.aggregate(n_commits, index, zs, ys, ws, chunk_log)
    got = run_aggregate(zkp, ver, n_commits, index, zl, yl, wl)
    for what, g, e in zip(("commitment weights", "r z", "r", "-sum r y"), got, (cw, rz, r, [neg])):
        assert np.array_equal(g, orc.fr_from_ints(e)), (n, name, what)


@pytest.mark.parametrize("chunk_log", [0, 4])
def test_aggregate_is_the_model_bit_for_bit(zkp, orc, chunk_log):
    ver = verifier(zkp, orc, chunk_log)
    for n in SIZES:
        for name, (n_commits, index) in groupings(n, random.Random(0x7520 + n)).items():
            check_aggregate(zkp, orc, ver, n, name, n_commits, index, chunk_log, 0x7530 + n)


def test_a_second_smaller_batch_sees_nothing_of_the_first(zkp, orc):
    ver = verifier(zkp, orc, 0)
    for at, n in enumerate((1025, 2, 257, 1)):
        for name, (n_commits, index) in groupings(n, random.Random(0x7540 + at)).items():
            check_aggregate(zkp, orc, ver, n, name, n_commits, index, 0, 0x7550 + at)
    none = np.zeros((0, 4), dtype=np.uint64)
    got = run_aggregate(zkp, ver, 3, [], none, none, none)  # no opening at all: zeros
    assert not got[0].any() and not got[3].any()


# ------------------------------------------------------------------------------------------------ verdicts
def both_entries(zkp, ver, b, wt):
    host = ver.verify(weights=wt, **b.host())
    assert ver.verify_dev(**b.on_device(wt)) == host
    return host


def test_honest_batches_accept_on_both_entries(zkp, orc):
    for at, name in enumerate(("257 over 3", "constant", "zero")):
        b = batch(zkp, orc, name)
        assert both_entries(zkp, verifier(zkp, orc, (0, 4, None)[at]), b, b.weights(orc, 0x7560 + at)), name
    b = batch(zkp, orc, "constant")
    assert b.proofs_inf.all() and not b.commits_inf.any()
    b = batch(zkp, orc, "zero")
    assert b.commits_inf[0] == 1 and b.proofs_inf[0] == 1
    assert verifier(zkp, orc).verify(np.zeros((0, 12), dtype=np.uint64), *[np.zeros((0, 4), dtype=np.uint64)] * 2, np.zeros((0, 12), dtype=np.uint64),
                                     np.zeros((0, 4), dtype=np.uint64)), "an empty batch accepts"


def test_one_opening_of_kzg_open_accepts(zkp, orc):
    """N = 1, the commitment and the opening from the entries that were there before; the scalar construction of this file gives the
    same points"""
    xy = zkp.srs_g1(orc.fr_from_ints([SECRET])[0], 16)
    bases = zkp.G1Bases.from_host(xy)
    f = rand_poly(0x7501, 16)
    z = 0x1234567
    (w, winf), y = zkp.kzg_open(bases, orc.fr_from_ints(f), orc.fr_from_ints([z])[0])
    c, cinf = zkp.kzg_commit(bases, orc.fr_from_ints(f))
    b = Batch(zkp, orc, [f], [0], [z])
    assert np.array_equal(b.proofs[0], w) and np.array_equal(b.commits[0], c) and np.array_equal(b.ys[0], y) and not winf and not cinf
    ver = verifier(zkp, orc)
    wt = b.weights(orc, 0x7570)
    assert ver.verify((c[None], np.array([cinf], dtype=np.uint8)), orc.fr_from_ints([z]), y[None], w[None], wt)  # the identity index
    assert both_entries(zkp, ver, b, wt)
    assert not ver.verify(c[None], orc.fr_from_ints([z + 1]), y[None], w[None], wt)


def test_tampered_batches_reject(zkp, orc):
    b = batch(zkp, orc, "9 over 3")
    ver = verifier(zkp, orc, 0)
    wt = b.weights(orc, 0x7580)
    assert both_entries(zkp, ver, b, wt)
    one = orc.fr_from_ints([1])
    ys = b.ys.copy()
    ys[4] = orc.fr_add(ys[4][None], one)[0]
    assert not ver.verify(weights=wt, **b.host(ys=ys)), "y_i + 1"
    assert not ver.verify_dev(**b.on_device(wt, ys=ys)), "the device entry too"
    zs = b.zs.copy()
    zs[8] = orc.fr_add(zs[8][None], one)[0]
    assert not ver.verify(weights=wt, **b.host(zs=zs)), "z_i changed"
    proofs = b.proofs.copy()
    proofs[[1, 6]] = proofs[[6, 1]]
    assert not ver.verify(weights=wt, **b.host(proofs=(proofs, b.proofs_inf))), "W_i swapped with W_j"
    commits = b.commits.copy()
    commits[1] = b.proofs[0]
    assert not ver.verify(weights=wt, **b.host(commitments=(commits, b.commits_inf))), "C_m replaced by another point of G1"
    ci = b.ci.copy()
    ci[0] = 1
    assert not ver.verify(weights=wt, **b.host(commit_index=ci)), "a wrong commit_index"
    zero = wt.copy()
    zero[4] = 0
    assert ver.verify(weights=zero, **b.host(ys=ys)), "a weight of 0 drops its opening"
    assert ver.verify(weights=wt, **b.host()), "and the verifier is as it was"


def test_identity_index_agrees_with_batch_verify(zkp, orc):
    """N = 5 <= 8, opening i of commitment i: the verdict is zkp_kzg_batch_verify's on the same arrays, honest and tampered"""
    b = batch(zkp, orc, "5 one each")
    ver = verifier(zkp, orc)
    wt = b.weights(orc, 0x7590)
    assert not b.commits_inf.any() and not b.proofs_inf.any()
    one = orc.fr_from_ints([1])
    cases = {"honest": {}}
    ys = b.ys.copy()
    ys[0] = orc.fr_add(ys[0][None], one)[0]
    cases["y"] = dict(ys=ys)
    zs = b.zs.copy()
    zs[4] = orc.fr_sub(zs[4][None], one)[0]
    cases["z"] = dict(zs=zs)
    proofs = b.proofs.copy()
    proofs[[2, 3]] = proofs[[3, 2]]
    cases["proofs"] = dict(proofs=proofs)
    commits = b.commits.copy()
    commits[1] = commits[0]
    cases["commits"] = dict(commits=commits)
    for name, over in cases.items():
        a = dict(commits=b.commits, zs=b.zs, ys=b.ys, proofs=b.proofs)
        a.update(over)
        old = zkp.kzg_batch_verify(g2s(zkp, orc), a["commits"], a["zs"], a["proofs"], a["ys"], wt)
        assert old == (name == "honest"), name
        assert ver.verify(a["commits"], a["zs"], a["ys"], a["proofs"], wt) == old, name
        assert ver.verify_dev(dev(a["commits"]), 5, 5, dev(a["zs"]), dev(a["ys"]), dev(a["proofs"]), dev(wt)) == old, name


# ------------------------------------------------------------------------------------------------ the blob form
@pytest.mark.parametrize("bitrev", [False, True])
def test_blob_form_checks_rows_without_values(zkp, orc, bitrev):
    """5 rows at n = 2^4, one of them opened inside the domain; commitments and proofs are KzgEvalOpener's"""
    log_n, n, rows = 4, 16, 5
    xy = zkp.srs_g1(orc.fr_from_ints([SECRET])[0], n)
    bases = zkp.G1Bases.from_host(xy)
    lagrange = bases.lagrange(log_n)
    from zkp_hip.kzg_evals import KzgEvalOpener
    opener = KzgEvalOpener(lagrange, log_n, rows, bitrev=bitrev)
    evals = orc.rand_fr(0x75A0 + bitrev, rows * n).reshape(rows, n, 4)
    w = orc.fr_to_ints(orc.fr_root_of_unity(log_n)[None])[0]
    zs_int = [random.Random(0x75A2 + p).randrange(R) for p in range(rows)]
    zs_int[3] = pow(w, 5, R)  # in the domain
    zs = orc.fr_from_ints(zs_int)
    commits, commits_inf = opener.commit_batch(evals)
    (proofs, proofs_inf), ys = opener.open_batch(evals, zs)
    ver = verifier(zkp, orc)
    wt = orc.fr_from_ints([random.Random(0x75A8 + p).randrange(1, 1 << 128) for p in range(rows)])
    run = lambda ev: ver.verify_evals_dev(opener, dev(ev), rows, dev(zs), dev(commits), dev(proofs), dev(wt), dev(commits_inf), dev(proofs_inf))
    assert run(evals)
    assert ver.verify((commits, commits_inf), zs, ys, (proofs, proofs_inf), wt), "the same openings with their values supplied"
    at_z = 0b1010 if bitrev else 5  # where row 3 keeps its value at w^5: the one value of that row its opening depends on
    for row, pos in ((3, at_z), (0, 15), (4, 0)):
        bad = evals.copy()
        bad[row, pos] = orc.fr_add(bad[row, pos][None], orc.fr_from_ints([1]))[0]
        assert not run(bad), ("one changed value", row, pos)
    assert run(evals)
    small = points_module().KzgPointVerifier(g2s(zkp, orc), 4, 4)
    with pytest.raises(zkp.ZkpError) as ei:
        small.verify_evals_dev(opener, dev(evals), rows, dev(zs), dev(commits), dev(proofs), dev(wt))
    assert ei.value.code == zkp.ZKP_E_SIZE
    small.close()
    opener.close()
    lagrange.close()


# ------------------------------------------------------------------------------------------------ the lowest failing opening
def test_find_bad_names_the_lowest_failing_opening(zkp, orc):
    b = batch(zkp, orc, "37 over 3")
    ver = verifier(zkp, orc)
    wt = b.weights(orc, 0x75B0)
    one = orc.fr_from_ints([1])
    zkp.profile_enable(True)
    try:
        for bad_set, want in ((set(), None), ({0}, 0), ({36}, 36), ({17, 30}, 17)):
            ys = b.ys.copy()
            for i in bad_set:
                ys[i] = orc.fr_add(ys[i][None], one)[0]
            zkp.profile_reset()
            assert ver.find_bad(weights=wt, **b.host(ys=ys)) == want, bad_set
            checks = zkp.profile_read("kzg_points_pairing")[1]
            assert checks <= 1 + 6, (bad_set, checks)  # ceil(log2 37) = 6
            ys_int = [(y + 1) % R if i in bad_set else y for i, y in enumerate(b.ys_int)]
            model = pm.find_bad(SECRET, b.at_s, b.quot, 3, b.index, b.zs_int, ys_int, b.weights_int(0x75B0))
            assert model == (pm.SIZE_MAX if want is None else want, checks), "the model's bisection, check for check"
        ys = b.ys.copy()
        ys[17] = orc.fr_add(ys[17][None], one)[0]
        assert ver.find_bad_dev(**b.on_device(wt, ys=ys)) == 17, "the device entry"
        assert ver.find_bad_dev(**b.on_device(wt)) is None
    finally:
        zkp.profile_enable(False)
    acc, bad = zkp.C.c_int(0), zkp.C.c_size_t(0)
    assert zkp.lib().zkp_kzg_verify_points_find_bad(ver._h, None, None, 0, 0, None, None, None, None, None, None, zkp.C.byref(acc),
                                                    zkp.C.byref(bad)) == zkp.ZKP_OK
    assert acc.value == 1 and bad.value == points_module().NO_BAD_OPENING, "an empty batch is accepted: SIZE_MAX"


# ------------------------------------------------------------------------------------------------ refusals
def raw_ints(row):
    return (sum(int(v) << (64 * k) for k, v in enumerate(row[:6])), sum(int(v) << (64 * k) for k, v in enumerate(row[6:])))


def raw_row(x, y):
    return [(x >> (64 * k)) & MASK for k in range(6)] + [(y >> (64 * k)) & MASK for k in range(6)]


def test_bad_points_are_named(zkp, orc):
    b = batch(zkp, orc, "9 over 3")
    ver = verifier(zkp, orc)
    wt = b.weights(orc, 0x75C0)
    mont = lambda v: v * (1 << 384) % P
    x, y = raw_ints(b.proofs[5])
    outside = raw_row(mont(4), mont(pow(4 ** 3 + 4, (P + 1) // 4, P)))  # on the curve, outside G1
    cases = [("proofs", 5, raw_row(x, y + 1), "curve"), ("proofs", 3, raw_row(x + P, y), "canonical"), ("commits", 1, outside, "subgroup")]
    for array, at, row, word in cases:
        commits, proofs = b.commits.copy(), b.proofs.copy()
        (proofs if array == "proofs" else commits)[at] = row
        if array == "proofs":
            proofs[at + 1] = row  # a second bad point behind it: the lowest index is named
        for entry in ("host", "dev", "find_bad"):
            with pytest.raises(zkp.ZkpError) as ei:
                if entry == "host":
                    ver.verify(weights=wt, **b.host(commitments=(commits, b.commits_inf), proofs=(proofs, b.proofs_inf)))
                elif entry == "dev":
                    ver.verify_dev(**b.on_device(wt, commits=commits, proofs=proofs))
                else:
                    ver.find_bad(weights=wt, **b.host(commitments=(commits, b.commits_inf), proofs=(proofs, b.proofs_inf)))
            msg = str(ei.value)
            assert ei.value.code == zkp.ZKP_E_ARG and f"{array}[{at}]" in msg and word in msg, msg
    assert ver.verify(weights=wt, **b.host()), "the verifier stays usable"
    # a bad point behind an infinity flag is no point at all
    z = batch(zkp, orc, "zero")
    commits = z.commits.copy()
    commits[0] = MASK
    assert ver.verify(weights=z.weights(orc, 0x75C8), **z.host(commitments=(commits, z.commits_inf)))


def test_call_refusals_come_before_any_launch(zkp, orc):
    b = batch(zkp, orc, "9 over 3")
    small = points_module().KzgPointVerifier(g2s(zkp, orc), 8, 2)
    wt = b.weights(orc, 0x75D0)

    def code(fn):
        with pytest.raises(zkp.ZkpError) as ei:
            fn()
        return ei.value.code, str(ei.value)

    assert code(lambda: small.verify(weights=wt, **b.host()))[0] == zkp.ZKP_E_SIZE  # 9 openings of 8
    eight = slice(0, 8)
    cut = dict(zs=b.zs[eight], ys=b.ys[eight], proofs=(b.proofs[eight], b.proofs_inf[eight]), commit_index=b.ci[eight])
    assert code(lambda: small.verify(weights=wt[eight], **b.host(**cut)))[0] == zkp.ZKP_E_SIZE  # 3 commitments of 2
    two = (b.commits[:2], b.commits_inf[:2])
    c, msg = code(lambda: small.verify(weights=wt[eight], **b.host(commitments=two, **cut)))
    assert c == zkp.ZKP_E_ARG and "opening 2" in msg and "commitment" in msg, msg  # index[2] = 2 of 2 commitments
    c, msg = code(lambda: small.verify(weights=wt[eight], **b.host(commitments=two, **dict(cut, commit_index=None))))
    assert c == zkp.ZKP_E_ARG and "commit_index" in msg, msg  # no index: as many commitments as openings
    import torch
    out = torch.zeros(64, dtype=torch.int64, device="cuda")
    c, msg = code(lambda: small.aggregate_dev(2, 8, dev(b.zs[eight]), dev(b.ys[eight]), dev(wt[eight]), out, out, out, out, commit_index=b.ci[eight]))
    assert c == zkp.ZKP_E_ARG and "opening 2" in msg
    c, msg = code(lambda: small.find_bad(weights=wt[eight], **b.host(commitments=two, **cut)))
    assert c == zkp.ZKP_E_ARG and "opening 2" in msg
    ok = np.array([0, 1, 0, 1, 0, 1, 1, 0], dtype=np.uint32)
    acc = zkp.C.c_int(7)  # null arguments
    args = [small._h, b.commits.ctypes.data, None, 2, 8, ok.ctypes.data, b.zs.ctypes.data, b.ys.ctypes.data, b.proofs.ctypes.data, None, wt.ctypes.data]
    for hole in (1, 6, 7, 8, 10):
        a = list(args)
        a[hole] = None
        assert zkp.lib().zkp_kzg_verify_points(*a, zkp.C.byref(acc)) == zkp.ZKP_E_ARG, hole
    assert zkp.lib().zkp_kzg_verify_points(*args, None) == zkp.ZKP_E_ARG and acc.value == 7
    assert zkp.lib().zkp_kzg_verify_points_find_bad(*args, zkp.C.byref(acc), None) == zkp.ZKP_E_ARG and acc.value == 7
    assert not small.verify(weights=wt[eight], **b.host(commitments=two, **dict(cut, commit_index=ok))), "usable, and this index is wrong"
    small.close()


def test_creation_refusals(zkp, orc):
    g2 = zkp.g2_generator()
    create = zkp.lib().zkp_kzg_point_verifier_create
    handle = zkp.C.c_void_p()
    assert create(None, 8, 2, zkp.C.byref(handle)) == zkp.ZKP_E_ARG and create(g2.ctypes.data, 8, 2, None) == zkp.ZKP_E_ARG
    for max_openings, max_commits in ((0, 1), (1, 0), ((1 << 30) + 1, 1)):
        assert create(g2.ctypes.data, max_openings, max_commits, zkp.C.byref(handle)) == zkp.ZKP_E_ARG and not handle.value
    off = g2.copy()
    off[0] ^= 1
    with pytest.raises(zkp.ZkpError) as ei:
        points_module().KzgPointVerifier(off, 8, 2)
    assert ei.value.code == zkp.ZKP_E_ARG and "[s]_2" in str(ei.value)
    points_module().KzgPointVerifier(g2, 1, 1).close()  # the smallest verifier there is


# ------------------------------------------------------------------------------------------------ the wrappers
def test_kzg_scheme_verify_points_draws_its_weights_and_verify_bytes_decodes(zkp, orc):
    b = batch(zkp, orc, "9 over 3")
    s = zkp.Srs.new_from_secret(orc.fr_from_ints([SECRET])[0], 16)
    scheme = zkp.KzgScheme(s, expand_bases=False)
    args = ((b.commits, b.commits_inf), b.zs, b.ys, (b.proofs, b.proofs_inf))
    assert scheme.verify_points(g2s(zkp, orc), *args, commit_index=b.ci)
    assert scheme.verify_points(g2s(zkp, orc), b.commits, b.zs, b.ys, b.proofs, commit_index=b.ci), "no flags: no identity among them"
    ys = b.ys.copy()
    ys[8] = orc.fr_add(ys[8][None], orc.fr_from_ints([1]))[0]
    assert not scheme.verify_points(g2s(zkp, orc), args[0], b.zs, ys, args[3], commit_index=b.ci)
    assert scheme.verify_points(g2s(zkp, orc), *args, commit_index=b.ci, weights=orc.fr_from_ints(list(range(1, 10))))
    five = batch(zkp, orc, "5 one each")
    assert scheme.verify_points(g2s(zkp, orc), five.commits, five.zs, five.ys, five.proofs), "the identity index"
    assert (scheme._point_verifier[1].max_openings, scheme._point_verifier[1].max_commits) == (9, 5), "grown, not shrunk"
    scheme.close()
    assert scheme._point_verifier is None
    ver = verifier(zkp, orc)
    to_bytes = lambda ints: np.frombuffer(b"".join(v.to_bytes(32, "big") for v in ints), dtype=np.uint8).reshape(-1, 32).copy()
    c48, p48 = zkp.g1_compress(b.commits, b.commits_inf), zkp.g1_compress(b.proofs, b.proofs_inf)
    wt = b.weights(orc, 0x75E0)
    assert ver.verify_bytes(c48, to_bytes(b.zs_int), to_bytes(b.ys_int), p48, wt, commit_index=b.ci)
    bad = list(b.ys_int)
    bad[2] = (bad[2] + 1) % R
    assert not ver.verify_bytes(c48, to_bytes(b.zs_int), to_bytes(bad), p48, wt, commit_index=b.ci)
    with pytest.raises(zkp.ZkpError) as ei:
        ver.verify_bytes(c48, to_bytes(b.zs_int), to_bytes(b.ys_int[:4] + [R] + b.ys_int[5:]), p48, wt, commit_index=b.ci)
    assert ei.value.code == zkp.ZKP_E_ARG and "ys32[4]" in str(ei.value)
