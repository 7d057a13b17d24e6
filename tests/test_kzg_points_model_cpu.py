"""The big-integer model of the batched point-opening verification (tests/model/kzg_points_model.py) against the definition: its
four outputs against plain sums, the batched equation in scalars against openings the CPU oracle divides out in coefficient form
(y = f(z), q = (f - y) / (X - z), both the oracle's), every single-word corruption of an honest batch, and the bisection.  The GPU
tests compare the device with this model bit for bit."""
import random

import pytest

import kzg_points_model as pm

R = pm.R
S = 0x1F2E3D4C5B6A7988


def evaluate(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc


def openings(orc, seed, count, n_commits, degree=12):
    """count openings over n_commits polynomials, opened by the oracle -> commit scalars f_m(s), index, zs, ys, proof scalars q_i(s)"""
    rng = random.Random(seed)
    polys = [orc.rand_fr(seed + 17 * m, degree) for m in range(n_commits)]
    index = [rng.randrange(n_commits) for _ in range(count)]
    zs = [rng.randrange(R) for _ in range(count)]
    ys, qs = [], []
    for m, z in zip(index, zs):
        zl = orc.fr_from_ints([z])[0]
        ys.append(orc.fr_to_ints(orc.poly_eval_fr(polys[m], zl)[None])[0])
        qs.append(evaluate(orc.fr_to_ints(orc.poly_div_linear_fr(polys[m], zl)), S))
    return [evaluate(orc.fr_to_ints(f), S) for f in polys], index, zs, ys, qs


@pytest.mark.parametrize("count", [1, 2, 9, 255, 256, 257, 600])
def test_outputs_are_the_plain_sums(count):
    rng = random.Random(0x7400 + count)
    for n_commits, index in ((count, None), (1, [0] * count), (count + 1, list(range(count))), (3, [rng.choice((0, 0, 0, 2)) for _ in range(count)])):
        zs = [rng.randrange(R) for _ in range(count)]
        ys = [rng.randrange(1 << 256) for _ in range(count)]  # not canonical: reduced by the arithmetic
        ws = [rng.randrange(1 << 128) for _ in range(count)]
        ws[0], zs[-1], ys[count // 2] = R - 1, 0, 0
        for chunk_log in (0, 4):
            cw, rz, r, neg = pm.aggregate(n_commits, index, zs, ys, ws, chunk_log)
            names = index if index is not None else list(range(count))
            assert cw == [sum(w for w, m in zip(ws, names) if m == c) % R for c in range(n_commits)]
            assert rz == [w * z % R for w, z in zip(ws, zs)] and r == ws
            assert neg == (-sum(w * y for w, y in zip(ws, ys))) % R
            assert all(0 <= v < R for v in cw + rz + r + [neg])


@pytest.mark.parametrize("count,n_commits", [(1, 1), (2, 2), (9, 3)])
def test_honest_openings_of_the_oracle_accept_and_every_corrupted_word_rejects(orc, count, n_commits):
    cs, index, zs, ys, qs = openings(orc, 0x7410 + count, count, n_commits)
    rng = random.Random(0x7420 + count)
    ws = [rng.randrange(1, 1 << 128) for _ in range(count)]
    for chunk_log in (0, 4):
        assert pm.accepts(S, cs, qs, n_commits, index, zs, ys, ws, chunk_log)
    assert pm.accepts(S, cs, qs, n_commits, index, zs, ys, [rng.randrange(R) for _ in range(count)]), "whatever the weights"
    if count == n_commits:  # the identity index: commitment i for opening i
        by_opening = [cs[m] for m in index]
        assert pm.accepts(S, by_opening, qs, count, None, zs, ys, ws)
    used = sorted(set(index))
    for what, values in (("y", ys), ("z", zs), ("proof", qs), ("commitment", cs)):
        for at in (range(count) if what != "commitment" else used):
            for word in range(4):
                bad = list(values)
                bad[at] = (bad[at] ^ (1 << (64 * word + rng.randrange(62)))) % R
                if bad[at] == values[at]:
                    bad[at] = (bad[at] + 1) % R
                args = {"y": (cs, qs, zs, bad), "z": (cs, qs, bad, ys), "proof": (cs, bad, zs, ys), "commitment": (bad, qs, zs, ys)}[what]
                assert not pm.accepts(S, args[0], args[1], n_commits, index, args[2], args[3], ws), (what, at, word)
    zero = list(ws)
    zero[0] = 0
    bad = list(ys)
    bad[0] = (bad[0] + 1) % R
    assert pm.accepts(S, cs, qs, n_commits, index, zs, bad, zero), "a weight of 0 drops its opening"


def test_bisection_finds_the_lowest_failing_opening(orc):
    count, n_commits = 37, 3
    cs, index, zs, ys, qs = openings(orc, 0x7430, count, n_commits, degree=6)
    ws = [random.Random(0x7440 + i).randrange(1, 1 << 128) for i in range(count)]
    assert pm.find_bad(S, cs, qs, n_commits, index, zs, ys, ws) == (pm.SIZE_MAX, 1)
    for bad_set, want in (({0}, 0), ({36}, 36), ({17, 30}, 17), (set(range(37)), 0)):
        bad = [(y + 1) % R if i in bad_set else y for i, y in enumerate(ys)]
        got, checks = pm.find_bad(S, cs, qs, n_commits, index, zs, bad, ws)
        assert got == want and checks <= 1 + 6, (bad_set, got, checks)  # ceil(log2 37) = 6
    one = pm.find_bad(S, [cs[index[0]]], qs[:1], 1, None, zs[:1], [(ys[0] + 1) % R], ws[:1])
    assert one == (0, 1), "a batch of one that fails names opening 0 without a further check"
