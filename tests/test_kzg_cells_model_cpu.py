"""The big-integer model of the batched cell verification's field half (tests/model/kzg_cells_model.py) against the definition: the
identity sum_k (F mod (X^l - rho^k)) = r (F mod X^l) that turns the sum of the weighted interpolants into one inverse transform of
n, pinned against g1_coset_model.interpolant; the grouping with its chunks; and the batched equation itself with integers standing in
for points.  The GPU tests compare the device with this model bit for bit."""
import random

import pytest

import g1_coset_model as cm
import kzg_cells_model as km

R = km.R
SHAPES = [(4, 1), (5, 0), (6, 3), (7, 6)]


def cell_sets(rng, r, commits):
    """[(commit_index, coset_index)]: random with repeated cosets, the same cell twice, unused cosets, one coset only, one cell"""
    out = []
    cells = [(rng.randrange(commits), rng.randrange(r)) for _ in range(11)]
    cells[7] = cells[2]  # the same cell twice
    out.append(cells)
    out.append([(rng.randrange(commits), 0 if i % 2 else r - 1) for i in range(9)])  # two cosets in use, the others unused
    out.append([(i % commits, r // 2) for i in range(6)])  # one coset
    out.append([(commits - 1, rng.randrange(r))])  # one cell
    out.append([(m, k) for m in range(commits) for k in range(r)])  # every cell of every commitment
    return [([c[0] for c in s], [c[1] for c in s]) for s in out]


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_one_inverse_transform_gives_the_sum_of_the_interpolants(log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    r, commits = n // l, 3
    rng = random.Random(0x7200 + 16 * log_n + log_l)
    for commit_index, coset_index in cell_sets(rng, r, commits):
        cells = len(coset_index)
        evals = [[rng.randrange(R) for _ in range(l)] for _ in range(cells)]  # (no polynomial behind them: the identity needs none)
        weights = [rng.randrange(R) for _ in range(cells)]
        weights[0] = 0 if cells > 3 else weights[0]
        direct = km.interpolant_sum(log_n, log_l, coset_index, evals, weights)
        for chunk_log in (0, 1, 3):
            interp, cw, ps = km.aggregate(log_n, log_l, commits, commit_index, coset_index, evals, weights, chunk_log)
            assert interp == direct, (cells, chunk_log)
            assert cw == [sum(w for w, m in zip(weights, commit_index) if m == c) % R for c in range(commits)]
            assert ps == [w * pow(km.root(log_n), l * k, R) % R for w, k in zip(weights, coset_index)]
        a = km.vector_a(log_n, log_l, coset_index, evals, weights)
        for k in set(range(r)) - set(coset_index):
            assert not any(a[k::r]), "a coset no cell names stays zero"


@pytest.mark.parametrize("chunk_log", [0, 1, 2, 5])
def test_grouping_is_stable_and_chunks_stay_inside_segments(chunk_log):
    rng = random.Random(0x7210 + chunk_log)
    for count, cells in ((1, 9), (4, 1), (8, 40), (16, 16), (3, 0)):
        keys = [rng.randrange(count) for _ in range(cells)]
        for compact in (True, False):
            order, chunk_start, used, seg = km.sort_with_chunks(keys, count, chunk_log, compact)
            assert sorted(order) == list(range(cells))
            assert [keys[i] for i in order] == sorted(keys) and all(a < b for a, b in zip(order, order[1:]) if keys[a] == keys[b])
            assert chunk_start[0:1] in ([0], [cells]) and chunk_start[-1] == cells
            names = used if compact else list(range(count))
            assert len(seg) == len(names) + 1 and seg[-1] == len(chunk_start) - 1
            for u, k in enumerate(names):
                got = [i for q in range(seg[u], seg[u + 1]) for i in order[chunk_start[q]:chunk_start[q + 1]]]
                assert got == [i for i in range(cells) if keys[i] == k]
                for q in range(seg[u], seg[u + 1]):
                    assert 1 <= chunk_start[q + 1] - chunk_start[q] <= 1 << chunk_log
            if compact:
                assert used == sorted(set(keys))
            assert len(chunk_start) - 1 <= km.max_chunks(cells, count, chunk_log)


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_batched_equation_with_integers_for_points(log_n, log_l):
    """[a]G is a: a proof is q_k(s), a commitment f(s), and the equation reads  L s^l == right  in Fr.  Honest batches satisfy it
    whatever the weights; one altered evaluation does not (for these weights)."""
    n, l = 1 << log_n, 1 << log_l
    r, s = n // l, 0x1F2E3D4C5B6A7988
    rng = random.Random(0x7220 + 16 * log_n + log_l)
    polys = [[rng.randrange(R) for _ in range(n)], [rng.randrange(R) for _ in range(l)], [0]]
    values = [cm.transform(list(f) + [0] * (n - len(f))) for f in polys]
    proofs = [[cm.evaluate(cm.quotient(f, n, l, k), s) for k in range(r)] for f in polys]
    commits = [cm.evaluate(f, s) for f in polys]
    assert not any(proofs[1]) and commits[2] == 0
    cells = [(m, k) for m in range(3) for k in range(r)]
    rng.shuffle(cells)
    cells = cells[:12] + cells[:2]
    commit_index, coset_index = [c[0] for c in cells], [c[1] for c in cells]
    evals = [values[m][k::r] for m, k in cells]
    weights = [rng.randrange(1 << 128) for _ in cells]

    def holds(ev):
        interp, cw, ps = km.aggregate(log_n, log_l, 3, commit_index, coset_index, ev, weights, 1)
        left = sum(w * proofs[m][k] for w, (m, k) in zip(weights, cells)) % R
        right = (sum(c * x for c, x in zip(cw, commits)) - cm.evaluate(interp, s) + sum(p * proofs[m][k] for p, (m, k) in zip(ps, cells))) % R
        return left * pow(s, l, R) % R == right

    assert holds(evals)
    bad = [list(e) for e in evals]
    bad[3][l - 1] = (bad[3][l - 1] + 1) % R
    assert not holds(bad)
