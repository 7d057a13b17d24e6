"""tests/model/msm_reduce_model.py against itself, without a GPU: two bucket sets of c = 8 are reduced in plain Python (limb_model's
adds, S and every U_j by direct summation in logical order), the checker accepts the result, and it rejects -- by window, result and
kind -- every single mutation a wrong reduction could produce.  The same for a folded and a combined bucket, and the layout helpers
round-trip.  tests/test_gpu_msm_reduce.py hands the device's outputs to the same checker."""
import numpy as np
import pytest

import limb_model as L
import msm_reduce_model as RM

C, NB = 8, 128
LIVE = 0b1010010   # the one live bucket of set 1 (0-based index): U_j is that bucket for j in {1, 4, 6} and infinity otherwise


class Case:
    pass


@pytest.fixture(scope="module")
def case(orc):
    s = Case()
    s.orc = orc
    s.pool = pool = RM.Pool(orc, seed=0xC0DE, nbase=16)
    rnd = np.random.RandomState(7)
    m0 = rnd.randint(0, len(pool), NB)                      # every form, infinity included
    m0[10], m0[11] = pool.idx(3, RM.Z), pool.idx(3, RM.Z2)  # an equal pair under two z: a doubling inside S
    m0[20], m0[21] = pool.idx(5, RM.WORST), pool.idx(5, RM.NEG)
    m1 = np.full(NB, pool.INF)
    m1[LIVE] = pool.idx(9, RM.WORST)
    s.maps = np.stack([m0, m1])
    s.logs = RM.result_logs(pool.logs(s.maps))
    flat = RM.points_of_logs(orc, [k for row in s.logs for k in row])
    s.want = [flat[w * C:(w + 1) * C] for w in range(2)]
    s.words = np.stack([RM.reduce_by_adds(pool.gather(m)) for m in s.maps])   # (2, C, 64)
    return s


def words_of_log(s, k, **kw):
    pt = RM.points_of_logs(s.orc, [k])[0]
    return np.zeros(64, dtype=np.uint32) if pt is None else RM.words_of(L.x28_from_point(pt, **kw))


def rejected(s, words, *names, want=None):
    with pytest.raises(AssertionError) as e:
        RM.check_results(words, want or s.want)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_the_model_reduces_to_what_the_maps_say(case):
    s = case
    RM.check_results(s.words, s.want)
    # the live-bucket set: U_j is the bucket itself where bit j of its index is set, infinity elsewhere
    for j in range(C - 1):
        assert (s.want[1][1 + j] is not None) == bool((LIVE >> j) & 1)
        assert s.logs[1][1 + j] == (s.logs[1][0] if (LIVE >> j) & 1 else 0)
    assert s.want[1][0] == s.pool.pt[s.pool.idx(9, RM.WORST)]
    assert all(p is not None for p in s.want[0])


def test_two_results_of_a_window_swapped(case):
    w = case.words.copy()
    w[0, [2, 5]] = w[0, [5, 2]]
    rejected(case, w, "window 0, result 2", "U_1: odd half of level 1")


def test_the_results_of_two_windows_swapped(case):
    rejected(case, case.words[::-1].copy(), "window 0, result 0 (sum)")


def test_u_j_with_one_bucket_too_many(case):
    s, j = case, 3
    extra = next(i for i in range(NB) if not (i >> j) & 1 and s.maps[0][i] != s.pool.INF)
    w = s.words.copy()
    w[0, 1 + j] = words_of_log(s, s.logs[0][1 + j] + s.pool.k[s.maps[0][extra]], z=5)
    rejected(s, w, "window 0, result 4", "U_3: odd half of level 3")


def test_u_j_built_on_the_next_bit(case):
    s, j = case, 2
    w = s.words.copy()
    w[0, 1 + j] = s.words[0, 2 + j]
    rejected(s, w, "window 0, result 3", "U_2: odd half of level 2")


def test_an_equal_point_with_x_past_14p(case):
    s = case
    w = s.words.copy()
    w[0, 6] = words_of_log(s, s.logs[0][6], z=3, kx=14)
    assert L.affine_of(RM.point_of(w[0, 6])) == s.want[0][6]      # the same point: only the invariant is broken
    rejected(s, w, "window 0, result 6", "U_5", "not a stored point", "14p")
    w[0, 6] = words_of_log(s, s.logs[0][6], z=3, kx=13)           # the worst representative the invariant admits passes
    RM.check_results(w, s.want)


def test_infinity_and_not(case):
    s = case
    e = next(1 + j for j in range(C - 1) if not (LIVE >> j) & 1)
    w = s.words.copy()
    w[1, e] = s.words[1, 0]                                       # a point where infinity is expected
    rejected(s, w, f"window 1, result {e}", "expected infinity")
    w = s.words.copy()
    w[1, 0] = 0                                                   # infinity where a point is expected
    rejected(s, w, "window 1, result 0 (sum)", "is infinity")


def test_unwritten_words_are_no_stored_point(case):
    w = case.words.copy()
    w[1, 3] = 0xFFFFFFFF                                          # what the hook's 0xFF fill leaves where no launch wrote
    rejected(case, w, "window 1, result 3", "not a stored point")


# ---- fold and combine ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def buckets(case):
    """four buckets of one set, each the sum of three parts; bucket 3 is also a combine of 5 pieces and a carry"""
    s = case
    pool = s.pool
    b = Case()
    b.part_maps = np.array([[pool.idx(1), pool.idx(2, RM.Z), pool.INF, pool.idx(4, RM.NEG)],
                            [pool.INF, pool.idx(2, RM.Z2), pool.idx(6, RM.WORST), pool.idx(4)],
                            [pool.idx(7, RM.Z), pool.idx(8), pool.idx(6, RM.WORST), pool.INF]])
    b.piece_map = [pool.idx(j, RM.Z) for j in (10, 11, 11, 12, 13)]
    b.carry = pool.idx(14, RM.WORST)
    return b


def fold_by_adds(pool, part_maps):
    return np.stack([RM.words_of(RM.add_all([RM.point_of(pool.words[m]) for m in col])) for col in np.asarray(part_maps).T])[None]


def test_folded_buckets(case, buckets):
    s, b = case, buckets
    want = [RM.points_of_logs(s.orc, RM.fold_logs(s.pool.logs(b.part_maps)).tolist())]
    assert want[0][3] is None                                     # -P + P + infinity
    RM.check_buckets(fold_by_adds(s.pool, b.part_maps), want)
    with pytest.raises(AssertionError) as e:                      # a fold that lost one part
        RM.check_buckets(fold_by_adds(s.pool, b.part_maps[:2]), want)
    assert "window 0, bucket 1" in str(e.value)
    short = b.part_maps.copy()
    short[2, 2] = s.pool.INF                                      # ... of one bucket only
    with pytest.raises(AssertionError) as e:
        RM.check_buckets(fold_by_adds(s.pool, short), want)
    assert "window 0, bucket 3" in str(e.value)


def test_combined_bucket(case, buckets):
    s, b = case, buckets
    pool = s.pool
    pts = lambda idx: [RM.point_of(pool.words[m]) for m in idx]
    full = RM.combine_log([pool.k[m] for m in b.piece_map], pool.k[b.carry])
    want = [[None, None, RM.points_of_logs(s.orc, [full])[0]]]

    def words(piece_idx, carry_idx):
        w = np.zeros((1, 3, 64), dtype=np.uint32)
        w[0, 2] = RM.words_of(RM.add_all(pts(list(piece_idx) + list(carry_idx)), quad=True))
        return w

    RM.check_buckets(words(b.piece_map, [b.carry]), want, only=[(0, 2)])
    for bad in (words(b.piece_map[:-1], [b.carry]), words(b.piece_map, [])):   # the last piece missing; the carry missing
        with pytest.raises(AssertionError) as e:
            RM.check_buckets(bad, want, kind="combined bucket", only=[(0, 2)])
        assert "window 0, combined bucket 3" in str(e.value)
    assert RM.combine_log([pool.k[m] for m in b.piece_map]) != full


# ---- layouts -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [2, 128, 256])
def test_layout_round_trips(nb):
    i = np.arange(nb)
    pos = RM.pyr_pos(i, nb)
    assert sorted(pos.tolist()) == list(range(nb))                          # a permutation:
    assert np.array_equal(pos[0::2], np.arange(nb // 2)) and np.array_equal(pos[1::2], nb // 2 + np.arange(nb // 2))  # evens first
    assert [RM.pyr_pos(int(k), nb) for k in i] == pos.tolist()
    W = 3
    sets = np.random.RandomState(nb).randint(0, 1 << 32, (W, nb, 64), dtype=np.uint64).astype(np.uint32)
    planes = RM.pack_planes(sets)
    assert planes.shape == (16, W * nb, 4)
    # chunk q of bucket i + 1 of set w sits at uint4 index q cap + w nb + pyr_pos(i, nb)
    for w, k, q in ((0, 0, 0), (1, 1, 5), (2, nb - 1, 15), (1, nb // 2, 7)):
        assert np.array_equal(planes[q, w * nb + RM.pyr_pos(k, nb)], sets[w, k, 4 * q:4 * q + 4])
    assert np.array_equal(RM.unpack_planes(planes, W, nb), sets)
    assert np.array_equal(RM.unpack_planes(planes.reshape(-1), W, nb), sets)
    phys = RM.to_physical(sets)
    assert np.array_equal(phys[2 * nb + RM.pyr_pos(1, nb)], sets[2, 1])
    assert np.array_equal(RM.from_physical(phys, W, nb), sets)
    assert np.array_equal(RM.entries_of_planes(RM.planes_of_entries(phys)), phys)


def test_result_logs_by_hand():
    rows = RM.result_logs([[1, 10, 100, 1000]])                   # c = 3: S, U_0 (odd indices), U_1 (indices 2, 3)
    assert rows == [[1111, 1010, 1100]]
    assert RM.result_logs([[RM.R - 1, 1]]) == [[0, 1]]
