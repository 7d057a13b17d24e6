"""The host model of the MSM's digit recoding and sort (tests/model/msm_sort_model.py) checks itself, and its checker bites: it accepts
a valid set of stage outputs for three small geometries and rejects each of a list of single corruptions, one assertion each.  This is
what shows that tests/test_gpu_msm_sort.py would fail on a subtly wrong kernel -- without breaking a kernel on a GPU."""
import copy
import random

import numpy as np
import pytest

import msm_sort_model as S

FILL = S.FILL


def random_scalars(seed, n):
    rnd = random.Random(seed)
    return [rnd.randrange(S.R) for _ in range(n)]


class Case:
    def __init__(self, g, scalars, inf=None):
        self.g = g
        self.digits = S.reference_digits(g, scalars, inf)
        self.out = S.reference_outputs(g, self.digits)


@pytest.fixture(scope="module")
def c8():
    """per-window c = 8, 2^14 scalars: run_limit 512 > 255, so the saturated size class holds candidates that get no pieces"""
    n = 1 << 14
    g = S.model_geometry(1, n, c=8)
    assert g["run_limit"] == 512 and g["piece"] == 128 and g["nhi"] == 1 and g["nwin"] == 32
    sc = S.plant_c8_buckets(g, random_scalars(0xC8, n), S.edge_scalars(g["off"]))
    inf = np.zeros(n, dtype=np.uint8)
    inf[-3:] = 1  # the flagged bases sit behind the planted buckets' scalars
    return Case(g, [sc], inf)


@pytest.fixture(scope="module")
def c16():
    """per-window c = 16: 128 partitions of 256 bins, a batch of two"""
    n = 3000
    g = S.model_geometry(2, n, c=16)
    assert g["nhi"] == 128 and g["lo_bits"] == 8 and g["nwin"] == 32
    a, b = random_scalars(0xC16, n), random_scalars(0xC17, n)
    edge = S.edge_scalars(g["off"])
    a[:len(edge)] = edge
    inf = np.zeros(n, dtype=np.uint8)
    inf[[7, 100, n - 1]] = 1
    return Case(g, [a, b], inf)


@pytest.fixture(scope="module")
def shared11():
    """shared bucket set over bases expanded at 11 bits: 24 slices of 11 and 10 bits, one scalar shared by half the terms"""
    n = 1500
    off = S.balanced_slice_offsets(256, 11)
    g = S.model_geometry(1, n, slice_off=off)
    assert g["c"] == 11 and g["nslice"] == 24 and {off[s + 1] - off[s] for s in range(24)} == {10, 11} and g["nhi"] == 4
    sc = random_scalars(0x511, n)
    edge = S.edge_scalars(off)
    sc[:len(edge)] = edge
    sc[1::2] = [sc[-1]] * len(sc[1::2])
    return Case(g, [sc])


def test_checker_accepts_the_reference_outputs(c8, c16, shared11):
    for case in (c8, c16, shared11):
        S.check_sort_outputs(case.g, case.digits, case.out)


def test_planted_buckets_are_what_the_corruptions_need(c8):
    g, t = c8.g, S._window_truth(c8.g, 0, c8.digits[0].astype(np.int64))
    assert list(t["counts"][:4]) == [255, g["run_limit"], g["run_limit"] + 1, 3 * g["piece"] + 1]
    assert int(c8.out["over"][0][0]) == 4 and int(c8.out["over"][0][1]) == 5  # four saturated candidates, one of them oversized: 513 / 128
    assert t["total"] < g["n"]  # (the flagged bases)


def test_digit_model_on_the_edge_scalars():
    for off in ([8 * s for s in range(33)], [16 * s for s in range(17)], S.balanced_slice_offsets(256, 11), S.balanced_slice_offsets(256, 20),
                S.balanced_slice_offsets(256, 19)):
        for k in S.edge_scalars(off):
            assert k < S.R
            digits, carry = S.recode(k, off)
            S.check_recoding(k, off, digits, carry)
        top = 1 << (off[1] - 1)
        assert S.recode(top, off)[0][0] == top and S.recode(top + 1, off)[0][:2] == [top + 1 - 2 * top, 1]  # largest positive, first negative
    off = S.balanced_slice_offsets(129, 16)
    for k in S.edge_scalars(off, glv=True) + [S.LAMBDA, S.LAMBDA - 1, S.LAMBDA + 1]:
        assert k < S.R
        for half in (k % S.LAMBDA, k // S.LAMBDA):
            digits, carry = S.recode(half, off)
            S.check_recoding(half, off, digits, carry)
    g = S.model_geometry(1, 4, slice_off=off, glv=True)
    d = S.reference_digits(g, [[S.R - 1, S.LAMBDA, 5, 0]], [0, 0, 1, 0]).reshape(2, g["nslice"], 4)
    assert d[0, 0, 1] == 0 and d[1, 0, 1] == 2 and not d[:, :, 2].any() and not d[:, :, 3].any()  # lambda = 0 + 1 lambda; an infinity base; 0


def test_encoding():
    assert [S.encode(d) for d in (0, 1, -1, 128, -127)] == [0, 2, 3, 256, 255]
    # an all-ones slice with a carry coming in is the digit 0 with a carry out: the skip word 0, never a "negative zero" 1
    digits, carry = S.recode(0xFFFF, [0, 8, 16, 24])
    assert digits == [-1, 0, 1] and carry == 0 and [S.encode(d) for d in digits] == [3, 0, 2]


# ---- single corruptions: each takes a deep copy of a valid set and returns (window, stage the checker must name)
def _nonempty_buckets(case, w):
    t = S._window_truth(case.g, w, case.digits[w].astype(np.int64))
    return t, np.flatnonzero(t["counts"]) + 1


def drop_sign(case, o):
    w = 1
    t, _ = _nonempty_buckets(case, w)
    pos = int(np.flatnonzero(o["sorted"][w, :t["total"]] >> 31)[0])
    o["sorted"][w, pos] &= 0x7FFFFFFF
    return w, "sorted"


def swap_buckets(case, o):
    w = min(1, case.g["nwin"] - 1)
    t, bs = _nonempty_buckets(case, w)
    p, q = int(t["start"][bs[0]]), int(t["start"][bs[-1]])
    o["sorted"][w, [p, q]] = o["sorted"][w, [q, p]]
    return w, "sorted"


def duplicate_index(case, o):
    p = int(S._window_truth(case.g, 0, case.digits[0].astype(np.int64))["start"][1])  # bucket 1 of window 0: 255 entries, all positive
    o["sorted"][0, p + 1] = o["sorted"][0, p]
    return 0, "sorted"


def start_off_by_one(case, o):
    o["start"][2, 5] += 1
    return 2, "start"


def start_total_short(case, o):
    o["start"][2, case.g["nb"] + 1] -= 1
    return 2, "start"


def write_past_total(case, o):
    t, _ = _nonempty_buckets(case, 3)
    assert t["total"] < case.g["n"]
    o["sorted"][3, t["total"]] = 0
    return 3, "sorted"


def swap_perm_classes(case, o):
    nb = case.g["nb"]
    o["perm"][0, [0, nb - 1]] = o["perm"][0, [nb - 1, 0]]
    return 0, "perm"


def perm_missing_bucket(case, o):
    o["perm"][4, 3] = o["perm"][4, 4]
    return 4, "perm"


def ghist_moved(case, o):
    k = int(np.flatnonzero(o["ghist"][5])[0])
    o["ghist"][5, k] -= 1
    o["ghist"][5, k + 1] += 1
    return 5, "ghist"


def piece_too_long(case, o):
    o["desc"][0, 1, 3] += 1
    return 0, "desc"


def missing_last_piece(case, o):
    n_over, n_pieces = (int(v) for v in o["over"][0])
    o["over"][0, 1] = n_pieces - 1
    o["over_off"][0, n_over] = n_pieces - 1
    o["desc"][0, n_pieces - 1] = FILL
    return 0, "over_off"


def piece_for_a_small_candidate(case, o):
    """bucket 4 (3 piece + 1 entries: saturated class, under run_limit) gets the pieces its size would ask for"""
    g = case.g
    n_over, n_pieces = (int(v) for v in o["over"][0])
    r = int(np.flatnonzero(o["over_b"][0, :n_over] == 4)[0])
    t = S._window_truth(g, 0, case.digits[0].astype(np.int64))
    at, extra = int(o["over_off"][0, r]), 4
    rows = [(4, p, int(t["start"][4]) + p * g["piece"], min(int(t["start"][4]) + (p + 1) * g["piece"], int(t["start"][5]))) for p in range(extra)]
    desc = np.concatenate([o["desc"][0, :at], np.array(rows, dtype=np.uint32), o["desc"][0, at:n_pieces]])
    o["desc"][0, :n_pieces + extra] = desc
    o["over_off"][0, r + 1:n_over + 1] += extra
    o["over"][0, 1] = n_pieces + extra
    return 0, "over_off"


def over_b_against_perm(case, o):
    o["over_b"][0, [0, 1]] = o["over_b"][0, [1, 0]]
    return 0, "over_b"


def wrong_partition(case, o):
    w = min(1, case.g["nwin"] - 1)
    t, _ = _nonempty_buckets(case, w)
    hs = np.flatnonzero(t["pcount"])
    p, q = int(t["pstart"][hs[0]]), int(t["pstart"][hs[-1]])
    o["entries"][w, [p, q]] = o["entries"][w, [q, p]]
    return w, "entries"


def entry_lost(case, o):
    t, _ = _nonempty_buckets(case, 1)
    o["entries"][1, t["total"] - 1] = FILL
    return 1, "entries"


CORRUPTIONS = [("c8", drop_sign), ("c8", swap_buckets), ("c8", duplicate_index), ("c8", start_off_by_one), ("c8", start_total_short),
               ("c8", write_past_total), ("c8", swap_perm_classes), ("c8", perm_missing_bucket), ("c8", ghist_moved), ("c8", piece_too_long),
               ("c8", missing_last_piece), ("c8", piece_for_a_small_candidate), ("c8", over_b_against_perm), ("c16", wrong_partition),
               ("c16", entry_lost), ("shared11", swap_buckets), ("shared11", wrong_partition)]


@pytest.mark.parametrize("fixture,corrupt", CORRUPTIONS, ids=[f"{f}-{c.__name__}" for f, c in CORRUPTIONS])
def test_checker_rejects_a_single_corruption(request, fixture, corrupt):
    case = request.getfixturevalue(fixture)
    o = copy.deepcopy(case.out)
    w, stage = corrupt(case, o)
    assert any(not np.array_equal(o[k], case.out[k]) for k in o), "the corruption changed nothing"
    with pytest.raises(S.SortContractError) as ei:
        S.check_sort_outputs(case.g, case.digits, o)
    assert ei.value.window == w and ei.value.stage == stage, str(ei.value)
    S.check_sort_outputs(case.g, case.digits, case.out)  # the original is untouched and still valid


def test_tiling_property_alone(c8):
    """The tiling check on its own: a descriptor set that a wrong `piece` would give (pieces twice as long) passes every table
    comparison once those are told the same wrong piece, but not a checker that knows the plan's."""
    g2 = dict(c8.g, piece=2 * c8.g["piece"])
    o = S.reference_outputs(g2, c8.digits)
    with pytest.raises(S.SortContractError):
        S.check_sort_outputs(c8.g, c8.digits, o)


def test_caps_are_a_condition(c8):
    with pytest.raises(S.SortContractError) as ei:
        S.check_sort_outputs(dict(c8.g, over_cap=3), c8.digits, {k: (v[:, :3] if k == "over_b" else v[:, :4] if k == "over_off" else v)
                                                                 for k, v in c8.out.items()})
    assert ei.value.stage == "plan"
