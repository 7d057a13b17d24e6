"""CPU only: the limb-level model of the Fr transform (tests/model/ntt_fr_model.py) against the oracle, the adversarial vectors of
tests/ntt_adversarial.py through that model (every primitive in contract, the words the oracle gives), and the data-independent ceilings
of the lazy reduction against every contract that reads the grown values.

Reach of the vectors, as test_reach measured it (values in units of r; the walk's ceiling is data-independent):

  canonical input (a single pass, a column of pass 0), forward / inverse twiddles
    log_r            4      5      6      7      8      9      10     11
    forward          17.86  21.67  25.48  29.23  33.09  36.77  40.37  44.12
    inverse          17.83  21.81  25.81  29.81  33.71  37.45  41.05  44.89
    64 random tiles  16.64  19.85  23.46  27.05  30.14  32.99  36.52  40.36   (forward)
    ceiling          18     22     26     30     34     38     42     46
  tight input                      vector  64 random tiles  ceiling
    coset pre-scale, radix 2^8     32.78   30.49            36
    coset pre-scale, radix 2^11    43.89   40.34            48
    last pass of 2^12, radix 2^6   25.64   23.03            28
    last pass of 2^16, radix 2^8   33.41   30.42            36
  Tight inputs arrive below 1.4r, not 2r (a product is below a w / 2^261 + r), which is why their ceiling is out of reach.

The mutants (test_mutants): without the normalise at the end of a round every adversarial vector from radix 2^4 up leaves the
multiplier's limb contract at stage 2.  Random words trip that mutant as well, a stage or two later (limbs overflow whatever the values
are); at radix 2^4 some random sets pass.  With sub_tight in place of sub_wide8 in the unit butterfly NO vector leaves a contract or
changes a word: the subtrahend would have to reach 4r - 2^232, and the sum of two arrivals stays below 2.8r.  Only the walk, which takes
the nominal 2r per tight input, refuses that variant."""
import os

import numpy as np
import pytest

import bigmodel as M
import limb_model as L
import ntt_adversarial as A
import ntt_fr_model as N

R = M.R
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def oracle_fr(orc, words, **kw):
    if kw.get("coset") is not None:
        kw["coset"] = A.to_array([kw["coset"]])[0]
    return A.to_ints(orc.ntt_fr(A.to_array(words), **kw))


# ------------------------------------------------------------------------------------------------------------- model validity
@pytest.mark.parametrize("coset", [None, A.COSET], ids=["plain", "coset"])
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("log_n", [1, 2, 3, 4, 5, 6, 7, 8, 11, 12])
def test_model_equals_oracle_on_random_words(orc, log_n, inverse, coset):
    words = A.to_ints(A.random_array(0x30DE1 + log_n, 1 << log_n))
    assert N.ntt_fr(words, inverse=inverse, coset=coset) == oracle_fr(orc, words, inverse=inverse, coset=coset)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
def test_model_equals_oracle_on_the_two_level_table_route(orc, inverse):
    """pass 0's inter-pass twiddle as powtab_get's product of two entries (tight, not canonical) instead of the matrix entry"""
    words = A.to_ints(A.random_array(0x30DE2, 1 << 12))
    assert N.ntt_fr(words, inverse=inverse, matrix=False) == oracle_fr(orc, words, inverse=inverse)


def test_value_twin_follows_the_limb_model():
    """the builder searches on values alone: the same largest value as the limbs, stage by stage, on random and on adversarial words"""
    for log_r, inverse in ((3, False), (6, True), (9, False)):
        tw, twv = N.radix_table(log_r, inverse), N.radix_values(log_r, inverse)
        for words in (A.to_ints(A.random_array(log_r, 1 << log_r)), A.single(log_r, inverse)[0]):
            x = [N.load(words[N.bitrev(e, log_r)]) for e in range(1 << log_r)]
            v = [words[N.bitrev(e, log_r)] for e in range(1 << log_r)]
            trace = N.Trace()
            N.tile(x, log_r, tw, trace=trace)
            assert N.vtile(v, log_r, twv) == trace.max_value
            assert v == [L.v29(e) for e in x]


# ------------------------------------------------------------------------------------------------------------- the vectors in contract
@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("log_n", range(1, 12))
def test_single_pass_vectors_stay_in_contract(orc, log_n, inverse):
    words, reach = A.single(log_n, inverse)
    trace = N.Trace()
    assert N.ntt_fr(words, inverse=inverse, trace=trace) == oracle_fr(orc, words, inverse=inverse)   # inverse: SCALE_CONST on the grown values
    assert trace.max_value == reach


@pytest.mark.parametrize("log_n", [8, 11])
def test_coset_vectors_stay_in_contract(orc, log_n):
    words, reach = A.single_coset(log_n)
    trace = N.Trace()
    assert N.ntt_fr(words, coset=A.COSET, trace=trace) == oracle_fr(orc, words, coset=A.COSET)
    assert trace.max_value == reach
    words, reach = A.single(log_n, True)   # the inverse coset: the same tile as the inverse, then the coset table times 1/n on the grown values
    assert N.ntt_fr(words, inverse=True, coset=A.COSET) == oracle_fr(orc, words, inverse=True, coset=A.COSET)


@pytest.mark.parametrize("inverse", [False, True], ids=["forward", "inverse"])
@pytest.mark.parametrize("name", list(A.PLANTED))
def test_planted_pass0_columns_stay_in_contract(orc, name, inverse):
    """Pass 0 of every multi-pass class on the planted columns: tile, inter-pass product (matrix entry or two-level product), store_tight.
    2^12 runs whole and goes against the oracle; above, the planted columns alone go against the definition of what pass 0 hands on:
    (sum_j x_j w_R^(jk)) w_N^(k i), times 1/n on an inverse."""
    c = A.PLANTED[name]
    a, where = A.planted(name, inverse)
    tr = N.Transform(c["log_n"], inverse, wide=c["wide"], matrix=c["matrix"])
    n, log_r = 1 << c["log_n"], tr.r[0]
    if c["log_n"] == 12:
        words = A.to_ints(a)
        assert tr.run(words) == oracle_fr(orc, words, inverse=inverse)
    w_n = N.root(c["log_n"], inverse)
    scale = pow(n, -1, R) if inverse else 1
    for b, i in where:
        idx = tr.column_indices(0, 0, i)
        words = A.to_ints(a[np.array(idx) + b * n])
        assert words == A.single(log_r, inverse)[0]
        trace = N.Trace()
        got = tr.column(0, 0, i, words, trace)
        assert trace.max_value == A.single(log_r, inverse)[1]
        dft = M.ntt(words, R, inverse)   # (bigmodel scales an inverse by 1 / R0)
        for k, v in enumerate(got):
            assert v < 2 * R and v % R == dft[k] * (len(words) if inverse else 1) * pow(w_n, k * i, R) * scale % R


def test_last_pass_vector_2_12_stays_in_contract(orc):
    a, k0, reach, _ = A.last_pass(12)
    words = A.to_ints(a)
    tr = N.Transform(12)
    data = tr.pass_strided(0, words)
    assert tr.pass_last(data) == oracle_fr(orc, words)
    src, _ = tr.last_indices(k0, 0)
    trace = N.Trace()
    tr.last(k0, 0, [data[j] for j in src], trace)
    assert trace.max_value == reach


def test_last_pass_vector_2_16_stays_in_contract(orc):
    """all of pass 0 on limbs (what arrives at the tile is what store_tight wrote), then the target tile and its 256 output words"""
    a, k0, reach, _ = A.last_pass(16)
    words = A.to_ints(a)
    tr = N.Transform(16)
    data = tr.pass_strided(0, words)
    src, dst = tr.last_indices(k0, 0)
    trace = N.Trace()
    got = tr.last(k0, 0, [data[j] for j in src], trace)
    assert trace.max_value == reach
    ref = oracle_fr(orc, words)
    assert got == [ref[k] for k in dst]


# ------------------------------------------------------------------------------------------------------------- the ceilings
def closed_form(log_r, cls):
    """What the comments state by hand: the input (below r / 2r), then the chain that grows most -- the sum of stage 0, the + 8r of the
    unit butterfly, + 4r per later stage."""
    x = {"canonical": 1, "tight": 2}[cls]
    return (x + 4) * R if log_r == 1 else (2 * x + 8 + 4 * (log_r - 2)) * R


@pytest.mark.parametrize("cls", ["canonical", "tight"])
def test_ceilings_stay_inside_every_contract(cls):
    """Every radix a recorded Fr plan contains, both input classes: inside the tile (multiplier limbs below 2^31, value product at most
    70 r^2, subtrahend limbs under the constant's, no 32-bit wrap) and at what reads the finished tile (check_consumers)."""
    assert N.fr_radices() == list(range(1, 12))
    for log_r in N.fr_radices():
        stages, rows = N.walk(log_r, cls)
        N.check_consumers(rows)
        assert stages == sorted(stages) and closed_form(log_r, cls) - 4 <= stages[-1] < closed_form(log_r, cls)
        assert stages[-1] * N.FACTOR_PRODUCT <= 70 * R * R and N.FACTOR_PRODUCT < 1.015 * R


def test_source_comments_state_the_walks_ceilings():
    """fr29.hpp and ntt.hpp give the bound by hand for radix 2^8 .. 2^11: the figures there are the walk's"""
    csrc = os.path.join(ROOT, "zkp-implementation_amd", "csrc")
    fr29, ntt = open(os.path.join(csrc, "fr29.hpp")).read(), open(os.path.join(csrc, "ntt.hpp")).read()
    for log_r in (8, 9, 10, 11):
        canonical, tight = (-(-N.ceiling(log_r, cls) // R) for cls in ("canonical", "tight"))
        assert "2^%d: %dr / %dr" % (log_r, canonical, tight) in ntt
    assert "12r + 9 * 4r = %dr" % -(-N.ceiling(11, "tight") // R) in ntt
    assert "4r + 8r + 6 * 4r = %dr" % -(-N.ceiling(8, "tight") // R) in fr29


def test_a_third_lazy_stage_would_leave_the_limb_contract():
    """ntt.hpp: "a third lazy stage would need re-normalised limbs" -- the walk agrees: two stages after a fix leave limbs that a third
    stage's product may not take"""
    N.walk(2, "tight", variant="no_fix")   # one round: no stage follows it
    with pytest.raises(L.ContractError, match="limb of the multiplier"):
        N.walk(4, "tight", variant="no_fix")


# ------------------------------------------------------------------------------------------------------------- reach
def test_reach():
    """A condition on the INPUTS: a first-pass vector comes within 2r of the ceiling (log_r 4 .. 11, both twiddle directions); a
    tight-input vector exceeds the largest value of 64 random tiles of its radix and class by at least 2r.  Prints the table of the
    module docstring."""
    lines = []
    for inverse in (False, True):
        for log_r in range(4, 12):
            reach, ceil = A.single(log_r, inverse)[1], N.ceiling(log_r, "canonical")
            lines.append("canonical %s 2^%d: reach %.2f r, 64 random tiles %.2f r, ceiling %.2f r" %
                         ("inverse" if inverse else "forward", log_r, reach / R, N.random_reach(log_r, inverse, "canonical", 77) / R, ceil / R))
            assert ceil - reach <= 2 * R, lines[-1]
    tight = []
    for log_n in (8, 11):
        tight.append(("coset pre-scale 2^%d" % log_n, log_n, A.single_coset(log_n)[1], N.random_reach(log_n, False, "tight", 0x7161 + log_n)))
    for log_n in (12, 16):
        _, _, reach, baseline = A.last_pass(log_n)
        tight.append(("last pass of 2^%d" % log_n, N.Transform(log_n).plan["last"]["log_r"], reach, baseline))
    for what, log_r, reach, baseline in tight:
        lines.append("tight %s (radix 2^%d): reach %.2f r, 64 random tiles %.2f r, ceiling %.2f r" %
                     (what, log_r, reach / R, baseline / R, N.ceiling(log_r, "tight") / R))
        assert reach - baseline >= 2 * R, lines[-1]
    print("\n" + "\n".join(lines))   # (pytest -s shows it)


# ------------------------------------------------------------------------------------------------------------- the tests themselves
def test_mutants():
    """Sanity of these tests, on the model alone.  Without the normalise at the end of a round the adversarial vectors leave the
    multiplier's limb contract.  sub_tight in the unit butterfly is caught by the walk alone (module docstring)."""
    for log_n in (4, 8, 11):
        with pytest.raises(L.ContractError, match="stage 2 .* not below 0x80000000"):
            N.ntt_fr(A.single(log_n, False)[0], variant="no_fix")
    assert N.ntt_fr(A.single_coset(8)[0], coset=A.COSET, variant="unit_sub_tight") == N.ntt_fr(A.single_coset(8)[0], coset=A.COSET)
    N.walk(8, "canonical", variant="unit_sub_tight")
    with pytest.raises(L.ContractError, match="unit butterfly: limb 8 of the subtrahend"):
        N.walk(8, "tight", variant="unit_sub_tight")
