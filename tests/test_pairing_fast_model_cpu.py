"""The fast pairing model (tests/model/pairing_fast_model.py: prepared lines, sparse product, Frobenius, cyclotomic squaring, inverse,
x-chain final exponentiation) pinned to the plain model (pairing_model.py).  A model pairing costs most of a second: a handful each."""
import random

import pytest

import bigmodel as M
import pairing_fast_model as FM
import pairing_model as PM

P, R = M.P, M.R


def rand_f12(seed):
    rng = random.Random(seed)
    c = [rng.randrange(P) for _ in range(12)]
    return (((c[0], c[1]), (c[2], c[3]), (c[4], c[5])), ((c[6], c[7]), (c[8], c[9]), (c[10], c[11])))


@pytest.fixture(scope="module")
def miller_g():
    return PM.miller_loop(M.G1, PM.G2)


def test_hard_part_identity():
    """lambda_0 + lambda_1 p + lambda_2 p^2 + lambda_3 p^3 = 3 (p^4 - p^2 + 1) / r, hence E is the cube of the plain exponent"""
    assert (P ** 4 - P ** 2 + 1) % R == 0
    assert FM.LAMBDA0 + FM.LAMBDA1 * P + FM.LAMBDA2 * P ** 2 + FM.LAMBDA3 * P ** 3 == 3 * (P ** 4 - P ** 2 + 1) // R
    assert (P ** 6 - 1) * (P ** 2 + 1) * (P ** 4 - P ** 2 + 1) == P ** 12 - 1
    assert FM.N_STEPS == 68 and bin(FM.DBL_MASK).count("1") == 63


def test_frobenius_constants_against_pow():
    f = rand_f12(1)
    assert PM.f2_mul(FM.f2_pow(FM.XI, (P - 1) // 6), FM.f2_pow(FM.XI, (P - 1) // 6)) == FM.GAMMA[1][2]
    assert FM.f2_pow(FM.GAMMA[1][1], 6) == FM.f2_pow(FM.XI, P - 1)          # (w^(p-1))^6 = xi^(p-1)
    assert all(g[1] == 0 for g in FM.GAMMA[2])                              # the p^2 constants lie in Fq
    assert FM.f12_frobenius(f, 1) == PM.f12_pow(f, P)
    assert FM.f12_frobenius(f, 2) == FM.f12_frobenius(FM.f12_frobenius(f, 1), 1)
    assert FM.f12_frobenius(f, 3) == FM.f12_frobenius(FM.f12_frobenius(f, 2), 1)


def test_inverse_and_sparse_product():
    f = rand_f12(2)
    assert PM.f12_mul(f, FM.f12_inv(f)) == PM.F12_ONE
    assert FM.f12_inv((PM.F6_ZERO, PM.F6_ZERO)) == (PM.F6_ZERO, PM.F6_ZERO)
    rng = random.Random(3)
    a, b, c = (rng.randrange(P), rng.randrange(P)), (rng.randrange(P), rng.randrange(P)), rng.randrange(P)
    assert FM.f12_mul_line(f, a, b, c) == PM.f12_mul(f, FM.line_as_f12(a, b, c))
    assert FM.f12_mul_line(f, PM.F2_ZERO, (P - 1, 0), 1) == PM.f12_mul(f, FM.line_as_f12(PM.F2_ZERO, (P - 1, 0), 1))


def test_cyclotomic_square_needs_the_easy_part():
    f = rand_f12(4)
    m = FM.easy_part(f)
    assert m == PM.f12_pow(f, (P ** 6 - 1) * (P ** 2 + 1))
    assert FM.f12_cyclotomic_sqr(m) == PM.f12_mul(m, m)
    assert FM.f12_cyclotomic_sqr(f) != PM.f12_mul(f, f)     # outside the subgroup the two differ: the test tells them apart
    assert PM.f12_mul(m, PM.f12_conj(m)) == PM.F12_ONE      # there the conjugate is the inverse


def test_final_exp_is_the_cube_of_the_plain_exponent(miller_g):
    f = rand_f12(5)
    assert FM.final_exp(f) == PM.f12_pow(f, 3 * PM.FINAL_EXP)
    assert FM.final_exp(miller_g) == PM.f12_pow(miller_g, 3 * PM.FINAL_EXP)
    assert FM.final_exp(PM.F12_ONE) == PM.F12_ONE


def test_prepared_miller_loop_matches_one_pair(miller_g):
    lines = FM.prepare_g2(PM.G2)
    assert len(lines) == 68
    assert FM.miller_product([M.G1], [lines]) == miller_g
    assert FM.miller_product([None], [lines]) == PM.F12_ONE
    assert FM.miller_product([M.G1], [None]) == PM.F12_ONE


def test_prepared_miller_loop_matches_product_of_three(miller_g):
    ps = [M.G1, M.g1_mul(M.G1, 5), M.g1_mul(M.G1, R - 7)]
    qs = [PM.G2, PM.g2_mul(PM.G2, 3), PM.g2_mul(PM.G2, 11)]
    want = PM.F12_ONE
    for p, q in zip(ps, qs):
        want = PM.f12_mul(want, miller_g if (p, q) == (M.G1, PM.G2) else PM.miller_loop(p, q))
    got = FM.miller_product(ps, [FM.prepare_g2(q) for q in qs])
    assert got == want
    # 1 * 1 + 5 * 3 - 7 * 11 = -61: that product is not one; 1 * 1 + 5 * 3 - 16 * 1 = 0: this one is
    ps2 = [M.G1, M.g1_mul(M.G1, 5), M.g1_mul(M.G1, R - 16)]
    qs2 = [PM.G2, PM.g2_mul(PM.G2, 3), PM.G2]
    assert FM.final_exp(FM.miller_product(ps2, [FM.prepare_g2(q) for q in qs2])) == PM.F12_ONE
    assert FM.final_exp(got) != PM.F12_ONE


def test_memory_form_round_trip():
    f = rand_f12(6)
    assert FM.f12_from_words(FM.f12_to_words(f)) == f
    assert len(FM.frobenius_table_words()) == 15
