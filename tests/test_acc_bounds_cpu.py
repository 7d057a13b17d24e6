"""The bounds g1_28_madd (csrc/g1_28.hpp) relies on where it hands R = S2 + (8p - S1) to the products without normalising it: the
constant KP8_28 of csrc/fq28.hpp re-derived from the big-int model, and the column sums of the squaring and of the two-product
reduction of Y3 with the largest limbs the operands can have (CPU only)."""
import bigmodel as M
from test_limb_constants import arrays, value

TIGHT = (1 << 28) - 1   # largest limb 0..12 of a product, of a stored X and of a stored Y


def test_kp8_28_is_8p_and_dominates_a_stored_y():
    c = arrays("fq28.hpp", "Fq28C")
    l = c["KP8_28"]
    assert len(l) == 14 and value(l, 28) == 8 * M.P
    assert all(TIGHT <= x < (1 << 29) for x in l[:13])      # no limb of 8p - Y negative, every limb of it below 2^29
    assert l[13] >= ((6 * M.P) >> 364) + 1                  # the top limb of a stored Y (value < 6p) with its carries


def test_columns_of_the_products_of_an_unnormalised_r():
    c = arrays("fq28.hpp", "Fq28C")
    ns1 = max(c["KP8_28"])                                  # 8p - S1
    r = TIGHT + ns1                                         # S2 tight
    t = TIGHT + max(c["KP16_29"])                           # Q - X3 = Q + 16p - X3, Q tight
    assert r < 3 << 28 and t <= 1 << 30 and ns1 < 1 << 29
    carry = 1 << 36                                         # what a column below 2^64 hands to the next
    reduction = 14 * TIGHT * TIGHT                          # m[i] * MOD[j]
    # fq28_mul2_chain(R, t, 8p - S1, PPP): 14 products of each pair in the longest column
    assert 14 * r * t + 14 * ns1 * TIGHT + reduction + carry < 1 << 64
    # fq28_sqr_chain(R): at most seven doubled products and one square per column
    assert 7 * (2 * r) * r + r * r + reduction + carry < 1 << 64
    # the values are those of sub8(S2, S1): R < 2p + 8p, R^2 and R t + (8p - S1) PPP inside 2520 p^2 (g1_28.hpp, xyzz_finish)
    assert 10 * 10 <= 2520 and 10 * 18 + 8 * 2 <= 2520
