"""The big-integer model of the cell recovery (tests/model/kzg_recover_model.py) against Lagrange interpolation through the present
points, for every shape with n <= 64 and every admissible number of missing cosets, and the consistency rule in both directions.
The GPU tests compare the device with the polynomial they started from; this file ties the construction (vanishing polynomial by a
padded product tree, masked multiply, division on a shifted domain) to the definition."""
import random

import pytest

import kzg_recover_model as km

R = km.R
SHAPES = [(log_n, log_l) for log_n in range(1, 7) for log_l in range(log_n)]


def evaluate(f, n):
    return km.ntt(list(f) + [0] * (n - len(f)))


def domain_points(log_n):
    w = km.root(log_n)
    return [pow(w, i, R) for i in range(1 << log_n)]


@pytest.mark.parametrize("log_n,log_l", SHAPES)
def test_recovery_is_the_interpolant_through_the_present_points(log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    rng = random.Random(0x7100 + 16 * log_n + log_l)
    pts = domain_points(log_n)
    for m in range(r):  # every admissible m: at least one coset stays
        cap = (r - m) * l
        missing = set(rng.sample(range(r), m))
        present = [0 if k in missing else 1 for k in range(r)]
        keep = [i for i in range(n) if present[i % r]]
        for length in sorted({1, cap, rng.randint(1, cap)}):
            f = [rng.randrange(R) for _ in range(length)]
            ev = evaluate(f, n)
            given = [ev[i] if present[i % r] else R - 1 for i in range(n)]  # what stands at a missing position is not read
            leaf_log = (1, 2, 5)[(m + length) % 3]
            got, ok = km.recover(given, present, length, log_n, log_l, leaf_log)
            assert got == f and ok, (m, length, leaf_log)
            if n <= 16 or m in (0, 1, r // 2, r - 1):
                full = km.lagrange([pts[i] for i in keep], [ev[i] for i in keep])
                assert full[:length] == f and not any(full[length:]), (m, length)


@pytest.mark.parametrize("log_n,log_l", [(3, 1), (4, 2), (5, 0), (6, 3)])
def test_consistency_rule_in_both_directions(log_n, log_l):
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    rng = random.Random(0x7200 + 16 * log_n + log_l)
    pts = domain_points(log_n)
    for m in (0, 1, r // 2):
        missing = set(rng.sample(range(r), m))
        present = [0 if k in missing else 1 for k in range(r)]
        keep = [i for i in range(n) if present[i % r]]
        cap = len(keep)
        for length in {cap, max(1, cap - l), 1}:
            f = [rng.randrange(R) for _ in range(length)]
            ev = evaluate(f, n)
            bad = list(ev)
            at = rng.choice(keep)
            bad[at] = (bad[at] + 1) % R
            got, ok = km.recover(bad, present, length, log_n, log_l, 2)
            full = km.lagrange([pts[i] for i in keep], [bad[i] for i in keep])
            assert got == full[:length]  # the low part of the interpolant through what was given, either way
            # exactly enough cells: every input is consistent; surplus cells: one altered value cannot be (the difference of the two
            # interpolants has cap - 1 roots among the present points and a degree below cap, so its degree is cap - 1 >= length)
            assert ok == (length == cap) == (not any(full[length:])), (m, length)
            assert km.recover(ev, present, length, log_n, log_l, 2) == (f, True)


def test_vanishing_polynomial_through_the_tree_is_the_plain_product():
    rng = random.Random(0x7300)
    log_n, log_l = 6, 0
    rho = km.root(log_n - log_l)
    for m in (1, 2, 3, 4, 5, 7, 8, 9, 21, 32, 33, 63):
        missing = sorted(rng.sample(range(64), m))
        plain = [1]
        for k in missing:
            plain = km.poly_mul_linear(plain, pow(rho, k, R))
        for leaf_log in (1, 2, 3, 5, 8):
            assert km.vanishing(log_n, log_l, leaf_log, missing) == plain, (m, leaf_log)
    # every other coset: Zs = Y^(r/2) - 1, sparse, with the carry into the top coefficient
    assert km.vanishing(6, 0, 2, list(range(0, 64, 2))) == [R - 1] + [0] * 31 + [1]
