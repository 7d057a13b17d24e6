"""Operands shared by the pairing tower tests (tests/test_pairing_tower_cpu.py on the host instantiation, tests/test_gpu_pairing_selftest.py
on the device's): Fq12 elements with 0, 1 and p - 1 in every coefficient slot, random ones, and the expected value of every tower
operation from the big-int model (tests/model/pairing_fast_model.py)."""
import random

import bigmodel as M
import pairing_fast_model as FM
import pairing_model as PM

P = M.P


def f12_from_coeffs(c):
    return (((c[0], c[1]), (c[2], c[3]), (c[4], c[5])), ((c[6], c[7]), (c[8], c[9]), (c[10], c[11])))


def edge_elements():
    """0, 1 and p - 1 in every slot: the three constant vectors and the three rotations of the pattern (0, 1, p - 1)"""
    vals = (0, 1, P - 1)
    out = [f12_from_coeffs([v] * 12) for v in vals]
    out += [f12_from_coeffs([vals[(i + rot) % 3] for i in range(12)]) for rot in range(3)]
    return out


def random_elements(seed, n):
    rng = random.Random(seed)
    return [f12_from_coeffs([rng.randrange(P) for _ in range(12)]) for _ in range(n)]


def as_line(b):
    """The line an Fq12 operand stands for in the sparse product: (A, B, C) = (c0.c0, c0.c1, c1.c1.c0)"""
    return b[0][0], b[0][1], b[1][1][0]


# operation name -> (number on the C ABI, takes a second operand, the model)
OPS = {
    "mul": (0, True, lambda a, b: PM.f12_mul(a, b)),
    "sqr": (1, False, lambda a, b: PM.f12_mul(a, a)),
    "line": (2, True, lambda a, b: FM.f12_mul_line(a, *as_line(b))),
    "inv": (3, False, lambda a, b: FM.f12_inv(a)),
    "frob1": (4, False, lambda a, b: FM.f12_frobenius(a, 1)),
    "frob2": (5, False, lambda a, b: FM.f12_frobenius(a, 2)),
    "frob3": (6, False, lambda a, b: FM.f12_frobenius(a, 3)),
    "cyc": (7, False, lambda a, b: FM.f12_cyclotomic_sqr(a)),
    "fexp": (8, False, lambda a, b: FM.final_exp(a)),
}
