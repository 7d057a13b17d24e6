"""Big-integer mirror of the evaluation-form opening (csrc/kzg_evals_plan.hpp, kzg_evals.hpp, kzg_evals_host.inc): f(z) and the
values of the quotient from the values of f alone, the branch for a point of the domain, and the plan's constants the GPU test picks
its shapes from.  Written independently of the header over canonical integers; tests/test_kzg_evals_model_cpu.py checks it against
the oracle's coefficient-form opening, tests/host/kzg_evals_plan.cpp runs the header's own step list lane by lane over a small
field."""
import os
import re

from g1_ntt_model import R, bitrev, root

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
NATURAL, BITREV = 0, 1


def inv(a):
    return pow(a, R - 2, R)


def exponent(order, log_n, i):
    return bitrev(i, log_n) if order == BITREV else i


def permute(row, order, log_n):
    """natural-order values -> the row as a handle of `order` takes it (position i: the value at w^exponent(i)); an involution"""
    return [row[exponent(order, log_n, i)] for i in range(len(row))]


def open_row(row, z, log_n, order=NATURAL):
    """row: the n values in `order`; -> (y = f(z), the n values of (f - y) / (X - z) in NATURAL order, m or None)"""
    n = 1 << log_n
    assert len(row) == n
    w = root(log_n)
    z %= R
    wp = [pow(w, exponent(order, log_n, i), R) for i in range(n)]
    hit = [i for i in range(n) if wp[i] == z]
    assert len(hit) <= 1
    q = [0] * n
    if not hit:
        d = [inv((wp[i] - z) % R) for i in range(n)]
        y = (1 - pow(z, n, R)) * inv(n) % R * sum(row[i] * wp[i] % R * d[i] for i in range(n)) % R
        for i in range(n):
            q[exponent(order, log_n, i)] = (row[i] - y) * d[i] % R
        return y, q, None
    at = hit[0]
    m = exponent(order, log_n, at)
    y = row[at] % R
    acc = 0
    for i in range(n):
        if i == at:
            continue
        e = exponent(order, log_n, i)
        q[e] = (row[i] - y) * inv((wp[i] - z) % R) % R
        acc = (acc + q[e] * wp[i]) % R
    q[m] = -inv(pow(w, m, R)) * acc % R
    return y, q, m


def plan_constants():
    """The constants of csrc/kzg_evals_plan.hpp the tests take their shapes from"""
    text = open(os.path.join(ROOT, "zkp-implementation_amd", "csrc", "kzg_evals_plan.hpp")).read()
    num = lambda name: int(re.search(r"constexpr \w+ %s = (\d+)" % name, text).group(1))
    groups = re.search(r"KZG_EVALS_MSM_GROUP = (\d+), KZG_EVALS_MSM_GROUP_SPLIT = (\d+)", text)
    return {"threads": num("KZG_EVALS_THREADS"), "chunk": num("KZG_EVALS_CHUNK"), "span_log": num("KZG_EVALS_SPAN_LOG"),
            "msm_group": int(groups.group(1)), "msm_group_split": int(groups.group(2)), "inverse": num("KZG_EVALS_INVERSE")}


def edge_log_ns():
    """One size below the number of elements a workgroup inverts together, that number, one above (two workgroups and two partial
    sums per row), and one with four partial sums per row, which the finishing workgroup's lanes 0 .. 3 take one each"""
    s = plan_constants()["span_log"]
    return [s - 1, s, s + 1, s + 2]
