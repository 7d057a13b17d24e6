"""The transform over G1 points without a GPU: the model of the all-openings construction (tests/model/g1_ntt_model.py, integers mod
r in the exponent) against the definitions, and csrc/g1_ntt_plan.hpp -- built with g++ and the address and undefined-behaviour
sanitizers as a program of its own (tests/host/g1_ntt_plan.cpp) -- against its invariants and against the model's tables."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "model"))
import g1_ntt_model as m  # noqa: E402

R = m.R
SIZES = [2, 4, 8, 16, 32]  # every power of two in 2..32


def _poly_eval(f, x):
    acc = 0
    for c in reversed(f):
        acc = (acc * x + c) % R
    return acc


@pytest.mark.parametrize("n", [1, 2, 4, 8, 64, 128])
def test_staged_transform_is_the_definition(n):
    rng = random.Random(n)
    v = [rng.randrange(R) for _ in range(n)]
    v[0] = 0  # an identity among the points
    for inverse in (False, True):
        assert m.transform(v, inverse) == m.transform_by_definition(v, inverse)
    assert m.transform(m.transform(v), inverse=True) == v


@pytest.mark.parametrize("n", SIZES)
def test_open_all_gives_every_quotient_commitment(n):
    rng = random.Random(100 + n)
    s = rng.randrange(2, R)
    srs = [pow(s, k, R) for k in range(n)]
    log_n = n.bit_length() - 1
    w = m.root(log_n)
    lag = m.lagrange(srs, n)
    for length in range(1, n + 1):
        f = [rng.randrange(R) for _ in range(length)]
        if length > 1 and length % 3 == 0:
            f[-1] = 0  # a zero top coefficient is used as given
        proofs, evals = m.open_all(srs[:n - 1], f, n)
        fs = _poly_eval(f, s)
        for k in range(n):
            z = pow(w, k, R)
            assert evals[k] == _poly_eval(f, z)
            assert proofs[k] == (fs - evals[k]) * pow(s - z, R - 2, R) % R, (n, length, k)
        assert sum(a * b for a, b in zip(lag, evals)) % R == fs, (n, length)


def test_open_all_special_polynomials():
    n, s = 8, 0x1234567
    srs = [pow(s, k, R) for k in range(n - 1)]
    assert m.open_all(srs, [5], n)[0] == [0] * n                 # constant: every proof is the identity
    assert m.open_all(srs, [0] * n, n)[0] == [0] * n             # zero vector
    assert m.open_all(srs, [0, 1], n)[0] == [1] * n              # f = X: every quotient is 1, every proof S_0


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("g1_ntt_plan") / "g1_ntt_plan")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "zkp-implementation_amd", "csrc"), os.path.join(ROOT, "tests", "host", "g1_ntt_plan.cpp"),
                    "-o", exe], check=True)
    return exe


def test_plan_header_invariants_under_sanitizers(plan_exe):
    r = subprocess.run([plan_exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "sizes 0..24, 0 failures" in r.stdout


@pytest.mark.parametrize("log_n", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_plan_header_tables_match_the_model(plan_exe, log_n):
    r = subprocess.run([plan_exe, "dump", str(log_n)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-4000:]
    n = 1 << log_n
    seen = {"b": 0, "r": 0, "s": 0, "h": 0, "g": 0}
    none = lambda x: -1 if x is None else x
    for line in r.stdout.split("\n"):
        if not line:
            continue
        kind, *v = line.split()
        v = [int(x) for x in v]
        seen[kind] += 1
        if kind == "b":
            assert tuple(v[2:]) == m.butterfly(log_n, v[0], v[1]), line
        elif kind == "r":
            assert v[1] == m.bitrev(v[0], log_n), line
        elif kind == "s":
            assert v[1] == none(m.srs_slot_source(n, v[0])), line
        elif kind == "h":
            assert v[1] == none(m.slice_source(n, v[0])), line
        else:
            assert v[2] == none(m.coeff_slot_source(n, v[0], v[1])), line
    opener = log_n >= 1  # (the smallest opener has n = 2)
    assert seen == {"b": log_n * n // 2, "r": n, "s": 2 * n * opener, "h": n * opener, "g": n * 2 * n * opener}
