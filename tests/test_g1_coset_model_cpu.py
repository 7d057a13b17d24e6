"""The big-integer model of the coset openings (tests/model/g1_coset_model.py) without a GPU: its maps against the tables the plan
header prints (tests/host/g1_coset_plan.cpp, built with g++ and the sanitizers), its pipeline and its two closed forms against the
division recurrence.  Only test_plan_header_tables_match_the_model runs library code (the plan header); the pipeline and closed-form
tests validate the REFERENCE -- what tests/test_gpu_kzg_cosets.py expects of the GPU for n > 64 and what the verifier's identity
rests on -- and say nothing about the library by themselves."""
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "model"))
import g1_coset_model as cm  # noqa: E402

R = cm.R
SHAPES = [(4, 2, 16), (4, 0, 16), (3, 2, 8), (5, 3, 20), (4, 3, 16), (4, 1, 7), (3, 2, 3), (2, 1, 4), (1, 0, 2), (5, 2, 29)]


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("g1_coset_plan_model") / "g1_coset_plan")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "zkp-implementation_amd", "csrc"), os.path.join(ROOT, "tests", "host", "g1_coset_plan.cpp"),
                    "-o", exe], check=True)
    return exe


def _case(log_n, log_l, length, seed=0):
    rng = random.Random(1000 * log_n + 10 * log_l + length + seed)
    n, l = 1 << log_n, 1 << log_l
    s = rng.randrange(2, R)
    return n, l, s, [pow(s, k, R) for k in range(n)], [rng.randrange(R) for _ in range(length)]


@pytest.mark.parametrize("log_n,log_l,length", SHAPES)
def test_pipeline_gives_every_quotient_commitment(log_n, log_l, length):
    n, l, s, srs, f = _case(log_n, log_l, length)
    w = cm.root(log_n)
    want = [cm.evaluate(cm.quotient(f, n, l, k), s) for k in range(n // l)]
    for group_log in range(4):
        proofs, evals = cm.open_cosets(srs[:n - l], f, n, l, group_log)
        assert proofs == want, group_log
        assert evals == [cm.evaluate(f, pow(w, m, R)) for m in range(n)]
    if length <= l:
        assert want == [0] * (n // l)
    if log_l == 0:
        import g1_ntt_model as m1
        assert (proofs, evals) == m1.open_all(srs[:n - 1], f, n)


@pytest.mark.parametrize("log_n,log_l,length", SHAPES)
def test_closed_forms_against_the_recurrence(log_n, log_l, length):
    n, l, s, srs, f = _case(log_n, log_l, length, seed=7)
    r, w = n // l, cm.root(log_n)
    evals = [cm.evaluate(f, pow(w, m, R)) for m in range(n)]
    want = [cm.evaluate(cm.quotient(f, n, l, k), s) for k in range(r)]
    assert cm.proofs_closed_form(f, evals, s, n, l) == want
    fs = cm.evaluate(f, s)
    for k in range(r):
        interp = cm.interpolant(evals[k::r], n, l, k)
        for j in range(l):  # it is the interpolant ...
            assert cm.evaluate(interp, pow(w, k + j * r, R)) == evals[k + j * r]
        # ... and f(s) - I_k(s) = q_k(s) (s^l - x_k^l), what the verifier's pairings compare
        assert (fs - cm.evaluate(interp, s)) % R == want[k] * (pow(s, l, R) - pow(w, k * l, R)) % R


@pytest.mark.parametrize("log_n,log_l,group_log", [(1, 0, 0), (2, 1, 3), (3, 1, 0), (3, 2, 1), (4, 2, 2), (5, 0, 3), (5, 3, 0), (5, 3, 3),
                                                    (6, 5, 2), (6, 2, 1)])
def test_plan_header_tables_match_the_model(plan_exe, log_n, log_l, group_log):
    p = subprocess.run([plan_exe, "dump", str(log_n), str(log_l), str(group_log)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-4000:]
    n, l = 1 << log_n, 1 << log_l
    r = n // l
    none = lambda x: -1 if x is None else x
    seen = dict.fromkeys("sghmefz", 0)
    for line in p.stdout.split("\n"):
        if not line:
            continue
        kind, *v = line.split()
        v = [int(x) for x in v]
        seen[kind] += 1
        if kind == "s":
            assert v[2] == none(cm.srs_slot_source(n, l, v[0], v[1])), line
        elif kind == "g":
            assert v[3] == none(cm.coeff_slot_source(n, l, v[0], v[1], v[2])), line
        elif kind == "h":
            assert v[1] == none(cm.slice_source(n, l, v[0])), line
        elif kind == "m":
            assert tuple(v) == cm.mac(n, l, group_log), line
        elif kind == "e":
            assert v[2] == cm.mac_element(n, l, group_log, v[0], v[1]), line
        elif kind == "f":
            assert (v[1], v[2], bool(v[3])) == cm.fold_steps(n, l, group_log)[v[0]], line
        else:
            assert tuple(v) == cm.sizes(n, l, group_log), line
    lens = len({x for x in (1, l, l + 1, n - 1, n) if 1 <= x <= n})
    assert seen == {"s": 2 * n, "g": lens * 2 * n, "h": r, "m": 1, "e": 2 * n, "f": len(cm.fold_steps(n, l, group_log)), "z": 1}
