"""The coset-opening plan without a GPU: the additions to csrc/g1_ntt_plan.hpp, built with g++ and the address and
undefined-behaviour sanitizers as a program of its own (tests/host/g1_coset_plan.cpp), against their invariants and, over F_65537
with scalars standing in for points, against the division recurrence for every coset."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def coset_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("g1_coset_plan") / "g1_coset_plan")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "zkp-implementation_amd", "csrc"), os.path.join(ROOT, "tests", "host", "g1_coset_plan.cpp"),
                    "-o", exe], check=True)
    return exe


def test_coset_plan_invariants_and_pipeline_under_sanitizers(coset_plan_exe):
    r = subprocess.run([coset_plan_exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "g1 coset plan: 55 shapes, 0 failures" in r.stdout
