"""The batch of the coset-opening plan without a GPU: what csrc/g1_ntt_plan.hpp adds for zkp_kzg_open_cosets_batch, built with g++ and
the address and undefined-behaviour sanitizers as a program of its own (tests/host/g1_coset_batch_plan.cpp).  Every lane, table
entry, partial sum, u and h slot of a batch stays inside its polynomial and its buffer -- on the table of a max_polys = 1 opener as
well, where the single path's launch cut would overrun it -- and, over F_65537 with scalars standing in for points, row p of a batch
is the single-polynomial pipeline of polynomial p."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def batch_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("g1_coset_batch_plan") / "g1_coset_batch_plan")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "zkp-implementation_amd", "csrc"), os.path.join(ROOT, "tests", "host", "g1_coset_batch_plan.cpp"),
                    "-o", exe], check=True)
    return exe


def test_batch_plan_invariants_and_pipeline_under_sanitizers(batch_plan_exe):
    r = subprocess.run([batch_plan_exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "g1 coset batch plan: 28 shapes, 448 cases, 0 failures" in r.stdout
