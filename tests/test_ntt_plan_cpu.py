"""The NTT plan (csrc/ntt_plan.hpp: passes, radices, launch geometry, tables, the axis-0 split) against the shapes the driver computed
before the plan was split out of it, plus the invariants the driver relies on.  CPU only: compiles tests/host/ntt_plan_table.cpp with
g++ alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ntt_plans_match_recorded_table(tmp_path):
    exe = str(tmp_path / "ntt_plan_table")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zkp-implementation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "ntt_plan_table.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "ntt_plans.txt")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "1106 cases, 0 failures" in r.stdout
