"""The MSM plan (csrc/msm_plan.hpp: ranges, geometry, workspace sizes) against the plans the driver made before plan_msm was split
out of it, plus the invariants the driver relies on.  CPU only: compiles tests/host/msm_plan_table.cpp with g++ alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_msm_plans_match_recorded_table(tmp_path):
    exe = str(tmp_path / "msm_plan_table")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zkp-implementation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "msm_plan_table.cpp"), "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith(("ZKP_MSM_", "ZKP_SORT_"))}
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "msm_plans.txt")], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "710 cases, 0 failures" in r.stdout
