"""The MSM plan (csrc/msm_plan.hpp) on the host: ranges, geometry and workspace sizes against the plans the driver made before
plan_msm was split out of it; the shape of every launch (range geometry, accumulate, fold steps, bucket reduction, partscatter tile)
against the shapes the driver chose before they moved into the plan; the invariants the driver relies on, on every plan of both
tables; and the bucket reduction replayed over integers.  CPU only: compiles tests/host/msm_plan_table.cpp with g++ alone."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def run_table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("msm_plan") / "msm_plan_table")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zkp-implementation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "msm_plan_table.cpp"), "-o", exe], check=True)
    # (the program clears every knob the plan reads before each case)
    env = {k: v for k, v in os.environ.items() if not k.startswith(("ZKP_MSM_", "ZKP_SORT_", "ZKP_PYR_", "ZKP_FOLD_"))}

    def run(*args):
        r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=120, env=env)
        assert r.returncode == 0, r.stdout[-4000:]
        return r.stdout
    return run


def test_msm_plans_match_recorded_table(run_table):
    assert "710 cases, 0 failures" in run_table("plans", os.path.join(ROOT, "tests", "golden", "msm_plans.txt"))


def test_msm_launches_match_recorded_table(run_table):
    """Every launch shape of the pass, for a device given by its resident-wave bound, as the driver chose it inline before."""
    table = os.path.join(ROOT, "tests", "golden", "msm_launches.txt")
    lines = [ln for ln in open(table) if ln.strip() and not ln.startswith("#")]
    assert f"msm launches: {len(lines)} cases, 0 failures" in run_table("launches", table) and len(lines) >= 150
    # 544 bucket sets of four waves are more than a full card keeps resident: every level its own launch, then the gathering
    collect = [ln for ln in lines if ln.startswith("n=64 bn=64 count=17 w=0 glv=0 feed=0 waves=2048 env=- ")]
    assert len(collect) == 1 and " tail=collect " in collect[0]
    for refused in ("ZKP_PYR_TAIL_THREADS=100", "ZKP_PYR_TAIL_BLOCKS=0"):
        assert any(f"env={refused} -> rc=-" in ln and "ZKP_PYR_TAIL_THREADS must be a multiple of 64" in ln for ln in lines)


def test_msm_reduction_replays_exactly_and_without_races(run_table):
    """plan_reduce's schedule with the kernels' addressing over wrap-around integers: c = 2 .. 9, 1 and 3 bucket sets, both endings."""
    out = run_table("replay")
    assert "0 failures" in out and "(0 with" not in out and " 0 collect only" not in out
