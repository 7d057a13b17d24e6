"""plane_div (csrc/msm_plan.hpp): the multiply-high by a reciprocal with which msm_accumulate_run finds the plane of an entry of the
expanded bases, against the plain division it replaced -- plane boundaries of up to 35 planes, the ends of the range and a million
random entries for each of ten scalar counts.  CPU only: compiles tests/host/locate_div.cpp with g++ alone."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reciprocal_division_equals_division(tmp_path):
    exe = str(tmp_path / "locate_div")
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Werror", "-I", os.path.join(ROOT, "zkp-implementation_amd", "csrc"),
                    os.path.join(ROOT, "tests", "host", "locate_div.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:]
    m = re.search(r"locate_div: (\d+) checks, 0 failures", r.stdout)
    assert m and int(m.group(1)) > 10 * 1000000, r.stdout[-2000:]
