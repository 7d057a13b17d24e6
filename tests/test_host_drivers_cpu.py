"""Host-only pieces of the drivers: batch_to_affine (csrc/host_ff.hpp) byte for byte against HXyzz::to_affine, and the knob readers
(csrc/knobs.hpp) against the readers they replaced.  CPU only: compiles tests/host/knobs_and_affine.cpp with g++ alone."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkp-implementation_amd", "csrc")


def test_batch_to_affine_and_knob_readers(tmp_path):
    exe = str(tmp_path / "knobs_and_affine")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", CSRC, os.path.join(ROOT, "tests", "host", "knobs_and_affine.cpp"),
                    "-o", exe], check=True)
    env = {k: v for k, v in os.environ.items() if not k.startswith("ZKP_")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert "host drivers: 0 failures" in r.stdout


def test_getenv_only_in_the_knob_table():
    """Every environment read of the library goes through knobs.hpp."""
    hits = [name for name in sorted(os.listdir(CSRC)) if name != "knobs.hpp" and "getenv" in open(os.path.join(CSRC, name)).read()]
    assert hits == []
