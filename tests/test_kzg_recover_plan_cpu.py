"""The cell-recovery plan without a GPU: csrc/kzg_recover_plan.hpp, built with g++ and the address and undefined-behaviour
sanitizers as a program of its own (tests/host/kzg_recover_plan.cpp), against its invariants and, over F_65537, as the whole pipeline
walked step by step; and the new entries of the library without a device."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="session")
def recover_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kzg_recover_plan") / "kzg_recover_plan")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "zkp-implementation_amd", "csrc"), os.path.join(ROOT, "tests", "host", "kzg_recover_plan.cpp"),
                    "-o", exe], check=True)
    return exe


def test_recover_plan_invariants_and_pipeline_under_sanitizers(recover_plan_exe):
    r = subprocess.run([recover_plan_exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "kzg recover plan: 1624 pipelines, 0 failures" in r.stdout


@pytest.fixture(scope="module")
def zkp():
    import importlib.util
    spec = importlib.util.spec_from_file_location("zkp_build", os.path.join(ROOT, "zkp-implementation_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    import zkp_hip
    return zkp_hip


def test_new_symbols_are_exported(zkp):
    for name in ("zkp_kzg_recoverer_create", "zkp_kzg_recoverer_destroy", "zkp_kzg_recover_cosets", "zkp_kzg_recover_cosets_dev"):
        assert hasattr(zkp.lib(), name) and name in zkp.exported_symbols()
    assert zkp.lib().zkp_abi_version() == 1
    assert hasattr(zkp, "KzgRecoverer") and hasattr(zkp.KzgScheme, "recover_cosets")


def test_recoverer_needs_a_device(zkp):
    """Arguments are checked first; without a gfx950 device the creation fails loudly (there is no host path)."""
    import torch
    handle = zkp.C.c_void_p()
    for log_n, log_l in ((3, 3), (3, 4), (24, 6), (0, 0), (24, 0)):
        assert zkp.lib().zkp_kzg_recoverer_create(log_n, log_l, zkp.C.byref(handle)) == zkp.ZKP_E_ARG, (log_n, log_l)
        assert not handle.value
    assert zkp.lib().zkp_kzg_recoverer_create(4, 2, None) == zkp.ZKP_E_ARG
    zkp.lib().zkp_kzg_recoverer_destroy(None)
    if torch.cuda.is_available():
        return
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.KzgRecoverer(4, 2)
    assert ei.value.code == zkp.ZKP_E_DEVICE
