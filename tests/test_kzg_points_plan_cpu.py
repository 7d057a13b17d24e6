"""The plan of the batched point-opening verification without a GPU: csrc/kzg_points_plan.hpp, built with g++ and the address and
undefined-behaviour sanitizers as a program of its own (tests/host/kzg_points_plan.cpp), against its invariants and, over F_65537, as
the whole field pipeline walked lane by lane; and the new entries of the library without a device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkp-implementation_amd", "csrc")


@pytest.fixture(scope="session")
def points_plan_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kzg_points_plan") / "kzg_points_plan")
    subprocess.run(["g++", "-std=c++17", "-O2", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, os.path.join(ROOT, "tests", "host", "kzg_points_plan.cpp"), "-o", exe], check=True)
    return exe


def test_points_plan_invariants_and_pipeline_under_sanitizers(points_plan_exe):
    r = subprocess.run([points_plan_exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    # 3 chunk logs x (2 passes x 9 sizes x 4 groupings + 2 empty batches)
    assert "kzg points plan: 222 pipelines, 0 failures" in r.stdout


@pytest.fixture(scope="module")
def zkp():
    import importlib.util
    spec = importlib.util.spec_from_file_location("zkp_build", os.path.join(ROOT, "zkp-implementation_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    import zkp_hip
    return zkp_hip


NAMES = ("zkp_kzg_point_verifier_create", "zkp_kzg_point_verifier_destroy", "zkp_kzg_verify_points", "zkp_kzg_verify_points_dev",
         "zkp_kzg_verify_points_find_bad", "zkp_kzg_verify_points_find_bad_dev", "zkp_kzg_points_aggregate_dev",
         "zkp_kzg_verify_evals_batch_dev")


def test_new_symbols_are_exported(zkp):
    for name in NAMES:
        assert hasattr(zkp.lib(), name) and name in zkp.exported_symbols()
    assert zkp.lib().zkp_abi_version() == 1
    import zkp_hip.kzg_points as kp
    assert hasattr(zkp.KzgScheme, "verify_points") and issubclass(kp.KzgPointVerifier, zkp._Handle)
    for method in ("verify", "verify_dev", "verify_bytes", "aggregate_dev", "verify_evals_dev", "find_bad", "find_bad_dev", "close"):
        assert hasattr(kp.KzgPointVerifier, method)
    assert kp.KzgPointVerifier._destroy == "zkp_kzg_point_verifier_destroy" and "close" not in vars(kp.KzgPointVerifier)
    assert kp.NO_BAD_OPENING == (1 << 64) - 1


def test_the_knob_table_did_not_grow():
    """The verifier reads the cell verifier's chunk knob and adds none: the table has the entries the header documents, one for one."""
    text = open(os.path.join(CSRC, "knobs.hpp")).read()
    names = set(re.findall(r'"(ZKP_[A-Z0-9_]+)"', text))
    assert "ZKP_KZG_CELLS_CHUNK_LOG" in names and not any("POINTS" in n for n in names)
    for name in ("kzg_points_plan.hpp", "kzg_points.hpp", "kzg_points_host.inc"):
        src = open(os.path.join(CSRC, name)).read()
        assert "getenv" not in src
        knobs = set(re.findall(r"\bKNOB_[A-Z0-9_]+", src))
        assert knobs <= {"KNOB_KZG_CELLS_CHUNK_LOG", "KNOB_COUNT"}, knobs


def test_null_arguments_are_refused_before_the_device_is_looked_for(zkp):
    """What can be reached without a device is refused as an argument error and nothing is created; the entries that take a verifier
    refuse a null one and leave their outputs alone.  With valid arguments and no device, creation is ZKP_E_DEVICE: no host path."""
    import numpy as np
    import torch
    g2 = zkp.g2_generator()
    handle = zkp.C.c_void_p()
    create = zkp.lib().zkp_kzg_point_verifier_create
    assert create(None, 8, 2, zkp.C.byref(handle)) == zkp.ZKP_E_ARG and not handle.value
    assert create(g2.ctypes.data, 8, 2, None) == zkp.ZKP_E_ARG
    for max_openings, max_commits in ((0, 1), (1, 0), ((1 << 30) + 1, 1), (1, (1 << 30) + 1)):
        assert create(g2.ctypes.data, max_openings, max_commits, zkp.C.byref(handle)) == zkp.ZKP_E_ARG and not handle.value
    off = g2.copy()
    off[0] ^= 1
    assert create(off.ctypes.data, 8, 2, zkp.C.byref(handle)) == zkp.ZKP_E_ARG and not handle.value
    assert "[s]_2" in zkp.lib().zkp_last_error().decode()
    zkp.lib().zkp_kzg_point_verifier_destroy(None)
    acc, bad = zkp.C.c_int(7), zkp.C.c_size_t(9)
    lib = zkp.lib()
    assert lib.zkp_kzg_verify_points(None, None, None, 0, 0, None, None, None, None, None, None, zkp.C.byref(acc)) == zkp.ZKP_E_ARG
    assert lib.zkp_kzg_verify_points_dev(None, None, None, 0, 0, None, None, None, None, None, None, None, zkp.C.byref(acc)) == zkp.ZKP_E_ARG
    assert lib.zkp_kzg_verify_points_find_bad(None, None, None, 0, 0, None, None, None, None, None, None, zkp.C.byref(acc),
                                              zkp.C.byref(bad)) == zkp.ZKP_E_ARG
    assert lib.zkp_kzg_verify_points_find_bad_dev(None, None, None, 0, 0, None, None, None, None, None, None, None, zkp.C.byref(acc),
                                                  zkp.C.byref(bad)) == zkp.ZKP_E_ARG
    assert lib.zkp_kzg_points_aggregate_dev(None, 0, 0, None, None, None, None, None, None, None, None, None) == zkp.ZKP_E_ARG
    assert lib.zkp_kzg_verify_evals_batch_dev(None, None, None, 0, None, None, None, None, None, None, None, zkp.C.byref(acc)) == zkp.ZKP_E_ARG
    assert acc.value == 7 and bad.value == 9
    if torch.cuda.is_available():
        return
    with pytest.raises(zkp.ZkpError) as ei:
        import zkp_hip.kzg_points as kp
        kp.KzgPointVerifier(g2, 8, 2)
    assert ei.value.code == zkp.ZKP_E_DEVICE
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.G1Bases.from_host(np.zeros((8, 12), dtype=np.uint64))
    assert ei.value.code == zkp.ZKP_E_DEVICE
