"""Host side of Circuit::compile on the GPU (no GPU needed): the PlonkCircuit mirror packs exactly the gates the big-int model
(tests/model/plonk_model.py::Circuit, a restatement of plonk/src/circuit.rs and gate.rs) holds, the five entries are declared
and exported, and without a device zkp_plonk_prover_create_from_gates fails loudly."""
import ctypes as C
import os
import random
import re

import numpy as np
import pytest

import bigmodel as M
import plonk_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R
ENTRIES = ("zkp_plonk_prover_create_from_gates", "zkp_plonk_prover_set_witness", "zkp_plonk_prover_set_witness_dev",
           "zkp_plonk_get_circuit_poly", "zkp_plonk_prover_info")


@pytest.fixture(scope="module")
def zkp():
    import importlib.util
    spec = importlib.util.spec_from_file_location("zkp_build", os.path.join(ROOT, "zkp-implementation_amd", "build.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    mod.build()
    import zkp_hip
    return zkp_hip


class Both:
    """The same calls on the model's Circuit and on the product's PlonkCircuit."""

    def __init__(self, zkp):
        self.model, self.mirror = PM.Circuit(), zkp.PlonkCircuit()

    def __getattr__(self, name):
        def call(*args, **kw):
            getattr(self.model, name)(*args, **kw)
            getattr(self.mirror, name)(*args, **kw)
        return call


def rebuild(zkp, make):
    """Replay a model circuit builder of plonk_model.py on both classes (the builders only use the three add_* calls)."""
    both = Both(zkp)
    real = PM.Circuit
    PM.Circuit = lambda: both
    try:
        assert make() is both
    finally:
        PM.Circuit = real
    return both


def random_circuit(zkp, seed, gates):
    rnd = random.Random(seed)
    both = Both(zkp)
    n = 1 << (gates - 1).bit_length()
    for _ in range(gates):
        a, b, c = ((rnd.randrange(3), rnd.randrange(n), rnd.randrange(R)) for _ in range(3))
        kind = rnd.randrange(4)
        pi = rnd.randrange(1, R)
        if kind == 0:
            both.add_addition_gate(a, b, c, pi=pi)
        elif kind == 1:
            both.add_multiplication_gate(a, b, c, pi=pi)
        elif kind == 2:
            both.add_constant_gate(a, b, c, pi=pi)
        else:
            both.add_constant_gate(a, b, c, pi=pi, constant=rnd.randrange(R))
    return both


def mont_limbs(v):
    return M.to_limbs(M.fr_to_mont(v), 4)


def check_table(both):
    model, (pos, sel, vals) = both.model, both.mirror.gate_table()
    g = len(model.gates)
    assert g >= 2 and len(both.mirror) == g
    assert pos.dtype == np.uint32 and pos.shape == (g, 6)
    assert sel.dtype == np.uint64 and sel.shape == (g, 6, 4)
    assert vals.dtype == np.uint64 and vals.shape == (g, 3, 4)
    for i, gate in enumerate(model.gates):
        (ac, ar), (bc, br), (cc, cr), q_l, q_r, q_o, q_m, q_c, pi = gate
        assert [int(x) for x in pos[i]] == [ac, ar, bc, br, cc, cr], i
        for k, v in enumerate((q_m, q_l, q_r, q_o, q_c, pi)):   # the order of zkp_plonk_gates.sel; pi as stored (negated)
            assert [int(x) for x in sel[i, k]] == mont_limbs(v), (i, k)
        for k in range(3):
            assert [int(x) for x in vals[i, k]] == mont_limbs(model.vals[k][i]), (i, k)


@pytest.mark.parametrize("name", ["reference_test_circuit", "reference_test_circuit_02", "reference_test_circuit_03",
                                  "public_input_circuit"])
def test_gate_table_matches_the_model_circuit(zkp, name):
    both = rebuild(zkp, getattr(PM, name))
    check_table(both)
    if name == "public_input_circuit":
        assert any(g[8] for g in both.model.gates) and any(g[7] for g in both.model.gates)


def test_gate_table_matches_the_model_on_a_random_circuit(zkp):
    both = random_circuit(zkp, 0xC0117, 1000)
    kinds = {g[3:8] for g in both.model.gates}
    assert len(kinds) > 3 and all(g[8] for g in both.model.gates)   # add, mul and many constant gates; pi everywhere
    check_table(both)


def test_header_declares_and_library_exports_the_entries(zkp):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zkp_hip.h")).read(), flags=re.S)
    lib = zkp.lib()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", src), name
        assert hasattr(lib, name) and name in zkp.exported_symbols(), name
    assert re.search(r"typedef struct \{[^}]*\bgates;[^}]*\bpos;[^}]*\bsel;[^}]*\bvals;[^}]*\}\s*zkp_plonk_gates;", src)
    assert lib.zkp_abi_version() == 1


def test_create_from_gates_needs_a_device(zkp):
    """Without a GPU there is no SRS handle either, so the entry is called directly: it must fail with ZKP_E_DEVICE before it reads
    the handle (no CPU fallback), and its argument checks come before that."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the entry runs (tests/test_gpu_plonk_compile.py)")
    both = rebuild(zkp, PM.reference_test_circuit)
    pos, sel, vals = both.mirror.gate_table()
    lib = zkp.lib()
    not_an_srs = C.create_string_buffer(64)
    out = C.c_void_p()

    def call(g):
        gt = zkp._PlonkGates(g, pos.ctypes.data, sel.ctypes.data, vals.ctypes.data)
        return lib.zkp_plonk_prover_create_from_gates(C.cast(not_an_srs, C.c_void_p), C.byref(gt), C.byref(out))

    assert call(len(pos)) == zkp.ZKP_E_DEVICE
    assert b"device" in lib.zkp_last_error() and not out.value
    for g in (0, 1):
        assert call(g) == zkp.ZKP_E_ARG and b"at least 2 gates" in lib.zkp_last_error()
    assert call((1 << 24) + 1) == zkp.ZKP_E_ARG and b"log_n > 24" in lib.zkp_last_error()   # decided from the count alone
    with pytest.raises(zkp.ZkpError):
        zkp.G1Bases.from_host(np.zeros((1, 12), dtype=np.uint64))   # (what PlonkCircuit.compile would need first)
