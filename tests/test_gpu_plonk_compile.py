"""GPU: Circuit::compile on the device (zkp_plonk_prover_create_from_gates) and witness rebinding (zkp_plonk_prover_set_witness)
against the big-int restatement of plonk/src/circuit.rs (tests/model/plonk_model.py::Circuit.compile) and against the prover
zkp_plonk_prover_create makes from the same coefficient vectors.  Every comparison is bit-exact."""
import ctypes as C

import numpy as np
import pytest

import bigmodel as M
import plonk_model as PM
from test_plonk_compile_cpu import Both, random_circuit, rebuild
from test_plonk_model import challenges

pytestmark = pytest.mark.gpu
R = M.R
SMALL = {"ref": PM.reference_test_circuit, "ref02": PM.reference_test_circuit_02, "ref03": PM.reference_test_circuit_03,
         "pi": PM.public_input_circuit}
COMMITS = ("a", "b", "c", "z", "t_lo", "t_mid", "t_hi", "w_ev_x", "w_ev_wx")


@pytest.fixture(scope="module")
def zkp():
    import torch
    assert torch.cuda.is_available()
    import zkp_hip
    zkp_hip.init()
    return zkp_hip


def make_srs(zkp, orc, secret, n):
    return zkp.Srs.new_from_secret(orc.fr_from_ints([secret])[0], n)   # n + 3 points (srs.rs:51)


def coefficient_prover(zkp, orc, cc, srs):
    """The prover the parent's route makes: zkp_plonk_prover_create from the model's twelve coefficient vectors."""
    polys = {k: orc.fr_from_ints(cc[k]) if len(cc[k]) else np.zeros((0, 4), dtype=np.uint64) for k in zkp.CIRCUIT_POLYS}
    return zkp.PlonkProver(srs.bases, cc["n"].bit_length() - 1, polys, orc.fr_from_ints([cc["k1"]])[0], orc.fr_from_ints([cc["k2"]])[0])


def same_proof(p, q):
    return (all(p["commits"][k][1] == q["commits"][k][1] and np.array_equal(p["commits"][k][0], q["commits"][k][0]) for k in COMMITS)
            and np.array_equal(p["bars"], q["bars"]) and np.array_equal(p["u"], q["u"]) and p["degree"] == q["degree"])


def g2s_of(secret):
    import pairing_model as PairM
    from test_pairing_cpu import g2_from_ints
    return g2_from_ints(PairM.g2_mul(PairM.G2, secret))


# ------------------------------------------------------------------------------------------------ 1. coefficient vectors
@pytest.mark.parametrize("case", ["ref", "ref02", "ref03", "pi", "random1000"])
def test_circuit_polynomials_match_the_model_compile(zkp, orc, case):
    """All twelve polynomials, zero-padded to n, limb for limb.  random1000: wires drawn uniformly from the 3 x n positions (no true
    permutation: neither the reference nor the model asks for one), g = 1000 so n = 1024 with 24 dummy rows."""
    both = random_circuit(zkp, 0xC0117, 1000) if case == "random1000" else rebuild(zkp, SMALL[case])
    cc = both.model.compile()
    n = cc["n"]
    if case == "random1000":
        assert n == 1024 and len(both.model.gates) == 1000
    srs = make_srs(zkp, orc, 0x5EC + n, n)
    pr = both.mirror.compile(srs.bases)
    assert pr.n == n
    for name in zkp.CIRCUIT_POLYS:
        exp = cc[name] + [0] * (n - len(cc[name]))
        assert orc.fr_to_ints(pr.circuit_poly(name)) == exp, name
    log_n, k1, k2 = pr.info()
    assert log_n == n.bit_length() - 1
    assert orc.fr_to_ints(np.stack([k1, k2])) == [2, 3] == [cc["k1"], cc["k2"]]
    pr.close()


# ------------------------------------------------------------------------------------------------ 2. proof equality
@pytest.mark.parametrize("case", ["ref", "ref02", "ref03", "pi"])
def test_proof_equals_the_coefficient_route_and_verifies(zkp, orc, case):
    both = rebuild(zkp, SMALL[case])
    cc = both.model.compile()
    blinders, _ = challenges(7)
    secret = M.rand_fr_list(407, 1)[0]
    srs = make_srs(zkp, orc, secret, cc["n"])
    bl = orc.fr_from_ints(blinders)
    old = coefficient_prover(zkp, orc, cc, srs)
    new = both.mirror.compile(srs.bases)
    p_old, p_new = old.prove(bl), new.prove(bl)
    assert same_proof(p_old, p_new)
    assert new.verify(g2s_of(secret), p_new) == 1     # real pairings (plonk/src/verifier.rs:19-157)
    assert old.verify(g2s_of(secret), p_new) == 1
    assert same_proof(new.prove(bl), p_new)           # and again from the same handle
    old.close()
    new.close()


# ------------------------------------------------------------------------------------------------ 3. 2^16
def synthetic_circuit(zkp, log_n, seed):
    """The chain of tests/test_gpu_plonk.py::synthetic_circuit (mul / add / mul / constant, the output of gate i wired to the left
    input of gate i+1, right inputs free, non-zero public inputs on all three kinds), once as the twelve evaluation columns that
    test builds by hand and once as gates."""
    n = 1 << log_n
    rb = M.rand_fr_list(seed, n)
    a_v, b_v, c_v = [0] * n, rb, [0] * n
    q_m, q_l, q_r, q_o, q_c, pi_v = ([0] * n for _ in range(6))
    circ = zkp.PlonkCircuit()
    a = 5
    for i in range(n):
        kind = i % 4
        pi = 7 * i + 1 if i % 8 in (0, 1, 3) else 0
        a_v[i] = a
        a_pos = (2, i - 1) if i else (0, 0)             # a_i <- c_{i-1}
        c_pos = (0, i + 1) if i < n - 1 else (2, i)     # c_i <- a_{i+1}
        if kind == 3:      # constant gate: a - constant - pi = 0
            q_l[i], q_c[i], c_v[i] = 1, (pi - a) % R, a
            add, kw = circ.add_constant_gate, {"constant": (a - pi) % R}
        elif kind == 1:    # addition gate: a + b - c - pi = 0
            q_l[i], q_r[i], q_o[i], c_v[i] = 1, 1, R - 1, (a + rb[i] - pi) % R
            add, kw = circ.add_addition_gate, {}
        else:              # multiplication gate: ab - c - pi = 0
            q_m[i], q_o[i], c_v[i] = 1, R - 1, (a * rb[i] - pi) % R
            add, kw = circ.add_multiplication_gate, {}
        add(a_pos + (a,), (1, i, rb[i]), c_pos + (c_v[i],), pi=pi, **kw)
        pi_v[i] = (-pi) % R
        a = c_v[i]
    w = M.root_of_unity(log_n)
    roots = [1] * n
    for i in range(1, n):
        roots[i] = roots[i - 1] * w % R
    k1, k2 = 2, 3
    s1 = [(roots[i - 1] * k2) % R if i else roots[0] for i in range(n)]
    s2 = [roots[i] * k1 % R for i in range(n)]
    s3 = [roots[i + 1] if i < n - 1 else roots[i] * k2 % R for i in range(n)]
    cols = {"f_a": a_v, "f_b": b_v, "f_c": c_v, "q_m": q_m, "q_l": q_l, "q_r": q_r, "q_o": q_o, "q_c": q_c, "pi": pi_v,
            "s_sigma_1": s1, "s_sigma_2": s2, "s_sigma_3": s3}
    return cols, circ


@pytest.fixture(scope="module")
def full_size(zkp, orc):
    log_n = 16
    cols, circ = synthetic_circuit(zkp, log_n, 0xC16C)
    polys = {k: zkp.ntt_fr(orc.fr_from_ints(v), inverse=True) for k, v in cols.items()}   # the existing route
    return log_n, polys, circ.gate_table()


@pytest.mark.parametrize("expand", [0, -1])
def test_full_size_2_16_equals_the_existing_route(zkp, orc, full_size, expand):
    """expand = 0: the plain SRS; -1: the SRS expanded with the library's automatic width (the configuration bench.py times)."""
    log_n, polys, table = full_size
    n = 1 << log_n
    f = lambda v: orc.fr_from_ints([v])[0]
    srs = make_srs(zkp, orc, M.rand_fr_list(0x5EC, 1)[0], n)
    if expand:
        srs.bases.precompute(0)
    blinders, _ = challenges(0x16)
    bl = orc.fr_from_ints(blinders)
    new = zkp.PlonkProver.from_gates(srs.bases, *table)
    assert new.n == n
    for name in zkp.CIRCUIT_POLYS:
        assert np.array_equal(new.circuit_poly(name), polys[name]), name
    old = zkp.PlonkProver(srs.bases, log_n, polys, f(2), f(3))
    p_old, p_new = old.prove(bl), new.prove(bl)
    assert p_new["degree"] == n + 1
    assert same_proof(p_old, p_new)
    old.close()
    new.close()


# ------------------------------------------------------------------------------------------------ 4. rebinding
def pythagoras(zkp, x, y, z, wrong=0):
    """plonk/src/verifier.rs:232-258 for any triple x^2 + y^2 = z^2 (no public inputs); wrong: added to one value."""
    both = Both(zkp)
    both.add_multiplication_gate((1, 0, x), (0, 0, x), (0, 3, x * x))
    both.add_multiplication_gate((1, 1, y), (0, 1, y), (1, 3, y * y))
    both.add_multiplication_gate((1, 2, z), (0, 2, z), (2, 3, z * z))
    both.add_addition_gate((2, 0, x * x), (2, 1, y * y), (2, 2, z * z + wrong))
    return both


def statement(zkp, x, y, p0, y2, p1, wrong=0):
    """Three gates (n = 4, one dummy row) with public inputs that belong to the witness:
       g0 mul: x y - m - p0 = 0     g1 add: m + y2 - s - p1 = 0 (m copied from g0's output)     g2 constant: 9 - 9 = 0"""
    both = Both(zkp)
    m = (x * y - p0) % R
    both.add_multiplication_gate((0, 0, x), (1, 0, y), (0, 1, m), pi=p0)
    both.add_addition_gate((2, 0, m), (1, 1, y2), (2, 1, (m + y2 - p1 + wrong) % R), pi=p1)
    both.add_constant_gate((0, 2, 9), (1, 2, 0), (2, 2, 0))
    return both


REBIND = {"pythagoras": (pythagoras, (3, 4, 5), (5, 12, 13), False),
          "statement": (statement, (3, 4, 5, 10, 2), (6, 11, 17, 1234567, 40), True)}


def rounds123(zkp, orc, pr, blinders, ch):
    f = lambda v: orc.fr_from_ints([v])[0]
    pr.round1(orc.fr_from_ints(blinders[:6]))
    pr.round2(f(ch["beta"]), f(ch["gamma"]), orc.fr_from_ints(blinders[6:9]))
    pr.round3(f(ch["alpha"]))
    return {k: pr.get_poly(k) for k in ("ax", "z", "t")}


@pytest.mark.parametrize("case", ["pythagoras", "statement"])
def test_set_witness_equals_a_fresh_prover(zkp, orc, case):
    import torch
    make, wa, wb, with_pi = REBIND[case]
    A, B, bad = make(zkp, *wa), make(zkp, *wb), make(zkp, *wb, wrong=1)
    secret = M.rand_fr_list(0xB1D, 1)[0]
    srs = make_srs(zkp, orc, secret, 4)
    g2s = g2s_of(secret)
    blinders, ch = challenges(11)
    bl = orc.fr_from_ints(blinders)
    (pos_a, sel_a, vals_a), (pos_b, sel_b, vals_b) = A.mirror.gate_table(), B.mirror.gate_table()
    assert np.array_equal(pos_a, pos_b) and np.array_equal(sel_a[:, :5], sel_b[:, :5])   # one circuit, two witnesses
    assert with_pi == (not np.array_equal(sel_a[:, 5], sel_b[:, 5]))
    pi_of = lambda sel: np.ascontiguousarray(sel[:, 5]) if with_pi else None
    g = len(pos_a)

    pr = A.mirror.compile(srs.bases)
    proof_a = pr.prove(bl)
    assert pr.verify(g2s, proof_a) == 1
    fresh_b = B.mirror.compile(srs.bases)
    proof_b = fresh_b.prove(bl)
    assert not same_proof(proof_a, proof_b)

    pr.set_witness(vals_b, pi_of(sel_b))
    assert same_proof(pr.prove(bl), proof_b)
    assert fresh_b.verify(g2s, proof_b) == 1 and pr.verify(g2s, proof_b) == 1
    for name in ("f_a", "f_b", "f_c", "pi"):
        assert np.array_equal(pr.circuit_poly(name), fresh_b.circuit_poly(name)), name
    got, exp = rounds123(zkp, orc, pr, blinders, ch), rounds123(zkp, orc, fresh_b, blinders, ch)
    for name in ("ax", "z", "t"):
        assert got[name].shape[0] and np.array_equal(got[name], exp[name]), name
    exp_model = PM.prove(B.model.compile(), secret, blinders, ch)["polys"]
    for name in ("ax", "z", "t"):
        assert M.poly_trim(orc.fr_to_ints(got[name])) == exp_model[name], name

    pr.set_witness(vals_a, pi_of(sel_a))
    assert same_proof(pr.prove(bl), proof_a)

    # one wrong value: reported where an unsatisfied circuit is reported today, and the handle recovers
    pr.set_witness(bad.mirror.gate_table()[2], pi_of(sel_b))
    with pytest.raises(zkp.ZkpError) as ei:
        pr.prove(bl)
    assert ei.value.code == zkp.ZKP_E_ARG and "No remainder expected" in str(ei.value) and "gate row" in str(ei.value), str(ei.value)
    pr.set_witness(vals_a, pi_of(sel_a))
    again = pr.prove(bl)
    assert same_proof(again, proof_a) and pr.verify(g2s, again) == 1

    # device form: tensors produced and read on a stream of the caller's
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        t_vals = torch.from_numpy(vals_b.view(np.int64).reshape(-1)).to("cuda", non_blocking=False).clone()
        t_pi = torch.from_numpy(pi_of(sel_b).view(np.int64).reshape(-1)).to("cuda").clone() if with_pi else None
        pr.set_witness_dev(t_vals, g, pi=t_pi, stream=stream.cuda_stream)
    assert same_proof(pr.prove(bl), proof_b)
    stream.synchronize()
    pr.close()
    fresh_b.close()


# ------------------------------------------------------------------------------------------------ 5. errors
def test_errors_name_their_cause_and_leave_the_srs_usable(zkp, orc):
    both = rebuild(zkp, PM.reference_test_circuit_02)      # 7 gates, n = 8
    pos, sel, vals = both.mirror.gate_table()
    g, n = 7, 8
    secret = M.rand_fr_list(0xE44, 1)[0]
    srs = make_srs(zkp, orc, secret, n)
    blinders, _ = challenges(3)
    bl = orc.fr_from_ints(blinders)

    def good():
        pr = zkp.PlonkProver.from_gates(srs.bases, pos, sel, vals)
        proof = pr.prove(bl)
        assert pr.verify(g2s_of(secret), proof) == 1
        return pr, proof

    def fails(code, *words):
        def check(fn):
            with pytest.raises(zkp.ZkpError) as ei:
                fn()
            assert ei.value.code == code, str(ei.value)
            for w in words:
                assert w in str(ei.value), str(ei.value)
            pr, proof = good()
            pr.close()
        return check

    ref, ref_proof = good()
    for cnt in (0, 1):
        fails(zkp.ZKP_E_ARG, "at least 2 gates")(lambda: zkp.PlonkProver.from_gates(srs.bases, pos[:cnt], sel[:cnt], vals[:cnt]))
    bad = pos.copy()
    bad[4, 2] = 3                                           # b wire of gate 4: column 3
    fails(zkp.ZKP_E_ARG, "Invalid position", "gate 4", "Pos(3,")(lambda: zkp.PlonkProver.from_gates(srs.bases, bad, sel, vals))
    bad = pos.copy()
    bad[6, 5] = n                                           # c wire of gate 6: row n
    fails(zkp.ZKP_E_ARG, "Invalid position", "gate 6", ", 8)")(lambda: zkp.PlonkProver.from_gates(srs.bases, bad, sel, vals))

    def too_many():                                         # log_n = 25 by the count alone: rejected before any array is read
        gt = zkp._PlonkGates((1 << 24) + 1, pos.ctypes.data, sel.ctypes.data, vals.ctypes.data)
        out = C.c_void_p()
        zkp._chk(zkp.lib().zkp_plonk_prover_create_from_gates(srs.bases._h, C.byref(gt), C.byref(out)))
    fails(zkp.ZKP_E_ARG, "log_n > 24")(too_many)

    short = make_srs(zkp, orc, secret, 4)                   # 7 points, the circuit needs 11
    with pytest.raises(zkp.ZkpError) as ei:
        zkp.PlonkProver.from_gates(short.bases, pos, sel, vals)
    assert ei.value.code == zkp.ZKP_E_SIZE and "circuit_size + 3" in str(ei.value)
    four = rebuild(zkp, PM.reference_test_circuit).mirror.compile(short.bases)   # n = 4 fits it
    assert four.verify(g2s_of(secret), four.prove(bl)) == 1
    four.close()

    fails(zkp.ZKP_E_ARG, "gate count 6", "7 gates")(lambda: ref.set_witness(vals[:6]))
    assert same_proof(ref.prove(bl), ref_proof)            # the refused call changed nothing
    old = coefficient_prover(zkp, orc, both.model.compile(), srs)
    fails(zkp.ZKP_E_ARG, "zkp_plonk_prover_create", "no gate table")(lambda: old.set_witness(vals))
    assert same_proof(old.prove(bl), ref_proof)
    old.close()
    ref.close()
