"""CPU-only: the exact limb model (tests/model/limb_model.py) against independent ground truth, and the generated asm text of the product
forms executed by a small interpreter (tests/model/asm_interp.py) against the model, bit for bit, on the contract-edge vectors of
tests/field_vectors.py.  tests/test_gpu_field_selftest.py runs the same vectors through the device primitives themselves."""
import importlib.util
import os
import re

import pytest

import asm_interp as A
import bigmodel as M
import field_vectors as V
import limb_model as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkp-implementation_amd", "csrc")
P, R = M.P, M.R
RI392, RI261 = pow(1 << 392, -1, P), pow(1 << 261, -1, R)


def load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ------------------------------------------------------------------------------------------------ the model against ground truth
def test_products_are_the_montgomery_products():
    for a, b in V.fq28_mul_cases():
        r = L.fq28_mul(a, b)
        assert L.v28(r) % P == L.v28(a) * L.v28(b) * RI392 % P and L.is_tight28(r)
    for a in V.fq28_sqr_cases():
        assert L.v28(L.fq28_sqr(a)) % P == L.v28(a) ** 2 * RI392 % P
    for a, b, c, d in V.fq28_mul2_cases():
        r = L.fq28_mul2(a, b, c, d)
        assert L.v28(r) % P == (L.v28(a) * L.v28(b) + L.v28(c) * L.v28(d)) * RI392 % P and L.is_tight28(r)
    for a, b in V.fr29_mul_cases():
        r = L.fr29_mul(a, b)
        assert L.v29(r) % R == L.v29(a) * L.v29(b) * RI261 % R and L.v29(r) < 2 * R and max(r) < (1 << 29)


def test_linear_forms_keep_the_residue():
    for name, k in (("sub4", 4), ("sub8", 8), ("sub16", 16), ("sub8w", 8)):
        for a, b in V.fq28_sub_cases(name):
            assert L.v28(getattr(L, "fq28_" + name)(a, b)) == L.v28(a) + k * P - L.v28(b)
    for a in V.fq28_neg4_cases():
        assert L.v28(L.fq28_neg4(a)) == 4 * P - L.v28(a)
    for a in V.fq28_normalise_cases():
        n = L.fq28_normalise(a)
        assert L.v28(n) == L.v28(a) and max(n[:13]) < (1 << 28)
    for name, k in (("sub_tight", 4), ("sub_wide8", 8)):
        for a, b in V.fr29_sub_cases(name):
            assert L.v29(getattr(L, "fr29_" + name)(a, b)) == L.v29(a) + k * R - L.v29(b)
    for a in V.fr29_normalise_cases():
        n = L.fr29_normalise(a)
        assert L.v29(n) == L.v29(a) and max(n[:8]) < (1 << 29)
    for a in V.fr29_to_canonical_cases():
        assert L.value(L.fr29_to_canonical(a)[0], 32) == L.v29(a) % R
    for a, b in V.fr_mem_cases():
        assert L.value(L.fr_mul_mem(a, b), 32) == L.value(a, 32) * L.value(b, 32) * pow(1 << 256, -1, R) % R
    for w in V.fr_canonical_words():
        assert L.v29(L.fr29_twiddle_from_mont(w)) == L.value(w, 32) * 32 % R
    for w in V.words_cases(8, 1, [R, R - 1]):
        assert L.v29(L.fr29_from_sat_shl5(w)) == 32 * L.value(w, 32) and L.v29(L.fr29_from_sat(w)) == L.value(w, 32)
    for w in V.words_cases(12, 2, [P, P - 1]):
        assert L.v28(L.fq28_from_sat(w)) == L.value(w, 32)
    for c in V.fr29_pack_cases():
        assert L.value(L.fr29_pack_tight(c), 32) == L.v29(c)
    V.gl_reduce_pairs()                                   # the model asserts == x mod p and the two "no second wrap" claims itself
    for a, b in V.gl_pairs(any64=True):
        assert L.gl_op("mul", a, b) == a * b % L.GL


def test_the_model_refuses_what_is_out_of_contract():
    B = 1 << 30
    with pytest.raises(L.ContractError):
        L.fq28_mul(V.canon(51 * P), V.canon(50 * P))                     # 2550 p^2
    with pytest.raises(L.ContractError):
        L.fq28_mul([B] * 14, V.canon(0))                                  # a limb at 2^30
    with pytest.raises(L.ContractError):
        L.fq28_mul2([1 << 29] * 14, [1 << 29] * 14, V.canon(0), V.canon(0))   # limb product 2^58
    with pytest.raises(L.ContractError):
        L.fq28_sub8(V.canon(0), V.canon(14 * P))                          # top limb above KP8_29's
    k = list(L.FQ["KP16_29"])
    k[3] += 1
    with pytest.raises(L.ContractError):
        L.fq28_sub16(V.canon(0), k)
    with pytest.raises(L.ContractError):
        L.fr29_mul(V.c29(36 * R), V.c29(2 * R))
    with pytest.raises(L.ContractError):
        L.fr29_to_canonical([0] * 8 + [1 << 29])                          # 2^261
    with pytest.raises(L.ContractError):
        L.fq28_tight_is_zero_mod_p(V.canon(2 * P))
    with pytest.raises(L.ContractError):
        L.check_stored(L.x28_from_point(M.G1, 1, 14, 0))


def _check_point(res, expect):
    L.check_stored(res)
    assert L.affine_of(res) == expect


def a28_point(q):
    ri = RI392
    return (L.v28(q["x"]) * ri % P, L.v28(q["y"]) * ri % P)


def test_curve_formulas_are_the_group_law_and_keep_the_invariants():
    kinds = set()
    for kind, acc, q in V.g1_madd_cases():
        L.check_stored(acc)
        res = L.g1_28_madd(acc, q)
        _check_point(res, M.g1_add(L.affine_of(acc), a28_point(q)))
        kinds.add((kind, L.is_inf(res)))
    assert {("sum", False), ("acc infinite", False), ("double", False), ("cancel", True)} <= kinds
    oks = set()
    for kind, acc, q in V.g1_mmadd_cases():
        ok, res = L.g1_28_mmadd(acc, q)
        oks.add((kind, ok))
        if ok:
            _check_point(res, M.g1_add(L.affine_of(acc), a28_point(q)))
        else:
            assert res == acc and a28_point(q)[0] == L.affine_of(acc)[0]
    assert oks == {("sum", True), ("same x", False)}
    kinds = set()
    for kind, a, b in V.g1_add_cases():
        res = L.g1_28_add(a, b)
        _check_point(res, M.g1_add(L.affine_of(a), L.affine_of(b)))
        kinds.add((kind, L.is_inf(res)))
        for other in (L.g1_28_add(a, b, stream=True), L.g1_28_add_quad(a, b)):     # the same point; X3, ZZ3, ZZZ3 in the same limbs
            _check_point(other, L.affine_of(res))
            assert L.is_inf(res) or [other[c] for c in ("x", "zz", "zzz")] == [res[c] for c in ("x", "zz", "zzz")]
    assert {("sum", False), ("a infinite", False), ("b infinite", False), ("both infinite", True), ("double", False), ("cancel", True)} <= kinds
    for a in V.g1_double_cases():
        _check_point(L.g1_28_double(a), M.g1_add(L.affine_of(a), L.affine_of(a)))
    for q in V.g1_double_affine_cases():
        _check_point(L.g1_28_double_affine(q), M.g1_add(a28_point(q), a28_point(q)))
    # the point with x = 0 is a finite point whose X is the all-zero limb vector
    t = L.x28_from_point(V.T3)
    assert t["x"] == [0] * 14 and not L.is_inf(t) and M.g1_on_curve(V.T3)
    assert L.affine_of(L.g1_28_madd(t, L.a28_from_point(M.G1))) == M.g1_add(V.T3, M.G1)
    # scalar multiples by repeated insertion: k G against bigmodel.g1_mul
    acc, g = L.x28_infinity(), L.a28_from_point(M.G1)
    for k in range(1, 12):
        acc = L.g1_28_madd(acc, g)
        _check_point(acc, M.g1_mul(M.G1, k))


# ------------------------------------------------------------------------------------------------ the generated asm text
G = load(os.path.join(ROOT, "tools", "gen_mont_asm.py"), "gen_mont_asm")
# kind -> file, one per generated statement: fq28_mul2x_asm.inc is "mul2x"; the one Fr statement, fr29_mul2_asm.inc, is "fr"
INC = {"fr" if name.startswith("fr29_") else name[len("fq28_"):-len("_asm.inc")]: name for name in G.VARIANTS}


def asm(kind):
    return A.Asm(open(os.path.join(CSRC, INC[kind])).read())


def run_fq(prog, lines=None, **ops):
    out, ov = prog.run(A.env_of(L.FQ, "Fq28C", **ops), lines)
    return out, ov


def run_fr(prog, lines=None, **ops):
    return prog.run(A.env_of(L.FR, "Fr29C", **ops), lines)


def pairs(cases):
    return zip(cases[::2], cases[1::2])


def wrong(result, **want):
    """result of a run, the model's limbs per output name -> True when a multiply-add carried out or an output differs"""
    out, ov = result
    return ov != 0 or any(A.limbs_of(out, name, len(limbs)) != limbs for name, limbs in want.items())


# kind -> (prog, lines) -> number of mismatching cases on the statement's vectors.  Every statement of VARIANTS needs an entry.
COMPARE = {
    "mul": lambda p, l: sum(wrong(run_fq(p, l, a=a, b=b), r=L.fq28_mul(a, b)) for a, b in V.fq28_mul_cases()),
    "mul2x": lambda p, l: sum(wrong(run_fq(p, l, a0=a0, b0=b0, a1=a1, b1=b1), r0=L.fq28_mul(a0, b0), r1=L.fq28_mul(a1, b1))
                              for (a0, b0), (a1, b1) in pairs(V.fq28_mul_cases())),
    "mul2x_inplace": lambda p, l: sum(wrong(run_fq(p, l, a0=a0, b0=b0, a1=a1, b1=b1), a0=L.fq28_mul(a0, b0), a1=L.fq28_mul(a1, b1))
                                      for (a0, b0), (a1, b1) in pairs(V.fq28_mul_cases())),
    "sqr": lambda p, l: sum(wrong(run_fq(p, l, a=a), r=L.fq28_sqr(a)) for a in V.fq28_sqr_cases()),
    "mul2": lambda p, l: sum(wrong(run_fq(p, l, a=a, b=b, c=c, d=d), r=L.fq28_mul2(a, b, c, d)) for a, b, c, d in V.fq28_mul2_cases()),
    "fr": lambda p, l: sum(wrong(run_fr(p, l, a0=a0, b0=b0, a1=a1, b1=b1), r0=L.fr29_mul(a0, b0), r1=L.fr29_mul(a1, b1))
                                  for (a0, b0), (a1, b1) in pairs(V.fr29_mul_cases())),
}


def compare_all(kinds=tuple(INC), lines=None):
    """The .inc files on their vectors against the model -> number of mismatching cases per file (0 for the committed text).
    lines: {kind: instruction lines to run instead of the file's own}"""
    return {k: COMPARE[k](asm(k), (lines or {}).get(k)) for k in kinds}


def test_every_generated_statement_is_listed_once():
    """the *_asm.inc files of csrc/, the generator's VARIANTS, what fq28.hpp and fr29.hpp include, and the comparisons above: one set"""
    on_disk = {f for f in os.listdir(CSRC) if f.endswith("_asm.inc")}
    included = {m for h in ("fq28.hpp", "fr29.hpp") for m in re.findall(r'#include "(\w+\.inc)"', open(os.path.join(CSRC, h)).read())}
    assert on_disk == set(G.VARIANTS) == included
    assert set(COMPARE) == set(INC) and len(INC) == len(G.VARIANTS)


def test_asm_text_equals_the_model_bit_for_bit():
    assert len(INC) >= 6 and compare_all() == dict.fromkeys(INC, 0)


def test_no_multiply_add_carries_out_at_the_documented_limb_bounds():
    m28, m29, m30, m31, m32 = [(1 << k) - 1 for k in (28, 29, 30, 31, 32)]
    assert run_fq(asm("mul"), a=[m30] * 14, b=[m30] * 14)[1] == 0
    assert run_fq(asm("mul2x"), a0=[m30] * 14, b0=[m30] * 14, a1=[m30] * 14, b1=[m30] * 14)[1] == 0
    assert run_fq(asm("mul2x_inplace"), a0=[m30] * 14, b0=[m30] * 14, a1=[m30] * 14, b1=[m30] * 14)[1] == 0
    assert run_fq(asm("sqr"), a=[m30] * 14)[1] == 0
    assert run_fq(asm("mul2"), a=[m28] * 14, b=[m30] * 14, c=[m30] * 14, d=[m28] * 14)[1] == 0
    assert run_fq(asm("mul2"), a=[m29] * 14, b=[m29] * 14, c=[m29] * 14, d=[m29] * 14)[1] == 0
    assert run_fr(asm("fr"), a0=[m31] * 9, b0=[m29] * 9, a1=[m31] * 9, b1=[m29] * 9)[1] == 0
    # and the count means something: one more bit on one side carries out
    assert run_fq(asm("mul"), a=[m32] * 14, b=[m30] * 14)[1] > 0
    assert run_fq(asm("mul2x_inplace"), a0=[m32] * 14, b0=[m30] * 14, a1=[m30] * 14, b1=[m30] * 14)[1] > 0
    assert run_fq(asm("sqr"), a=[m31] * 14)[1] > 0
    assert run_fq(asm("mul2"), a=[m30] * 14, b=[m30] * 14, c=[m30] * 14, d=[m30] * 14)[1] > 0
    assert run_fr(asm("fr"), a0=[m32] * 9, b0=[m31] * 9, a1=[m31] * 9, b1=[m29] * 9)[1] > 0


def test_committed_asm_is_what_the_generators_produce():
    for name, variant in G.VARIANTS.items():
        assert open(os.path.join(CSRC, name), "rb").read() == G.statement(*variant)[0].encode(), name


def test_the_interpreter_refuses_a_constraint_it_does_not_know():
    text = open(os.path.join(CSRC, INC["mul2x_inplace"])).read()
    for bad in (text.replace('"+v"(a1.l[3])', '"+&v"(a1.l[3])'), text.replace('"s"(Fq28C::INV)', '"n"(Fq28C::INV)')):
        assert bad != text
        with pytest.raises(ValueError):
            A.Asm(bad)


def _mutations(prog, mod_first, mask):
    """three in-memory mutations of a statement's lines: one MOD operand index changed, one multiply-add dropped, the limb mask widened"""
    lines = prog.lines
    mods = [i for i, x in enumerate(lines) if x.startswith("v_mad") and re.search(r", %(\d+), v\[", x) and int(re.search(r", %(\d+), v\[", x).group(1)) > mod_first]
    i = mods[len(mods) // 2]
    n = int(re.search(r", %(\d+), v\[", lines[i]).group(1))
    wrong_mod = lines[:i] + [lines[i].replace(f", %{n}, v[", f", %{n - 1}, v[")] + lines[i + 1:]
    mads = [i for i, x in enumerate(lines) if x.startswith("v_mad")]
    j = mads[len(mads) // 3]
    dropped = lines[:j] + lines[j + 1:]
    ands = [i for i, x in enumerate(lines) if x.startswith("v_and_b32") and mask in x]
    k = ands[len(ands) // 2]
    wide = lines[:k] + [lines[k].replace(mask, hex(int(mask, 16) * 2 + 1))] + lines[k + 1:]
    assert wrong_mod != lines and dropped != lines and wide != lines
    return {"MOD operand index": wrong_mod, "dropped multiply-add": dropped, "widened mask": wide}


@pytest.mark.parametrize("kind", list(INC))
def test_comparison_notices_a_mutated_statement(kind):
    """The bit-for-bit comparison bites: each mutation of the text makes the file's vectors fail."""
    prog = asm(kind)
    first_mod = len(prog.outs) + len([e for e in prog.ins if "MOD" not in e and "INV" not in e])     # operand number of MOD[0] (Fr: MOD[1])
    for what, lines in _mutations(prog, first_mod, "0x1fffffff" if kind == "fr" else "0xfffffff").items():
        assert compare_all((kind,), {kind: lines})[kind] > 0, (kind, what)


def test_binding_and_kernels_agree_on_the_operation_numbers():
    import zkp_hip
    src = open(os.path.join(CSRC, "selftest.hpp")).read()
    enum = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"ST_([A-Z0-9_]+) = (\d+)", src)}
    for fam, ops in zkp_hip.SELFTEST_OPS.items():
        pre = {"fq28": "fq28_", "fr29": "fr29_", "fp": "fp_", "gl": "gl_", "g1": "g1_"}[fam]
        for name, num in ops.items():
            assert enum[pre + name] == num, (fam, name)
        assert enum[pre + "ops"] == len(ops)
