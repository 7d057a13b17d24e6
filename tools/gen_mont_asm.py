#!/usr/bin/env python3
"""Generate every csrc/*_asm.inc: the body of a Montgomery product (product scanning, one column at a time) as ONE asm statement whose
multiply-adds form a strict chain.  VARIANTS below is the list of statements; tests/test_limb_model_cpu.py takes its list from it.
No argument: rewrite all the files.  --check: compare instead, exit 1 when a file differs.  Experiments import statement().

Why an asm block (profiles/r05_f_ntt_where_the_time_goes.md, section 4): integer addition is associative, so the compiler re-associates
every column sum -- it starts the column from zero, often as two sub-chains, and adds the pieces, the previous column's carry and the
widened m[k] afterwards: 24 v_lshl_add_u64 + 12 v_mov in the 235 instructions of an Fr product, 25 v_lshl_add_u64 in the 486 of an Fq
product.  A strict chain (carry = addend of the column's first multiply-add; Fr adds m[k] as m[k] * 1) is 206 and 461 instructions.
Why ONE statement: written as separate asm statements the chain is correct but the hazard recogniser, which cannot see inside asm,
separates every two dependent statements with an s_nop; inside one statement it inserts nothing, and the hardware needs no wait between
dependent v_mad_u64_u32 (the compiler's own chains have none).  Two chains are interleaved instruction by instruction, which keeps
every dependent pair two instructions apart anyway.

Registers.  The 64-bit accumulators are the fixed VGPR pairs v[ACC0+2c : ACC0+2c+1] (ACC0 even: 64-bit operands are even-aligned on
gfx90a and later), named in the clobber list: an asm operand of 64 bits cannot be addressed by halves, and the low half is what m[k] and
the result limbs are cut from.  The result limbs double as the storage of m[]: m[j] is last read in column j + NL - 1, result limb j is
written in column j + NL.  In place (a_c *= b_c): limb j of a is likewise read for the last time in column j + NL - 1, so the result can
take a's registers once m[] gets outputs of its own (m_c); a loop that carries a (ZZ, ZZZ of the bucket accumulator in msm_accumulate)
then needs no copy of the result back.

Forms.  mul: a b.  mul2: (a b + c d) / R with one reduction, all in one chain per column (Fq: 392 + 196 multiply-adds).  sqr: every
off-diagonal product once against the doubled operand dbl = 2 a (13 shifts: a[NL-1] is never the smaller index of a pair; limbs of
a < 2^30 keep the <= 7 doubled products of a column + the reduction terms below 2^64): Fq 105 + 196 multiply-adds instead of 392.

Tried and not kept: fr29 mul with ONE chain for the memory-form Fr product of fr29.hpp's operator*.  The element-wise kernels that use
it are no faster with it (PLONK 2^16 3.55 against 3.50 ms) and the fixed accumulator pair costs them registers."""
import os
import sys

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "zkp-implementation_amd", "csrc")

# field -> limbs, bits per limb, the struct of constants, and whether m[k] = lo * INV (else m[k] = 0 - lo, added as m[k] * 1: MOD[0] = 1)
FIELDS = {"fq28": (14, 28, "Fq28C", True), "fr29": (9, 29, "Fr29C", False)}
# file -> (field, form, chains, first accumulator VGPR)
VARIANTS = {
    "fq28_mul_asm.inc": ("fq28", "mul", 1, 164),
    "fq28_mul2x_asm.inc": ("fq28", "mul", 2, 164),
    "fq28_mul2x_inplace_asm.inc": ("fq28", "mul_inplace", 2, 164),
    "fq28_sqr_asm.inc": ("fq28", "sqr", 1, 164),
    "fq28_mul2_asm.inc": ("fq28", "mul2", 1, 164),
    "fr29_mul2_asm.inc": ("fr29", "mul", 2, 100),
}


def statement(field, form, chains, acc0):
    """-> (text of the asm statement, instructions per product, multiply-adds per product).  Operands are the C expressions themselves
    until the end, where each gets its %N from its place in the output list followed by the input list."""
    nl, bits, consts, has_inv = FIELDS[field]
    mask = hex((1 << bits) - 1)
    mod = [f"{consts}::MOD[{j}]" if j or has_inv else "1" for j in range(nl)]
    scalars = [x for x in mod if x != "1"] + ([f"{consts}::INV"] if has_inv else [])
    out_groups, in_groups, seqs = [], [], []         # per chain: lists of (constraint, limbs)
    for c in range(chains):
        limbs = lambda name, member=".l": [f"{name}{c if chains > 1 else ''}{member}[{i}]" for i in range(nl)]
        a, b, acc, lo = limbs("a"), limbs("b"), f"v[{acc0 + 2 * c}:{acc0 + 2 * c + 1}]", f"v{acc0 + 2 * c}"
        res = m = limbs("r")                         # m[k] shares the result's registers, except in place
        pairs = [(a, b)] + ([(limbs("c"), limbs("d"))] if form == "mul2" else [])
        if form == "mul_inplace":
            res, m = a, limbs("m", "")
            out_groups.append([("+v", a), ("=&v", m)])
            in_groups.append([b])
        elif form == "sqr":
            dbl = limbs("dbl", "")
            out_groups.append([("=&v", res), ("=&v", dbl)])
            in_groups.append([a])
        else:
            out_groups.append([("=&v", res)])
            in_groups.append([x for pair in pairs for x in pair])
        seq = [("v_lshlrev_b32", dbl[i], "1", a[i]) for i in range(nl - 1)] if form == "sqr" else []
        seqs.append(seq)
        for k in range(2 * nl - 1):                  # the column walk: products, reduction terms, then m[k] (low half) or a result limb
            cols = range(max(0, k - nl + 1), min(k, nl - 1) + 1)
            if form == "sqr":
                terms = [(dbl[i], a[k - i]) if i < k - i else (a[i], a[i]) for i in cols if i <= k - i]
            else:
                terms = [(x[i], y[k - i]) for x, y in pairs for i in cols]
            terms += [(m[i], mod[k - i]) for i in range(cols[0], min(k, nl))]
            if k < nl:
                seq += [("v_mad_u64_u32", acc, "vcc", x, y, acc if k or j else "0") for j, (x, y) in enumerate(terms)]
                seq.append(("v_mul_lo_u32", m[k], lo, scalars[-1]) if has_inv else ("v_sub_u32", m[k], "0", lo))
                seq.append(("v_and_b32", m[k], mask, m[k]))
                seq.append(("v_mad_u64_u32", acc, "vcc", m[k], mod[0], acc))
            else:
                seq += [("v_mad_u64_u32", acc, "vcc", x, y, acc) for x, y in terms]
                seq.append(("v_and_b32", res[k - nl], mask, lo))
            seq.append(("v_lshrrev_b64", acc, str(bits), acc))
        seq.append(("v_mov_b32", res[nl - 1], lo))
    outs = [(con, e) for groups in zip(*out_groups) for con, group in groups for e in group]        # group-major: a0 a1 m0 m1
    ins = [("v", e) for groups in in_groups for group in groups for e in group] + [("s", e) for e in scalars]   # chain-major: a0 b0 a1 b1
    num = {e: f"%{n}" for n, (_, e) in enumerate(outs + ins)}
    n, n_mad = len(seqs[0]), sum(x[0] == "v_mad_u64_u32" for x in seqs[0])
    text = [f"// GENERATED by tools/gen_mont_asm.py ({field} {form}, chains {chains}, accumulators from v{acc0}) -- do not edit.  "
            f"{n} instructions per product ({n_mad} v_mad_u64_u32).", "asm("]
    text += [f'    "{x[0]} {", ".join(num.get(o, o) for o in x[1:])}\\n\\t"' for group in zip(*seqs) for x in group]
    text += ["    : " + ", ".join(f'"{con}"({e})' for con, e in lst) for lst in (outs, ins)]
    text.append("    : " + ", ".join(['"vcc"'] + [f'"v{acc0 + i}"' for i in range(2 * chains)]) + ");")
    return "\n".join(text) + "\n", n, n_mad


if __name__ == "__main__":
    if sys.argv[1:] not in ([], ["--check"]):
        sys.exit(__doc__)
    differ = 0
    for name, variant in VARIANTS.items():
        text, n, n_mad = statement(*variant)
        path = os.path.join(CSRC, name)
        if sys.argv[1:]:
            same = os.path.exists(path) and open(path).read() == text
            differ += not same
            print(name, "is up to date" if same else "DIFFERS from what the generator emits")
        else:
            open(path, "w").write(text)
            print(name, n, "instructions per product,", n_mad, "multiply-adds")
    sys.exit(differ != 0)
