"""A small interpreter for the generated asm statements of csrc/*_asm.inc (tools/gen_mont_asm.py).

It executes the committed TEXT: the instruction lines with their %N operand numbers, bound to C expressions by the constraint lists at
the end of the statement.  Seven opcodes and the constraints "=&v", "+v", "v", "s" occur; anything else is an error.  Every v_mad_u64_u32 whose exact result needs more than 64
bits is counted in `overflows` (the hardware would drop the carry into vcc, which nothing reads)."""
import re

M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def bind(line, known):
    """one constraint line -> [(constraint, C expression)]; every "..."(...) group on it must parse, with a constraint from `known`"""
    ops = []
    for group in line.strip().lstrip(":").strip().split(", "):
        m = re.fullmatch(r'"([^"]*)"\(([^(),]+)\)', group)
        if not m or m.group(1) not in known:
            raise ValueError(f"operand outside the interpreter (constraints {known}): {group}")
        ops.append(m.groups())
    return ops


class Asm:
    def __init__(self, text):
        self.lines = re.findall(r'^\s*"([^"\\]+)\\n\\t"', text, flags=re.M)
        tail = text[text.rindex('\\n\\t"'):]
        outs, ins, _clob = [x for x in tail.split("\n") if x.strip().startswith(":")]
        outs, ins = bind(outs, ("=&v", "+v")), bind(ins, ("v", "s"))
        self.outs, self.ins = [e for _, e in outs], [e for _, e in ins]
        self.inouts = [i for i, (con, _) in enumerate(outs) if con == "+v"]      # read-write: seeded from env, read back at the end
        assert self.lines and self.outs and self.ins

    def run(self, env, lines=None):
        """env: C expression -> value for every input and read-write operand (e.g. "a.l[3]", "Fq28C::MOD[0]").
        -> ({output expression: value}, overflows)"""
        reg = {f"%{i}": env[self.outs[i]] & M32 for i in self.inouts}
        for i, e in enumerate(self.ins):
            reg[f"%{len(self.outs) + i}"] = env[e] & M32
        overflows = 0

        def rd(tok):
            if tok.startswith("v["):
                lo = int(tok[2:tok.index(":")])
                return reg[f"v{lo}"] | (reg[f"v{lo + 1}"] << 32)
            if tok.startswith(("%", "v")):
                return reg[tok]
            return int(tok, 0)

        def wr(tok, val):
            if tok.startswith("v["):
                lo = int(tok[2:tok.index(":")])
                reg[f"v{lo}"], reg[f"v{lo + 1}"] = val & M32, (val >> 32) & M32
            else:
                reg[tok] = val & M32

        for line in (self.lines if lines is None else lines):
            op, rest = line.split(None, 1)
            # operands are separated by ", " outside the brackets of a register pair
            a = [x.strip() for x in re.split(r",\s*(?![^\[]*\])", rest)]
            if op == "v_mad_u64_u32":
                assert a[1] == "vcc"
                v = rd(a[2]) * rd(a[3]) + rd(a[4])
                overflows += v > M64
                wr(a[0], v & M64)
            elif op == "v_mul_lo_u32":
                wr(a[0], rd(a[1]) * rd(a[2]))
            elif op == "v_and_b32":
                wr(a[0], rd(a[1]) & rd(a[2]))
            elif op == "v_lshrrev_b64":
                wr(a[0], rd(a[2]) >> rd(a[1]))
            elif op == "v_lshlrev_b32":
                wr(a[0], rd(a[2]) << rd(a[1]))
            elif op == "v_mov_b32":
                wr(a[0], rd(a[1]))
            elif op == "v_sub_u32":
                wr(a[0], rd(a[1]) - rd(a[2]))
            else:
                raise ValueError("opcode outside the interpreter: " + line)
        return {e: reg[f"%{i}"] for i, e in enumerate(self.outs) if f"%{i}" in reg}, overflows


def env_of(consts, prefix, **elems):
    """{"a.l[i]": ...} for every named limb list + the constants of the header struct (`prefix`::MOD[j], ::INV)"""
    env = {}
    for name, limbs in elems.items():
        for i, v in enumerate(limbs):
            env[f"{name}.l[{i}]"] = v
    for i, v in enumerate(consts["MOD"]):
        env[f"{prefix}::MOD[{i}]"] = v
    if "INV" in consts:
        env[f"{prefix}::INV"] = consts["INV"]
    return env


def limbs_of(out, name, n):
    return [out[f"{name}.l[{i}]"] for i in range(n)]
