#!/usr/bin/env python3
"""Instructions one insertion costs in msm_accumulate_kernel: the generic g1_28_madd<true> iteration of the steady-state loop of
msm_accumulate_run, opcode by opcode, the generated asm statements (the product chains, csrc/fq28_*_asm.inc) split from the code around
them.  Reads the device assembly hipcc writes with -S (the asm statements are bracketed by ;;#ASMSTART / ;;#ASMEND there):

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S zkp-implementation_amd/csrc/api.hip -o api.s
    python tools/acc_insertion_census.py api.s [--md] [kernel name part, default msm_accumulate_kernel]

The kernel holds msm_accumulate_run twice (a bucket's run, the pieces of an oversized bucket); each copy is reported.  How the iteration
is found: the innermost loop around a run of seven asm statements with the multiply-add counts of an insertion (two double products of
784, two squarings of 301, two products of 392, the fused pair of 588) is walked from its header.  At a conditional branch the walk
falls through -- the sign of the digit, the plane of the entry -- unless the block it would enter holds compiler-made multiply-adds
(the same-x paths: doubling, the squaring of R), and once the last chain is behind it takes every skip (the first insertion into an
empty bucket).  The labels of the walk are printed, so the path can be checked against the listing."""
import collections
import re
import sys

SIGNATURE = sorted([784, 784, 301, 301, 392, 392, 588])
HALF_RATE = ("v_mad_u64_u32", "v_mul_lo_u32", "v_mul_hi_u32", "v_lshrrev_b64", "v_lshlrev_b64", "v_lshl_add_u64", "v_add3_u32", "v_or3_b32",
             "v_lshl_add_u32", "v_mov_b64", "v_alignbit_b32", "v_add_lshl_u32", "v_and_or_b32", "v_lshl_or_b32", "v_xad_u32")  # bench_micro/issue_rate.hip


class Block:
    def __init__(self, label):
        self.label, self.ops, self.asm, self.term, self.target = label, collections.Counter(), [], None, None

    def mads_outside(self):
        return self.ops["v_mad_u64_u32"]


def parse(body):
    """basic blocks of a kernel's listing, in order; an asm statement is one item of its block"""
    blocks = [Block("entry")]
    cur_asm = None
    for line in body:
        s = line.strip()
        if s.startswith(";;#ASMSTART"):
            cur_asm = collections.Counter()
            continue
        if s.startswith(";;#ASMEND"):
            if cur_asm:  # (an empty statement is a barrier for the optimiser -- fq28.hpp: pinned -- and no instruction)
                blocks[-1].asm.append(cur_asm)
            cur_asm = None
            continue
        m = re.match(r"(\.LBB\d+_\d+):", s)
        if m:
            if blocks[-1].ops or blocks[-1].asm or blocks[-1].term:
                blocks.append(Block(m.group(1)))
            else:
                blocks[-1].label = m.group(1)
            continue
        if not s or s.startswith((";", ".")):
            continue
        op = s.split()[0]
        if op.endswith(("_e32", "_e64")):
            op = op[:-4]
        if cur_asm is not None:
            cur_asm[op] += 1
            continue
        blocks[-1].ops[op] += 1
        if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm")):
            blocks[-1].term = op
            t = re.search(r"(\.LBB\d+_\d+)", s)
            blocks[-1].target = t.group(1) if t else None
            blocks.append(Block(None))
    return blocks


def census(blocks):
    index = {b.label: i for i, b in enumerate(blocks) if b.label}
    flat = [(i, a) for i, b in enumerate(blocks) for a in b.asm]
    out = []
    j = 0
    while j + 7 <= len(flat):
        if sorted(a["v_mad_u64_u32"] for _, a in flat[j:j + 7]) != SIGNATURE:
            j += 1
            continue
        first, last = flat[j][0], flat[j + 6][0]
        j += 7
        # innermost loop: the closest backward branch after the last chain whose target lies at or before the first
        header = None
        for i in range(last, len(blocks)):
            t = blocks[i].target
            if t in index and index[t] <= first and blocks[i].term != "s_setpc_b64":
                header = index[t]
                back = i
                break
        if header is None:
            continue
        path, i, seen_last = [], header, False
        while True:
            b = blocks[i]
            path.append(i)
            seen_last = seen_last or i == last
            if i == back:
                break
            nxt = i + 1
            if b.term == "s_branch":
                nxt = index[b.target]
            elif b.term and b.term.startswith("s_cbranch") and b.target in index:
                skip = seen_last or blocks[i + 1].mads_outside() >= 50
                if skip and index[b.target] > i:
                    nxt = index[b.target]
            if nxt <= i and nxt != header or len(path) > 500:
                break
            if nxt == header:
                break
            i = nxt
        inside, outside = collections.Counter(), collections.Counter()
        for i in path:
            outside.update(blocks[i].ops)
            for a in blocks[i].asm:
                inside.update(a)
        out.append(([blocks[i].label or f"(after {blocks[i - 1].label or i - 1})" for i in path], inside, outside))
    return out


def report(path, inside, outside, md):
    tot_in, tot_out = sum(inside.values()), sum(outside.values())
    mads = inside["v_mad_u64_u32"]
    valu_out = sum(c for o, c in outside.items() if o.startswith("v_"))
    half_out = sum(c for o, c in outside.items() if o in HALF_RATE)
    half_in = sum(c for o, c in inside.items() if o in HALF_RATE) - mads
    print(f"path: {' '.join(path)}")
    print(f"{tot_in + tot_out} instructions per insertion: {mads} multiply-adds, {tot_in - mads} others inside the asm statements "
          f"({half_in} at the multiply-add's issue rate), {tot_out} outside ({valu_out} VALU, {half_out} of them at the multiply-add's rate; "
          f"{sum(c for o, c in outside.items() if o.startswith('s_'))} scalar, "
          f"{sum(c for o, c in outside.items() if o.startswith(('global_', 'flat_', 'buffer_')))} memory)")
    ops = sorted(set(inside) | set(outside), key=lambda o: -(inside[o] + outside[o]))
    if md:
        print("\n| opcode | inside asm | outside |\n|---|---|---|")
        for o in ops:
            print(f"| `{o}` | {inside[o] or ''} | {outside[o] or ''} |")
        print()
    else:
        for o in ops:
            print(f"    {o:24s} {inside[o]:6d} {outside[o]:6d}")


def main():
    args = [a for a in sys.argv[1:] if a != "--md"]
    md = "--md" in sys.argv
    pat = args[1] if len(args) > 1 else "msm_accumulate_kernel"
    src = open(args[0]).read()
    for f in re.split(r"\n(?=_Z\w+:)", src):
        m = re.match(r"(_Z\w+):", f)
        if not m or pat not in m.group(1):
            continue
        end = f.find(".Lfunc_end")
        body = f[:end if end > 0 else len(f)].split("\n")
        res = census(parse(body))
        print(f"{m.group(1)}: {len(res)} insertion loop(s)")
        for k, (path, inside, outside) in enumerate(res):
            print(f"\nloop {k}")
            report(path, inside, outside, md)
        for key in ("NumVgprs", "ScratchSize", "Occupancy"):
            mm = re.search(r"; %s: (\d+)" % key, f)
            if mm:
                print(f"{key} {mm.group(1)}", end="  ")
        print()


if __name__ == "__main__":
    main()
