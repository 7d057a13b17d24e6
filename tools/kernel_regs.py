#!/usr/bin/env python3
"""Register / scratch usage of the gfx950 kernels inside a built library (reads the code object of every translation unit out of the HIP fat binary):
    python tools/kernel_regs.py [lib.so] [name filter ...]"""
import re
import struct
import subprocess
import sys
import tempfile

path = sys.argv[1] if len(sys.argv) > 1 and sys.argv[1].endswith(".so") else "zkp-implementation_amd/libzkp_hip.so"
filters = [a for a in sys.argv[1:] if not a.endswith(".so")]
data = open(path, "rb").read()
g = lambda blk, k: (re.search(r"\.%s:\s+(\d+)" % k, blk) or [0, "?"])[1]
i = data.find(b"__CLANG_OFFLOAD_BUNDLE__")
while i >= 0:  # one bundle per translation unit of the library
    n = struct.unpack_from("<Q", data, i + 24)[0]
    off = i + 32
    co = None
    for _ in range(n):
        o, sz, tl = struct.unpack_from("<QQQ", data, off)
        off += 24
        triple = data[off:off + tl].decode()
        off += tl
        if "gfx950" in triple:
            co = data[i + o:i + o + sz]
    i = data.find(b"__CLANG_OFFLOAD_BUNDLE__", i + 1)
    if co is None:
        continue
    with tempfile.NamedTemporaryFile(suffix=".o") as f:  # private to this run: a fixed name under /tmp may belong to another user
        f.write(co)
        f.flush()
        txt = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True).stdout
    for blk in txt.split("- .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if not name or (filters and not any(f in name.group(1) for f in filters)):
            continue
        dem = subprocess.run(["c++filt", name.group(1)], capture_output=True, text=True).stdout.strip()
        print(f"{dem.split('(')[0][:70]:70s} vgpr {g(blk, 'vgpr_count'):>4} agpr {blk.split()[0]:>4} sgpr {g(blk, 'sgpr_count'):>4} "
              f"spill {g(blk, 'vgpr_spill_count'):>3} scratch {g(blk, 'private_segment_fixed_size'):>5} lds {g(blk, 'group_segment_fixed_size'):>6}")
