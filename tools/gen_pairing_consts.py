#!/usr/bin/env python3
"""Print the Frobenius constant block of csrc/pairing_tower.hpp (between its GENERATED markers) from the big-int model:
gamma_(k,m) = xi^(m (p^k - 1) / 6) for k = 1, 2, 3 and m = 1 .. 5, each an Fq2 of two Montgomery residues (radix 2^384) as six
little-endian 64-bit words.  tests/test_pairing_tower_cpu.py checks the header against the same table."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests", "model"))
import pairing_fast_model as FM  # noqa: E402


def block():
    lines = []
    words = FM.frobenius_table_words()
    for i, w in enumerate(words):
        k, m = i // 5 + 1, i % 5 + 1
        c0 = ", ".join("0x%016xull" % x for x in w[:6])
        c1 = ", ".join("0x%016xull" % x for x in w[6:])
        lines.append("    if (K == %d && m == %d) return Fq2<F>{F::lit(%s),\n                                        F::lit(%s)};" % (k, m, c0, c1))
    return "\n".join(lines)


if __name__ == "__main__":
    print(block())
