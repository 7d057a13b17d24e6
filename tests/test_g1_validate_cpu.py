"""The subgroup test of csrc/g1_check.hpp on the CPU: its constants against the big-integer model, and the chain itself
(tests/host/g1_check_chain.cpp, g++ alone, over HXyzz) with every verdict recomputed here as [r]P = O by an unreduced double-and-add."""
import os
import re
import subprocess

import bigmodel as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "zkp-implementation_amd", "csrc")

Z_ABS = 0xD201000000010000
BETA = 0x1A0111EA397FE699EC02408663D4DE85AA0D857D89759AD4897D29650FB85F9B409427EB4F49FFFD8BFD00000000AAAC
H = (Z_ABS + 1) ** 2 // 3  # (z - 1)^2 / 3 with z = -|z|


def _array(path, name, bits):
    src = open(os.path.join(CSRC, path)).read()
    body = re.search(name + r"\[\d+\]\s*=\s*\{([^}]*)\}", src).group(1)
    words = [int(w.rstrip("uUlL"), 0) for w in re.findall(r"0x[0-9a-fA-F]+[uUlL]*|\d+", body)]
    return words if bits is None else sum(w << (bits * i) for i, w in enumerate(words))


def mul_unreduced(pt, k):
    """[k]pt by double-and-add over bm.g1_add: bm.g1_mul reduces its scalar mod r, which is exactly what [r]P must not do"""
    acc = bm.INF
    for i in range(k.bit_length() - 1, -1, -1):
        acc = bm.g1_add(acc, acc)
        if (k >> i) & 1:
            acc = bm.g1_add(acc, pt)
    return acc


def in_g1(pt):
    return bm.g1_on_curve(pt) and mul_unreduced(pt, bm.R) is bm.INF


def phi(pt):
    return bm.INF if pt is bm.INF else (BETA * pt[0] % bm.P, pt[1])


def test_constants_of_the_header():
    src = open(os.path.join(CSRC, "g1_check.hpp")).read()
    assert int(re.search(r"Z_ABS = (0x[0-9a-f]+)ULL", src).group(1), 16) == Z_ABS
    assert Z_ABS * Z_ABS - 1 == _array("glv.hpp", "LAMBDA", 32)          # lambda = z^2 - 1
    assert _array("glv.hpp", "BETA", 64) == BETA
    bits = _array("g1_check.hpp", "Z_BITS", None)
    assert bits == [i for i in range(63, -1, -1) if (Z_ABS >> i) & 1] == [63, 62, 60, 57, 48, 16]
    # beta in the device-internal form: canonical residue of beta * 2^392, 14 limbs of 28 bits
    limbs = _array("g1_check.hpp", "BETA28", None)
    assert len(limbs) == 14 and all(l < (1 << 28) for l in limbs)
    assert sum(l << (28 * i) for i, l in enumerate(limbs)) == BETA * (1 << 392) % bm.P
    # the cofactor is odd (no 2-torsion: a doubling of an on-curve point never meets y = 0) and h r is the curve order's shape
    assert 3 * H == (Z_ABS + 1) ** 2 and H % 2 == 1
    lam = Z_ABS * Z_ABS - 1
    assert lam * lam + lam + 1 == bm.R


def test_identity_in_the_model():
    """[z^2]P = P + phi(P) on multiples of G; not on the small-x curve points, whose [h]Q passes and whose [r]Q does not"""
    for k in (1, 2, bm.R - 1, 0x1234567):
        p = bm.g1_mul(bm.G1, k)
        assert mul_unreduced(p, Z_ABS * Z_ABS) == bm.g1_add(p, phi(p))
    q = (4, pow(4 ** 3 + 4, (bm.P + 1) // 4, bm.P))
    assert bm.g1_on_curve(q) and not in_g1(q)
    assert mul_unreduced(q, Z_ABS * Z_ABS) != bm.g1_add(q, phi(q))
    hq, rq = mul_unreduced(q, H), mul_unreduced(q, bm.R)
    assert in_g1(hq) and rq is not bm.INF and not in_g1(rq)
    assert bm.g1_add(q, bm.g1_add(phi(q), phi(phi(q)))) is bm.INF     # P + phi(P) + phi^2(P) = O on the whole curve


def test_chain_on_the_host(tmp_path):
    exe = str(tmp_path / "g1_check_chain")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "g1_check_chain.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "g1_check: 233 cases, 0 failures" in r.stdout  # G, -G, 16 powers of two, 200 random, 10 small x, 2 of order 3, 3 more
    cases = re.findall(r"^case (\S+) x=([0-9a-f]{96}) y=([0-9a-f]{96}) in_g1=([01])$", r.stdout, flags=re.M)
    assert len(cases) == 233
    small_x = []
    x = 0
    while len(small_x) < 10:
        rhs = (x ** 3 + 4) % bm.P
        y = pow(rhs, (bm.P + 1) // 4, bm.P)
        if y * y % bm.P == rhs:
            small_x.append((x, y))
        x += 1
    assert [p[0] for p in small_x] == [0, 4, 5, 6, 8, 9, 10, 11, 12, 15]
    seen = {}
    for name, xs, ys, verdict in cases:
        pt = (int(xs, 16), int(ys, 16))
        assert bm.g1_on_curve(pt), name
        assert int(verdict) == int(in_g1(pt)), name     # every verdict again, with big integers
        seen[name] = pt
    assert seen["G"] == bm.G1 and seen["-G"] == bm.g1_neg(bm.G1) and seen["2^16G"] == bm.g1_mul(bm.G1, 1 << 16)
    assert [seen["small%d" % i] for i in range(10)] == small_x
    assert seen["(0,2)"] == (0, 2) and seen["(0,p-2)"] == (0, bm.P - 2) and seen["G+(0,2)"] == bm.g1_add(bm.G1, (0, 2))
    assert seen["[r]Q"] == mul_unreduced(small_x[1], bm.R) and seen["[h]Q"] == mul_unreduced(small_x[1], H)
    accepted = {n for n, _, _, v in cases if v == "1"}
    assert accepted == {"G", "-G", "[h]Q"} | {"2^%dG" % k for k in range(1, 17)} | {"rand%d" % i for i in range(200)}
