"""Big-integer model of the compressed G1 encoding (csrc/g1_codec.hpp, include/zkp_hip.h), straight from its definition.

A point is 48 bytes: bits 7, 6, 5 of byte 0 are c (compressed, must be 1), i (infinity), s (y > (p - 1) / 2); the other 381 bits are
the canonical x, big-endian.  Infinity is c0 followed by 47 zero bytes.  Points are bigmodel's: (x, y) canonical integers, or bm.INF.
"""
import bigmodel as bm

P, R = bm.P, bm.R
HALF = (P - 1) // 2
RINV = pow(1 << 384, -1, P)  # out of the ABI's Montgomery form
VALID, NON_CANONICAL, OFF_CURVE, OUTSIDE_SUBGROUP, MALFORMED = 0, 1, 2, 3, 4
INF_BYTES = bytes([0xC0]) + bytes(47)
WORDS = {NON_CANONICAL: "canonical", OFF_CURVE: "curve", OUTSIDE_SUBGROUP: "subgroup", MALFORMED: "encoding"}


def compress(pt):
    if pt is bm.INF:
        return INF_BYTES
    x, y = pt
    return (x | 1 << 383 | (1 << 381 if y > HALF else 0)).to_bytes(48, "big")


def sqrt(a):
    """a root of a mod p (p = 3 mod 4), or None"""
    y = pow(a, (P + 1) // 4, P)
    return y if y * y % P == a % P else None


def mul_unreduced(pt, k):
    """[k]pt with the scalar as it is (bm.g1_mul reduces it mod r, which [r]P must not)"""
    acc = bm.INF
    for i in range(k.bit_length() - 1, -1, -1):
        acc = bm.g1_add(acc, acc)
        if (k >> i) & 1:
            acc = bm.g1_add(acc, pt)
    return acc


def decompress(b, check_subgroup=False):
    """-> (status, point); the point is only meaningful with status VALID (bm.INF, the infinity, is None as well)"""
    v = int.from_bytes(b, "big")
    c, i, s, x = v >> 383 & 1, v >> 382 & 1, v >> 381 & 1, v & ((1 << 381) - 1)
    if not c or (i and (s or x)):
        return MALFORMED, None
    if i:
        return VALID, bm.INF
    if x >= P:
        return NON_CANONICAL, None
    y = sqrt(x ** 3 + 4)
    if y is None:
        return OFF_CURVE, None
    if (y > HALF) != bool(s):
        y = P - y
    if check_subgroup and mul_unreduced((x, y), R) is not bm.INF:
        return OUTSIDE_SUBGROUP, None
    return VALID, (x, y)


def abi_row(pt):
    """the twelve u64 limbs of the ABI (Montgomery radix 2^384, x then y) of a finite point; zeros for None"""
    if pt is None:
        return [0] * 12
    x, y = pt[0] * bm.FQ_MONT_R % P, pt[1] * bm.FQ_MONT_R % P
    return [(x >> (64 * k)) & bm.MASK64 for k in range(6)] + [(y >> (64 * k)) & bm.MASK64 for k in range(6)]


def point_of_row(row):
    """a finite point from twelve ABI limbs (no check)"""
    x = sum(int(v) << (64 * k) for k, v in enumerate(row[:6]))
    y = sum(int(v) << (64 * k) for k, v in enumerate(row[6:12]))
    return (x * RINV % P, y * RINV % P)


def fr_to_bytes(v, big_endian):
    return v.to_bytes(32, "big" if big_endian else "little")


def fr_from_bytes(b, big_endian):
    """-> (ok, canonical value or 0)"""
    v = int.from_bytes(b, "big" if big_endian else "little")
    return (True, v) if v < R else (False, 0)
