// g1_codec.hpp -- compressed G1 points and canonical scalars as bytes, to and from the ABI's limbs (zkp_g1_decompress*,
// zkp_g1_compress*, zkp_g1_bases_create_compressed, zkp_fr_from_bytes_dev, zkp_fr_to_bytes_dev: include/zkp_hip.h; entries:
// g1_codec_host.inc).
//
// The format: a point is 48 bytes.  Bits 7, 6 and 5 of byte 0 are the flags
//   c  compressed, must be 1
//   i  infinity
//   s  y is the larger of {y, p - y} as canonical integers, i.e. y > (p - 1) / 2
// and the remaining 381 bits are the canonical x, big-endian.  Infinity is c0 followed by 47 zero bytes.  It is what ark-bls12-381 0.4
// serialize_compressed writes and what the other BLS12-381 stacks exchange.  Decoding is strict; the status byte of a point is the first
// check that fails, in this order:
//   4  malformed encoding: c = 0, or i = 1 with s = 1 or any other bit set
//   1  non-canonical: x >= p
//   2  off the curve: x^3 + 4 is not a square
//   3  outside G1 -- only when the caller asked for the subgroup test (g1_check.hpp), which then runs as a second launch
// and 0 for a valid point, a well-formed infinity included.  1..3 mean what they mean in zkp_g1_validate.
//
// The square root: p = 3 (mod 4), so y = a^((p + 1) / 4) is a root of a whenever a has one, and y^2 = a tells whether it has.  The exponent
// is a compile-time constant of 379 bits walked MSB first in 2-bit digits over the table {a, a^2, a^3}: 378 squarings and 156 products,
// the same path in every lane.  The table is 3 x 14 words and stays in registers next to the accumulator and one product; a 4-bit table
// (15 x 14 words) would not.  -4 is no cube mod p, so no curve point has y = 0 and {y, p - y} are always two values.
//
// The chain and the sign rule are written once over an operations type Ops (Ops::El and the functions used below).  Under plain g++ they
// are instantiated with G1CodecHost over HFq (host_ff.hpp): tests/host/g1_codec_chain.cpp.  Under hipcc, with g1_ntt.hpp included first,
// with G1Codec28 over Fq28, and the kernels at the end of this file use it.
#pragma once
#include <stdint.h>

#ifndef __HIPCC__
#include "host_ff.hpp"
#endif

namespace zkp {

struct G1CodecParams {  // re-derived from the modulus by tests/test_g1_codec_cpu.py
    // (p + 1) / 4, 32-bit words, least significant first
    static constexpr uint32_t SQRT_EXP[12] = {0xffffeaabu, 0xee7fbfffu, 0xac54ffffu, 0x07aaffffu, 0x3dac3d89u, 0xd9cc34a8u,
                                              0x3ce144afu, 0xd91dd2e1u, 0x90d2eb35u, 0x92c6e9edu, 0x8e5ff9a6u, 0x0680447au};
    static constexpr int SQRT_DIGITS = 190;  // 2-bit digits; the top one (bits 378 and 379) is 1
    // (p - 1) / 2 in 13 limbs of 30 bits (the form of s30_canonical)
    static constexpr int32_t HALF30[13] = {0x3fffd555, 0x33fdffff, 0x0a9ffffd, 0x157fffd6, 0x187b120f, 0x21a541ed, 0x2895fb39,
                                           0x29709e70, 0x166bb23b, 0x0f6c8697, 0x34d258dd, 0x3d472ffc, 0x000d0088};
    // 2^784 mod p in 14 limbs of 28 bits: the Montgomery product of a canonical integer x with it is the internal residue x 2^392
    static constexpr uint32_t R2_392[14] = {0x010370edu, 0x06d1c345u, 0x0e243d62u, 0x0ec45c53u, 0x03b1d65au, 0x0093317du, 0x0b4f36a0u,
                                            0x05d74088u, 0x0c10ea72u, 0x0865d118u, 0x07320a75u, 0x0fd5cd50u, 0x0cc8a759u, 0x0000c8d4u};
};
static_assert(G1CodecParams::SQRT_EXP[11] >> 26 == 1, "the top digit of the exponent is 1: the chain starts from a");

// status byte of a decoded point: G1_VALID .. G1_OUTSIDE_SUBGROUP of g1_check.hpp, and
enum { G1_MALFORMED = 4 };
enum { G1_FLAG_C = 4, G1_FLAG_I = 2, G1_FLAG_S = 1 };  // the top three bits of byte 0, as a number

#ifndef ZKP_G1CODEC_FN
#ifdef __HIPCC__
#define ZKP_G1CODEC_FN __device__ __forceinline__
#else
#define ZKP_G1CODEC_FN inline
#endif
#endif

// digit i (bits 2i, 2i + 1) of the exponent.  The word is picked by compares against constants, so that the table folds into the
// instructions: no array is indexed at run time.
ZKP_G1CODEC_FN uint32_t g1_codec_sqrt_digit(int i) {
    uint32_t w = 0;
#ifdef __HIPCC__
#pragma unroll
#endif
    for (int k = 0; k < 12; k++) w = (i >> 4) == k ? G1CodecParams::SQRT_EXP[k] : w;
    return (w >> (2 * (i & 15))) & 3u;
}

// a^((p + 1) / 4): Ops::sqr, Ops::mul and Ops::pick(d, t1, t2, t3) = t_d for a digit d in 1..3 that is the same in every lane
template <class Ops>
ZKP_G1CODEC_FN typename Ops::El g1_codec_sqrt_candidate(const typename Ops::El& a) {
    typedef typename Ops::El El;
    const El a2 = Ops::sqr(a), a3 = Ops::mul(a2, a);
    El acc = a;
#ifdef __HIPCC__
#pragma unroll 1
#endif
    for (int i = G1CodecParams::SQRT_DIGITS - 2; i >= 0; i--) {
        acc = Ops::sqr(Ops::sqr(acc));
        const uint32_t d = g1_codec_sqrt_digit(i);
        if (d) acc = Ops::mul(acc, Ops::pick(d, a, a2, a3));  // uniform: the digits are constants
    }
    return acc;
}

// The y of a finite point from its x and its s flag: y = *negate ? Ops::neg(*root) : *root.  False when x^3 + 4 is no square (*root is
// then no coordinate of anything).  Ops::rhs(x) = x^3 + 4, Ops::is_root(y, a): y^2 = a, Ops::larger_half(y): the canonical integer of
// y is above (p - 1) / 2.
template <class Ops>
ZKP_G1CODEC_FN bool g1_codec_lift_x(const typename Ops::El& x, bool s, typename Ops::El* root, bool* negate) {
    const typename Ops::El a = Ops::rhs(x);
    *root = g1_codec_sqrt_candidate<Ops>(a);
    *negate = Ops::larger_half(*root) != s;
    return Ops::is_root(*root, a);
}

#ifndef __HIPCC__
struct G1CodecHost {
    typedef host::HFq El;
    static El sqr(const El& a) { return a.sqr(); }
    static El mul(const El& a, const El& b) { return a * b; }
    static const El& pick(uint32_t d, const El& t1, const El& t2, const El& t3) { return d == 1 ? t1 : d == 2 ? t2 : t3; }
    static El rhs(const El& x) { return x.sqr() * x + El::from_u64(4); }
    static bool is_root(const El& y, const El& a) { return y.sqr() == a; }
    static bool larger_half(const El& y) {  // y > (p - 1) / 2  <=>  2 y > p - 1  <=>  2 y >= p (p is odd)
        const El c = y.from_mont();
        uint64_t t[6];
        const uint64_t carry = host::Mont<6>::add(t, c.l, c.l);
        return carry || host::Mont<6>::ge(t, El::M().p);
    }
    static El neg(const El& y) { return y.neg(); }
};
#endif

#ifdef __HIPCC__
// Operand bounds (fq28.hpp): x tight; rhs < 6p with limbs 0..12 below 2^28, which sub8 takes as a subtrahend and a product as a factor
// (6 * 2 of the 2520 p^2); every power of the chain is a product, tight; neg is 4p - y with limbs below 2^30, a factor only.
struct G1Codec28 {
    typedef Fq28 El;
    static ZKP_DEV Fq28 sqr(const Fq28& a) { return fq28_sqr_chain(a); }
    static ZKP_DEV Fq28 mul(const Fq28& a, const Fq28& b) { return fq28_mul_chain(a, b); }
    static ZKP_DEV Fq28 pick(uint32_t d, const Fq28& t1, const Fq28& t2, const Fq28& t3) {
        Fq28 r;
#pragma unroll
        for (int i = 0; i < NL28; i++) r.l[i] = d == 1 ? t1.l[i] : d == 2 ? t2.l[i] : t3.l[i];
        return r;
    }
    static ZKP_DEV Fq28 rhs(const Fq28& x) {
        const Fq28 one = Fq28::one();
        const Fq28 two = one + one;
        return normalise(fq28_sqr_chain(x) * x + (two + two));  // as g1_28_on_curve
    }
    static ZKP_DEV bool is_root(const Fq28& y, const Fq28& a) {
        const Fq28 d = sub8(fq28_sqr_chain(y), a);  // < 10p, limbs < 2^30
        return tight_is_zero_mod_p(fq28_sqr_chain(d));
    }
    static ZKP_DEV bool larger_half(const Fq28& y) {
        Fq28 one = Fq28::zero();
        one.l[0] = 1;
        return s30_above_half(s30_canonical(y * one));  // y 2^392 * 1 / 2^392: the canonical integer
    }
    static ZKP_DEV Fq28 neg(const Fq28& y) { return sub4(Fq28::zero(), y); }
    // canonical integer of 30-bit limbs above (p - 1) / 2: the borrow of HALF - v
    static ZKP_DEV bool s30_above_half(const S30& v) {
        int32_t c = 0;
#pragma unroll
        for (int i = 0; i < NL30; i++) c = (G1CodecParams::HALF30[i] - v.v[i] + c) >> 30;
        return c < 0;
    }
};

// What the decode kernels accumulate per call: counts of statuses 1..4 and the smallest (index << 3 | status) of a bad point
struct G1DecodeReport {
    unsigned long long count[4];
    unsigned long long first;  // ~0 when nothing is bad
};

// as g1_check_reduce: four ballots, no atomic at all for a wave of valid points
ZKP_DEV void g1_decode_reduce(uint32_t status, uint64_t index, G1DecodeReport* rep) {
    const unsigned long long b1 = __ballot(status == 1), b2 = __ballot(status == 2), b3 = __ballot(status == 3), b4 = __ballot(status == 4);
    const unsigned long long bad = b1 | b2 | b3 | b4;
    if (!bad) return;
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned long long mine = lane == 0 ? b1 : lane == 1 ? b2 : lane == 2 ? b3 : b4;
    if (lane < 4 && mine) atomicAdd(&rep->count[lane], (unsigned long long)__popcll(mine));
    if (lane == __ffsll((long long)bad) - 1) atomicMin(&rep->first, ((unsigned long long)index << 3) | status);
}

// 48 big-endian bytes <-> 12 words, least significant first (the flags are the top three bits of word 11)
ZKP_DEV void g1_codec_load_be(const uint4* p, uint32_t* w) {
    const uint4 a = p[0], b = p[1], c = p[2];
    w[11] = __builtin_bswap32(a.x); w[10] = __builtin_bswap32(a.y); w[9] = __builtin_bswap32(a.z); w[8] = __builtin_bswap32(a.w);
    w[7] = __builtin_bswap32(b.x);  w[6] = __builtin_bswap32(b.y);  w[5] = __builtin_bswap32(b.z); w[4] = __builtin_bswap32(b.w);
    w[3] = __builtin_bswap32(c.x);  w[2] = __builtin_bswap32(c.y);  w[1] = __builtin_bswap32(c.z); w[0] = __builtin_bswap32(c.w);
}
ZKP_DEV void g1_codec_store_be(uint4* p, const uint32_t* w) {
    p[0] = make_uint4(__builtin_bswap32(w[11]), __builtin_bswap32(w[10]), __builtin_bswap32(w[9]), __builtin_bswap32(w[8]));
    p[1] = make_uint4(__builtin_bswap32(w[7]), __builtin_bswap32(w[6]), __builtin_bswap32(w[5]), __builtin_bswap32(w[4]));
    p[2] = make_uint4(__builtin_bswap32(w[3]), __builtin_bswap32(w[2]), __builtin_bswap32(w[1]), __builtin_bswap32(w[0]));
}

// n compressed points, one lane each; first = the global index of point 0 of this launch.  A lane whose point failed an earlier check,
// or is the infinity, runs the arithmetic on x = 0 (the curve point (0, 2)) and masks its answer.  A point with status != 0 is written
// as twelve zero limbs with is_inf = 0: (0, 0) is off the curve.
__global__ __launch_bounds__(MSM_THREADS) void g1_decode_kernel(const uint4* __restrict__ in, uint64_t n, uint64_t first,
                                                               uint4* __restrict__ out_xy, uint8_t* __restrict__ out_inf,
                                                               uint8_t* __restrict__ status, G1DecodeReport* __restrict__ rep) {
    const uint64_t i = (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    const bool live = i < n;
    Fq raw = Fq::zero();
    uint32_t flags = G1_FLAG_C;
    if (live) {
        g1_codec_load_be(in + i * 3, raw.l);
        flags = raw.l[11] >> 29;
        raw.l[11] &= 0x1fffffffu;
    }
    const bool s = (flags & G1_FLAG_S) != 0;
    const bool inf = (flags & G1_FLAG_I) != 0;
    const bool malformed = !(flags & G1_FLAG_C) || (inf && (s || !raw.is_zero()));
    uint32_t t[12];
    const bool canon = sub_limbs<12>(t, raw.l, FqParams::MOD) != 0;  // a borrow: below p
    if (malformed || inf || !canon) raw = Fq::zero();
    Fq28 r2;
#pragma unroll
    for (int k = 0; k < NL28; k++) r2.l[k] = G1CodecParams::R2_392[k];
    const Fq28 x = fq28_from_sat(raw) * r2;  // tight
    Fq28 root;
    bool negate;
    const bool on = g1_codec_lift_x<G1Codec28>(x, s, &root, &negate);
    const uint32_t st = malformed ? (uint32_t)G1_MALFORMED : inf ? (uint32_t)G1_VALID : !canon ? (uint32_t)G1_NON_CANONICAL
                  : !on ? (uint32_t)G1_OFF_CURVE : (uint32_t)G1_VALID;
    G1Affine o;
    o.x = fq28_to_abi(x);
    o.y = fq28_to_abi(negate ? G1Codec28::neg(root) : root);
    if (st != G1_VALID || inf) {
        o.x = Fq::zero();
        o.y = Fq::zero();
    }
    if (live) {
        o.store(out_xy + i * 6);
        out_inf[i] = st == G1_VALID && inf ? 1 : 0;
        if (status) status[i] = (uint8_t)st;
    }
    g1_decode_reduce(live ? st : (uint32_t)G1_VALID, first + i, rep);
}

// The subgroup half of a decode with ZKP_G1_DECODE_SUBGROUP, a launch of its own over the n points the decode kernel has just written
// (the chain of g1_check.hpp needs the whole register file and some scratch; the square root keeps three waves per SIMD without it).
// A point to test is one that is not flagged as infinity and not (0, 0), which is how every bad point was written; the others run the
// chain on (0, 0) and mask its answer, as g1_28_status does.  A point outside G1 gets status 3 and is zeroed like the other bad ones.
__global__ __launch_bounds__(MSM_THREADS) void g1_decode_subgroup_kernel(uint4* __restrict__ xy, const uint8_t* __restrict__ is_inf, uint64_t n,
                                                                        uint64_t first, uint8_t* __restrict__ status,
                                                                        G1DecodeReport* __restrict__ rep) {
    const uint64_t i = (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    const bool live = i < n;
    G1Affine p;
    p.x = Fq::zero();
    p.y = Fq::zero();
    if (live && !is_inf[i]) p = G1Affine::load(xy + i * 6);
    const bool finite = !(p.x.is_zero() && p.y.is_zero());
#pragma unroll 1
    for (int k = 0; k < 8; k++) {  // as g1_validate_raw_kernel: canonical in, canonical out
        p.x = dbl(p.x);
        p.y = dbl(p.y);
    }
    A28 q;
    q.x = fq28_from_sat(p.x);
    q.y = fq28_from_sat(p.y);
    const bool outside = !g1_in_subgroup<G1Check28>(q) && finite;
    if (outside) {
        G1Affine o;
        o.x = Fq::zero();
        o.y = Fq::zero();
        o.store(xy + i * 6);
        if (status) status[i] = (uint8_t)G1_OUTSIDE_SUBGROUP;
    }
    g1_decode_reduce(outside ? (uint32_t)G1_OUTSIDE_SUBGROUP : (uint32_t)G1_VALID, first + i, rep);
}

// n points in the 96-byte ABI form -> 48 bytes each.  No validation: limbs that are no point give bytes that are no encoding, and
// nothing here depends on the values.
__global__ __launch_bounds__(MSM_THREADS) void g1_encode_kernel(const uint4* __restrict__ in, const uint8_t* __restrict__ is_inf, uint64_t n,
                                                               uint4* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    if (i >= n) return;
    const bool inf = is_inf && is_inf[i];
    const G1Affine p = G1Affine::load(in + i * 6);
    Fq28 c = Fq28::zero();
    c.l[0] = 256;  // v 2^384 * 2^8 / 2^392 = v: out of Montgomery form
    const S30 x = s30_canonical(fq28_from_sat(p.x) * c), y = s30_canonical(fq28_from_sat(p.y) * c);
    Fq w = s30_to_sat(x);
    w.l[11] |= (uint32_t)G1_FLAG_C << 29 | (G1Codec28::s30_above_half(y) ? (uint32_t)G1_FLAG_S << 29 : 0u);
    if (inf) {
        w = Fq::zero();
        w.l[11] = (uint32_t)(G1_FLAG_C | G1_FLAG_I) << 29;
    }
    g1_codec_store_be(out + i * 3, w.l);
}

// ---- scalars: 32 canonical bytes, big-endian (Ethereum's KZG convention) or little-endian (ark's serialize of Fr), <-> Fr memory form
struct FrDecodeReport {
    unsigned long long bad;
    unsigned long long first;  // ~0 when nothing is bad
};

// a value >= r is counted, its index (first + its place in this launch) reported and its slot zeroed
__global__ __launch_bounds__(MSM_THREADS) void fr_from_bytes_kernel(const uint4* __restrict__ in, uint64_t n, uint32_t big_endian,
                                                                   uint4* __restrict__ out, uint64_t first, FrDecodeReport* __restrict__ rep) {
    const uint64_t i = (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    Fr v = Fr::zero();
    if (i < n) {
        v = Fr::load(in + i * 2);
        if (big_endian) {
            Fr b;
#pragma unroll
            for (int k = 0; k < 8; k++) b.l[k] = __builtin_bswap32(v.l[7 - k]);
            v = b;
        }
    }
    uint32_t t[8];
    const bool bad = sub_limbs<8>(t, v.l, FrParams::MOD) == 0;  // no borrow: r or more
    if (bad) v = Fr::zero();
    if (i < n) (v * Fr::r2()).store(out + i * 2);
    const unsigned long long b = __ballot(bad);
    if (!b) return;
    const int lane = (int)(threadIdx.x & 63u);
    if (lane == __ffsll((long long)b) - 1) {
        atomicAdd(&rep->bad, (unsigned long long)__popcll(b));
        atomicMin(&rep->first, (unsigned long long)(first + i));
    }
}

__global__ __launch_bounds__(MSM_THREADS) void fr_to_bytes_kernel(const uint4* __restrict__ in, uint64_t n, uint32_t big_endian,
                                                                 uint4* __restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    if (i >= n) return;
    Fr v = from_mont(Fr::load(in + i * 2));
    if (big_endian) {
        Fr b;
#pragma unroll
        for (int k = 0; k < 8; k++) b.l[k] = __builtin_bswap32(v.l[7 - k]);
        v = b;
    }
    v.store(out + i * 2);
}
#endif  // __HIPCC__

}  // namespace zkp
