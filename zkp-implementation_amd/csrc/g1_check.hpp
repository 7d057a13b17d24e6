// g1_check.hpp -- is an affine point of y^2 = x^3 + 4 in the prime-order subgroup G1?  The test of zkp_g1_validate* (include/zkp_hip.h).
//
// With z = -0xd201000000010000 and phi(x, y) = (beta x, y) (glv.hpp):  P is in G1  <=>  [z^2]P = P + phi(P).
//   sound:    phi^2 + phi + 1 = 0 on the whole curve; if phi(P) = [lambda]P with lambda = z^2 - 1 then [lambda^2 + lambda + 1]P = [r]P = O
//   complete: phi acts as lambda on G1
// [z^2]P = [|z|]([|z|]P): |z| has six set bits, so each pass is 63 doublings and 5 additions -- 126 doublings instead of the 255 of
// [r]P.  The chain is a compile-time constant: every lane of a wave takes the same path.  #E(Fq) = h r with h = (z - 1)^2 / 3 odd, so an
// on-curve point never doubles to y = 0; the other exceptional cases of the additions (an infinite accumulator, equal and opposite
// operands) ARE reached by points of small order -- (0, 2) has order 3 -- and the point operations handle them.
//
// The chain is written once over an operations type Ops (Ops::Affine, Ops::Point and the seven functions used below).  Under plain
// g++ it is instantiated with G1CheckHost over HXyzz (host_ff.hpp): tests/host/g1_check_chain.cpp.  Under hipcc, with msm.hpp included
// first, with G1Check28 over A28 / X28 (g1_28.hpp), and the two kernels at the end of this file use it.
#pragma once
#include <stdint.h>

#include "glv.hpp"
#ifndef __HIPCC__
#include "host_ff.hpp"
#endif

namespace zkp {

struct G1CheckParams {
    static constexpr uint64_t Z_ABS = 0xd201000000010000ULL;  // |z|
    static constexpr int Z_BITS[6] = {63, 62, 60, 57, 48, 16};
    // beta (GlvParams::BETA) in the device-internal form: beta * 2^392 mod p, canonical, 28-bit limbs (tests/test_g1_validate_cpu.py)
    static constexpr uint32_t BETA28[14] = {0x02421b59u, 0x0bee4867u, 0x01d31002u, 0x04760184u, 0x04cc5086u, 0x0c76dc00u, 0x0aae891bu,
                                            0x0ac70ad2u, 0x0fe377c4u, 0x0e4686b8u, 0x05ed1568u, 0x08f5a180u, 0x002b5c1fu, 0x0000d1a4u};
};

// status byte of a point, the first failing check: include/zkp_hip.h
enum { G1_VALID = 0, G1_NON_CANONICAL = 1, G1_OFF_CURVE = 2, G1_OUTSIDE_SUBGROUP = 3 };

#ifndef ZKP_G1CHECK_FN
#ifdef __HIPCC__
#define ZKP_G1CHECK_FN __device__ __forceinline__
#else
#define ZKP_G1CHECK_FN inline
#endif
#endif

// [|z|] q added up MSB first; the top bit is the operand itself.  `first` is 2 q (Ops has a cheaper doubling for an affine q).
template <class Ops, class Q, class Add>
ZKP_G1CHECK_FN typename Ops::Point g1_check_pass(typename Ops::Point first, const Q& q, Add add) {
    typename Ops::Point acc = first;
    if ((G1CheckParams::Z_ABS >> 62) & 1) add(acc, q);
#pragma unroll 1
    for (int i = 61; i >= 0; i--) {
        Ops::dbl(acc);
        if ((G1CheckParams::Z_ABS >> i) & 1) add(acc, q);  // uniform: the bit pattern is a constant
    }
    return acc;
}

// p finite and on the curve (a lane that is neither still runs this and masks the answer: the operations only need Ops' operand bounds)
template <class Ops>
ZKP_G1CHECK_FN bool g1_in_subgroup(const typename Ops::Affine& p) {
    typedef typename Ops::Point Point;
    typedef typename Ops::Affine Affine;
    const Point q = g1_check_pass<Ops>(Ops::dbl_affine(p), p, [](Point& a, const Affine& b) { Ops::madd(a, b); });  // [|z|]P
    Point d = q;
    Ops::dbl(d);
    Point acc = g1_check_pass<Ops>(d, q, [](Point& a, const Point& b) { Ops::add(a, b); });                        // [z^2]P
    Ops::madd(acc, Ops::neg(p));
    Ops::madd(acc, Ops::neg(Ops::phi(p)));
    return Ops::is_inf(acc);
}

#ifndef __HIPCC__
struct G1CheckHost {
    struct Affine {
        host::HFq x, y;
    };
    typedef host::HXyzz Point;
    static host::HFq beta() {
        static const host::HFq b = host::HFq::load(GlvParams::BETA).to_mont();
        return b;
    }
    static Point dbl_affine(const Affine& p) { return Point{p.x, p.y, host::HFq::one(), host::HFq::one()}.dbl(); }
    static void dbl(Point& a) { a = a.dbl(); }
    static void madd(Point& a, const Affine& b) { a = a.madd(b.x, b.y); }
    static void add(Point& a, const Point& b) { a = a.add(b); }
    static Affine neg(const Affine& p) { return Affine{p.x, p.y.neg()}; }
    static Affine phi(const Affine& p) { return Affine{p.x * beta(), p.y}; }
    static bool is_inf(const Point& a) { return a.is_inf(); }
};
#endif

#ifdef __HIPCC__
// Operand bounds (g1_28.hpp): p.x, p.y canonical.  neg: y -> 4p - y (neg4, inside madd's contract); phi: beta x is a product, tight
// (< 2p, limbs < 2^28), which every use of q.x in g1_28_madd allows (a factor of a product, a stored X < 14p, the x of
// g1_28_double_affine).  The accumulator becomes infinite only through the additions (X28::infinity(), exact zeros); doubling leaves
// such an accumulator alone.
struct G1Check28 {
    typedef A28 Affine;
    typedef X28 Point;
    static ZKP_DEV Fq28 beta() {
        Fq28 b;
#pragma unroll
        for (int i = 0; i < NL28; i++) b.l[i] = G1CheckParams::BETA28[i];
        return b;
    }
    static ZKP_DEV X28 dbl_affine(const A28& p) { return g1_28_double_affine(p); }
    static ZKP_DEV void dbl(X28& a) {
        if (!a.is_inf()) a = g1_28_double(a);
    }
    static ZKP_DEV void madd(X28& a, const A28& b) { g1_28_madd(a, b); }
    static ZKP_DEV void add(X28& a, const X28& b) { g1_28_add(a, b); }
    static ZKP_DEV A28 neg(const A28& p) {
        A28 r;
        r.x = p.x;
        r.y = neg4(p.y);
        return r;
    }
    static ZKP_DEV A28 phi(const A28& p) {
        A28 r;
        r.x = p.x * beta();
        r.y = p.y;
        return r;
    }
    static ZKP_DEV bool is_inf(const X28& a) { return a.is_inf(); }
};

// limbs of a canonical internal coordinate: every limb below 2^28, the value below p
ZKP_DEV bool fq28_is_canonical(const Fq28& a) {
    uint32_t hi = 0;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < NL28; i++) {
        hi |= a.l[i];
        c = ((int64_t)a.l[i] - (int64_t)Fq28C::MOD[i] + c) >> 28;  // borrow chain of a - p (limbs < 2^28)
    }
    return (hi >> 28) == 0 && c < 0;
}

// y^2 = x^3 + 4 for canonical x, y: d = y^2 - (x^3 + 4) through sub8 (subtrahend < 6p carried to limbs < 2^28), zero iff d^2 is
ZKP_DEV bool g1_28_on_curve(const A28& p) {
    const Fq28 one = Fq28::one();
    const Fq28 two = one + one;
    const Fq28 rhs = normalise(sqr(p.x) * p.x + (two + two));  // tight + 4 (< 4p, limbs < 2^30): < 6p
    const Fq28 d = sub8(sqr(p.y), rhs);                        // < 10p, limbs < 2^30
    return tight_is_zero_mod_p(sqr(d));
}

// Status of one finite point already in the internal form; a point whose coordinates are no canonical internal residues (it can only
// come from raw limbs >= p) counts as off the curve.  Every lane runs all of the arithmetic, on (0, 0) where its own limbs would
// break the operand bounds.
ZKP_DEV uint32_t g1_28_status(A28 p) {
    const bool canon = fq28_is_canonical(p.x) && fq28_is_canonical(p.y);
    if (!canon) {
        p.x = Fq28::zero();
        p.y = Fq28::zero();
    }
    const bool on = g1_28_on_curve(p);
    const bool sub = g1_in_subgroup<G1Check28>(p);
    return !canon || !on ? (uint32_t)G1_OFF_CURVE : !sub ? (uint32_t)G1_OUTSIDE_SUBGROUP : (uint32_t)G1_VALID;
}

// What the kernels accumulate per call: counts of statuses 1..3 and the smallest (index << 2 | status) of a bad point
struct G1CheckReport {
    unsigned long long count[3];
    unsigned long long first;  // ~0 when nothing is bad
};

// Per wave: three ballots, then lanes 0..2 add their counts and the first bad lane lowers the minimum -- no atomic at all for a wave
// of valid points
ZKP_DEV void g1_check_reduce(uint32_t status, uint64_t index, G1CheckReport* rep) {
    const unsigned long long b1 = __ballot(status == 1), b2 = __ballot(status == 2), b3 = __ballot(status == 3);
    const unsigned long long bad = b1 | b2 | b3;
    if (!bad) return;
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned long long mine = lane == 0 ? b1 : lane == 1 ? b2 : b3;
    if (lane < 3 && mine) atomicAdd(&rep->count[lane], (unsigned long long)__popcll(mine));
    if (lane == __ffsll((long long)bad) - 1) atomicMin(&rep->first, ((unsigned long long)index << 2) | status);
}

// n points in the 96-byte ABI form (Montgomery radix 2^384, saturated limbs), first = the global index of point 0 of this launch.
// The canonical check runs on the raw limbs BEFORE the eight doublings of the conversion (g1_to_internal_kernel): dbl and
// fq28_from_sat take values below p.
__global__ __launch_bounds__(MSM_THREADS) void g1_validate_raw_kernel(const uint4* __restrict__ in, const uint8_t* __restrict__ is_inf,
                                                                     uint64_t n, uint64_t first, uint8_t* __restrict__ status,
                                                                     G1CheckReport* __restrict__ rep) {
    const uint64_t i = (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    const bool live = i < n;
    const bool inf = live && is_inf && is_inf[i];
    G1Affine p;
    p.x = Fq::zero();
    p.y = Fq::zero();
    if (live && !inf) p = G1Affine::load(in + i * 6);
    uint32_t t[12];
    const bool canon = sub_limbs<12>(t, p.x.l, FqParams::MOD) && sub_limbs<12>(t, p.y.l, FqParams::MOD);  // a borrow: below p
    if (!canon) {
        p.x = Fq::zero();
        p.y = Fq::zero();
    }
#pragma unroll 1
    for (int k = 0; k < 8; k++) {
        p.x = dbl(p.x);
        p.y = dbl(p.y);
    }
    A28 q;
    q.x = fq28_from_sat(p.x);
    q.y = fq28_from_sat(p.y);
    uint32_t s = g1_28_status(q);
    s = !live || inf ? (uint32_t)G1_VALID : !canon ? (uint32_t)G1_NON_CANONICAL : s;
    if (live && status) status[i] = (uint8_t)s;
    g1_check_reduce(s, first + i, rep);
}

// n points of a handle (plane 0: 128 bytes each, internal form): checks 2 and 3
__global__ __launch_bounds__(MSM_THREADS) void g1_validate_internal_kernel(const uint4* __restrict__ in, const uint8_t* __restrict__ is_inf,
                                                                          uint64_t n, uint64_t first, uint8_t* __restrict__ status,
                                                                          G1CheckReport* __restrict__ rep) {
    const uint64_t i = (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    const bool live = i < n;
    const bool inf = live && is_inf && is_inf[i];
    A28 q;
    q.x = Fq28::zero();
    q.y = Fq28::zero();
    if (live && !inf) q = A28::load(in + i * 8);
    uint32_t s = g1_28_status(q);
    s = !live || inf ? (uint32_t)G1_VALID : s;
    if (live && status) status[i] = (uint8_t)s;
    g1_check_reduce(s, first + i, rep);
}
#endif  // __HIPCC__

}  // namespace zkp
