// fr_inv.hpp -- modular inverse of an Fr element without an exponentiation: fq28_inv.hpp restated for the 255-bit modulus r.
// Bernstein-Yang "safegcd" division steps (https://gcd.cr.yp.to/papers.html#safegcd), delta = 1 variant, on signed 30-bit limbs;
// the 30 steps on the low words are divsteps_30 of fq28_inv.hpp itself.  Every lane runs the same instruction stream, so 64 lanes
// invert 64 different elements in lockstep; the only branch is wave-uniform (all lanes finished early).
//
// Bound: with f = r odd and 0 <= g < r < 2^255, gcd(f, g) is reached after at most floor((49 * 255 + 57) / 17) = 738 division
// steps (Bernstein-Yang, Theorem 11.2, delta = 1 variant, d = 255) <= 25 x 30 = 750.
//
// Limbs: nine limbs of 30 bits (270 bits) hold f, g and d, e in (-2r, r): r < 2^255, so 2r < 2^256 leaves the top limb, which
// carries the sign, fourteen spare bits.  Each round applies a 2x2 matrix with |u| + |v| <= 2^30, |q| + |r| <= 2^30 to limbs below
// 2^30: a column sum of three products and a carry stays below 2^62 (tests/model/fr_safegcd_model.py range-checks every 32- and
// 64-bit quantity on edge inputs and on inputs chosen to need many rounds).
//
// Cost against the Fermat power fr_inverse (plonk.hpp: 255 squarings and ~125 products, one dependency chain): 25 rounds of 30
// branch-free steps and two 9-limb matrix applications; measured in profiles/kzg_open_evals.md.
#pragma once
#include "ff.hpp"
#include "fr29.hpp"
#include "fq28_inv.hpp"  // divsteps_30, M30

namespace zkp {

constexpr int FR_NL30 = 9;
constexpr int FR_INV_ROUNDS = 25;

struct Fr30C {  // tests/test_fr_safegcd_model.py checks these against the modulus
    // r in 9 limbs of 30 bits
    static constexpr int32_t MOD[9] = {0x00000001, 0x3ffffffc, 0x3fe5bfef, 0x2f6900bf, 0x21d80553, 0x27602026, 0x17d48333, 0x29d4ca67,
                                       0x000073ed};
    static constexpr uint32_t MOD_INV30 = 0x00000001u;  // r^-1 mod 2^30
    // 2^(3 * 256) mod r as 32-bit words: mont_mul(x^-1, R^3) = (a R)^-1 R^3 R^-1 = a^-1 R for the Montgomery residue x = a R
    static constexpr uint32_t R3[8] = {0x439b73afu, 0xc62c1807u, 0x8cf06990u, 0x1b3e0d18u, 0xc7b5f418u, 0x73d13c71u, 0xc8db33e9u, 0x6e2a5bb9u};
};

struct S30r {
    int32_t v[FR_NL30];  // value = sum v[i] 2^(30 i); limbs 0..7 in [0, 2^30), the top limb carries the sign
};

// (f, g) <- t (f, g) / 2^30 (exact)
ZKP_DEV void fr_update_fg_30(S30r& f, S30r& g, int32_t u, int32_t v, int32_t q, int32_t r) {
    int64_t cf = (int64_t)u * f.v[0] + (int64_t)v * g.v[0];
    int64_t cg = (int64_t)q * f.v[0] + (int64_t)r * g.v[0];
    cf >>= 30;
    cg >>= 30;
#pragma unroll
    for (int i = 1; i < FR_NL30; i++) {
        const int32_t fi = f.v[i], gi = g.v[i];
        cf += (int64_t)u * fi + (int64_t)v * gi;
        cg += (int64_t)q * fi + (int64_t)r * gi;
        f.v[i - 1] = (int32_t)cf & M30;
        g.v[i - 1] = (int32_t)cg & M30;
        cf >>= 30;
        cg >>= 30;
    }
    f.v[FR_NL30 - 1] = (int32_t)cf;
    g.v[FR_NL30 - 1] = (int32_t)cg;
}

// (d, e) <- t (d, e) / 2^30 mod r, both kept in (-2r, r)
ZKP_DEV void fr_update_de_30(S30r& d, S30r& e, int32_t u, int32_t v, int32_t q, int32_t r) {
    const int32_t sd = d.v[FR_NL30 - 1] >> 31, se = e.v[FR_NL30 - 1] >> 31;
    int32_t md = (u & sd) + (v & se), me = (q & sd) + (r & se);
    int64_t cd = (int64_t)u * d.v[0] + (int64_t)v * e.v[0];
    int64_t ce = (int64_t)q * d.v[0] + (int64_t)r * e.v[0];
    md -= (int32_t)((Fr30C::MOD_INV30 * (uint32_t)cd + (uint32_t)md) & (uint32_t)M30);
    me -= (int32_t)((Fr30C::MOD_INV30 * (uint32_t)ce + (uint32_t)me) & (uint32_t)M30);
    cd += (int64_t)Fr30C::MOD[0] * md;
    ce += (int64_t)Fr30C::MOD[0] * me;
    cd >>= 30;
    ce >>= 30;
#pragma unroll
    for (int i = 1; i < FR_NL30; i++) {
        const int32_t di = d.v[i], ei = e.v[i];
        cd += (int64_t)u * di + (int64_t)v * ei + (int64_t)Fr30C::MOD[i] * md;
        ce += (int64_t)q * di + (int64_t)r * ei + (int64_t)Fr30C::MOD[i] * me;
        d.v[i - 1] = (int32_t)cd & M30;
        e.v[i - 1] = (int32_t)ce & M30;
        cd >>= 30;
        ce >>= 30;
    }
    d.v[FR_NL30 - 1] = (int32_t)cd;
    e.v[FR_NL30 - 1] = (int32_t)ce;
}

// x in (-2r, r) -> [0, r), negated first when `negate` (f ended at -1)
ZKP_DEV void fr_normalize_30(S30r& x, int32_t negate) {
    int32_t cond_add = x.v[FR_NL30 - 1] >> 31;
#pragma unroll
    for (int i = 0; i < FR_NL30; i++) x.v[i] += Fr30C::MOD[i] & cond_add;
    const int32_t cn = negate ? -1 : 0;
#pragma unroll
    for (int i = 0; i < FR_NL30; i++) x.v[i] = (x.v[i] ^ cn) - cn;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < FR_NL30 - 1; i++) {
        x.v[i] += c;
        c = x.v[i] >> 30;
        x.v[i] &= M30;
    }
    x.v[FR_NL30 - 1] += c;
    cond_add = x.v[FR_NL30 - 1] >> 31;
#pragma unroll
    for (int i = 0; i < FR_NL30; i++) x.v[i] += Fr30C::MOD[i] & cond_add;
    c = 0;
#pragma unroll
    for (int i = 0; i < FR_NL30 - 1; i++) {
        x.v[i] += c;
        c = x.v[i] >> 30;
        x.v[i] &= M30;
    }
    x.v[FR_NL30 - 1] += c;
}

// g in [0, 2r) -> [0, r): one conditional subtraction, so that every multiple of r takes the "0 -> 0" path (for g = r the division
// steps would end with f = r and d = 1)
ZKP_DEV void fr_s30_reduce_once(S30r& g) {
    S30r t;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < FR_NL30; i++) {
        t.v[i] = g.v[i] - Fr30C::MOD[i] + c;
        if (i < FR_NL30 - 1) {
            c = t.v[i] >> 30;  // arithmetic: -1 on a borrow
            t.v[i] &= M30;
        }
    }
    const int32_t keep = t.v[FR_NL30 - 1] >> 31;  // all ones: g < r
#pragma unroll
    for (int i = 0; i < FR_NL30; i++) g.v[i] = (g.v[i] & keep) | (t.v[i] & ~keep);
}

// g^-1 mod r as an integer in [0, r) for 0 <= g < 2r (0 and r -> 0)
ZKP_DEV S30r fr_s30_modinv(S30r g) {
    fr_s30_reduce_once(g);
    S30r f, d, e;
#pragma unroll
    for (int i = 0; i < FR_NL30; i++) {
        f.v[i] = Fr30C::MOD[i];
        d.v[i] = 0;
        e.v[i] = i == 0 ? 1 : 0;
    }
    int32_t eta = -1;
#pragma unroll 1
    for (int it = 0; it < FR_INV_ROUNDS; it++) {
        int32_t u, v, q, r;
        eta = divsteps_30(eta, (uint32_t)f.v[0], (uint32_t)g.v[0], u, v, q, r);
        fr_update_de_30(d, e, u, v, q, r);
        fr_update_fg_30(f, g, u, v, q, r);
        int32_t nz = 0;
#pragma unroll
        for (int i = 0; i < FR_NL30; i++) nz |= g.v[i];
        if (!__any(nz != 0)) break;  // wave-uniform: every lane has reached g = 0
    }
    // f = +-gcd = +-1 (or +-r for g = 0 mod r, where d = 0): d = +-1/g
    fr_normalize_30(d, f.v[FR_NL30 - 1] >> 31);
    return d;
}

// 1 / a for the memory form (8 x 32-bit words, Montgomery radix 2^256): any value below 2r in, the canonical a^-1 R out; 0 and r -> 0
ZKP_DEV Fr fr_inverse_gcd(const Fr& a) {
    S30r g;
#pragma unroll
    for (int i = 0; i < FR_NL30; i++) {
        const int bit = 30 * i, w = bit >> 5, sh = bit & 31;
        uint64_t v = (uint64_t)a.l[w];
        if (w + 1 < 8) v |= (uint64_t)a.l[w + 1] << 32;
        g.v[i] = (int32_t)((uint32_t)(v >> sh) & (uint32_t)M30);
    }
    const S30r d = fr_s30_modinv(g);
    Fr y, r3;
#pragma unroll
    for (int w = 0; w < 8; w++) {
        const int bit = 32 * w, lo = bit / 30, sh = bit % 30;
        uint64_t v = (uint64_t)(uint32_t)d.v[lo] >> sh;
        if (lo + 1 < FR_NL30) v |= (uint64_t)(uint32_t)d.v[lo + 1] << (30 - sh);
        if (lo + 2 < FR_NL30) v |= (uint64_t)(uint32_t)d.v[lo + 2] << (60 - sh);
        y.l[w] = (uint32_t)v;
        r3.l[w] = Fr30C::R3[w];
    }
    return y * r3;  // (a R)^-1 R^3 R^-1 = a^-1 R
}

}  // namespace zkp
