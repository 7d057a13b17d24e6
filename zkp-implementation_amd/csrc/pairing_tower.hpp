// pairing_tower.hpp -- the BLS12-381 extension tower with the fast pairing arithmetic, written ONCE as C++17 templates over a base-field
// adapter F: Fq2 / Fq6 / Fq12 products and squarings, the Fq12 inverse, the sparse product by a Miller line, the Frobenius maps
// p, p^2, p^3, Granger-Scott cyclotomic squaring and the x-chain final exponentiation.  Instantiated over the host's HFq (HostFqOps
// below: tested without a GPU by tests/host/pairing_tower.cpp, and the host verifiers' final exponentiation) and over the device's
// saturated Fq (pairing.hpp: the kernels).  Nothing here names HIP: a plain g++ compiles it.
//
// Tower and normalisation are those of pairing_host.hpp and tests/model/pairing_model.py: Fq2 = Fq[u]/(u^2 + 1),
// Fq6 = Fq2[v]/(v^3 - (1 + u)), Fq12 = Fq6[w]/(w^2 - v), arkworks coefficient order.  tests/model/pairing_fast_model.py is the big-int
// model of exactly these algorithms; every function below is compared with it word for word.
//
// THE FINAL EXPONENTIATION HERE IS A CUBE.  final_exp(f) = f^(3 (p^12 - 1) / r): the easy part (p^6 - 1)(p^2 + 1), then the hard part
// lambda_0 + lambda_1 p + lambda_2 p^2 + lambda_3 p^3 = 3 (p^4 - p^2 + 1) / r with lambda_3 = (x - 1)^2, lambda_2 = x lambda_3,
// lambda_1 = x lambda_2 - lambda_3, lambda_0 = x lambda_1 + 3 and x = -0xd201000000010000: five x-powers of 63 cyclotomic squarings
// instead of a 4314-bit exponent.  gcd(3, r) = 1, so final_exp(f) == 1 iff the canonical pairing value is 1 -- every verdict is the
// same -- but the VALUE is the cube of what zkp_pairing returns (pairing_host.hpp keeps the plain exponent: that value is pinned).
//
// The adapter F:  typename F::T;  T zero(), one(), lit(six little-endian u64 words of a Montgomery residue);  T add(a, b), sub(a, b),
// mul(a, b), neg(a), inverse(a) (0 -> 0);  bool is_zero(a), eq(a, b).  Elements are canonical (fully reduced) Montgomery residues of
// radix 2^384, so equal field elements are equal words.
//
// PT_FN marks every function (host: inline; the device build defines it as __device__ inline), PT_NOINLINE the ones that must stay
// calls on the device: an Fq12 is 144 registers there and an inlined Fq12 product is 54 base-field products (pairing.hpp).
#pragma once
#include <stdint.h>

#ifndef PT_FN
#define PT_FN inline
#endif
#ifndef PT_NOINLINE
#define PT_NOINLINE
#endif

namespace zkp {
namespace tower {

constexpr uint64_t X_ABS = 0xd201000000010000ull;  // |x|; the curve parameter x is negative
// The Miller loop as 68 line steps (63 doublings, 5 additions), bits of |x| below the leading one, most significant first; step s
// squares the accumulator first iff it is a doubling
constexpr int MILLER_STEPS = 68;
PT_FN constexpr bool miller_step_is_doubling(int s) {
    // the additions: behind the doublings of the set bits 62, 60, 57, 48 and 16 of |x| (steps 0, 3, 7, 17 and 50)
    return !(s == 1 || s == 4 || s == 8 || s == 18 || s == 51);
}

template <class F>
struct Fq2 {
    typename F::T c0, c1;
};
template <class F>
struct Fq6 {
    Fq2<F> c0, c1, c2;
};
template <class F>
struct Fq12 {
    Fq6<F> c0, c1;
};

// ---- Fq2
template <class F> PT_FN Fq2<F> f2_zero() { return Fq2<F>{F::zero(), F::zero()}; }
template <class F> PT_FN Fq2<F> f2_one() { return Fq2<F>{F::one(), F::zero()}; }
template <class F> PT_FN Fq2<F> f2_add(const Fq2<F>& a, const Fq2<F>& b) { return Fq2<F>{F::add(a.c0, b.c0), F::add(a.c1, b.c1)}; }
template <class F> PT_FN Fq2<F> f2_sub(const Fq2<F>& a, const Fq2<F>& b) { return Fq2<F>{F::sub(a.c0, b.c0), F::sub(a.c1, b.c1)}; }
template <class F> PT_FN Fq2<F> f2_dbl(const Fq2<F>& a) { return f2_add(a, a); }
template <class F> PT_FN Fq2<F> f2_neg(const Fq2<F>& a) { return Fq2<F>{F::neg(a.c0), F::neg(a.c1)}; }
template <class F> PT_FN Fq2<F> f2_conj(const Fq2<F>& a) { return Fq2<F>{a.c0, F::neg(a.c1)}; }
template <class F> PT_FN Fq2<F> f2_mul_xi(const Fq2<F>& a) { return Fq2<F>{F::sub(a.c0, a.c1), F::add(a.c0, a.c1)}; }  // * (1 + u)
template <class F> PT_FN Fq2<F> f2_scale(const Fq2<F>& a, const typename F::T& k) { return Fq2<F>{F::mul(a.c0, k), F::mul(a.c1, k)}; }
template <class F> PT_FN bool f2_eq(const Fq2<F>& a, const Fq2<F>& b) { return F::eq(a.c0, b.c0) && F::eq(a.c1, b.c1); }
// Karatsuba: three base-field products
template <class F>
PT_FN PT_NOINLINE Fq2<F> f2_mul(const Fq2<F>& a, const Fq2<F>& b) {
    const typename F::T v0 = F::mul(a.c0, b.c0), v1 = F::mul(a.c1, b.c1);
    const typename F::T s = F::mul(F::add(a.c0, a.c1), F::add(b.c0, b.c1));
    return Fq2<F>{F::sub(v0, v1), F::sub(F::sub(s, v0), v1)};
}
// complex squaring: two base-field products
template <class F>
PT_FN PT_NOINLINE Fq2<F> f2_sqr(const Fq2<F>& a) {
    const typename F::T t = F::mul(a.c0, a.c1);
    return Fq2<F>{F::mul(F::add(a.c0, a.c1), F::sub(a.c0, a.c1)), F::add(t, t)};
}
template <class F>
PT_FN Fq2<F> f2_inverse(const Fq2<F>& a) {  // 0 -> 0
    const typename F::T n = F::inverse(F::add(F::mul(a.c0, a.c0), F::mul(a.c1, a.c1)));
    return Fq2<F>{F::mul(a.c0, n), F::mul(F::neg(a.c1), n)};
}

// ---- Fq6
template <class F> PT_FN Fq6<F> f6_zero() { return Fq6<F>{f2_zero<F>(), f2_zero<F>(), f2_zero<F>()}; }
template <class F> PT_FN Fq6<F> f6_one() { return Fq6<F>{f2_one<F>(), f2_zero<F>(), f2_zero<F>()}; }
template <class F> PT_FN Fq6<F> f6_add(const Fq6<F>& a, const Fq6<F>& b) { return Fq6<F>{f2_add(a.c0, b.c0), f2_add(a.c1, b.c1), f2_add(a.c2, b.c2)}; }
template <class F> PT_FN Fq6<F> f6_sub(const Fq6<F>& a, const Fq6<F>& b) { return Fq6<F>{f2_sub(a.c0, b.c0), f2_sub(a.c1, b.c1), f2_sub(a.c2, b.c2)}; }
template <class F> PT_FN Fq6<F> f6_neg(const Fq6<F>& a) { return Fq6<F>{f2_neg(a.c0), f2_neg(a.c1), f2_neg(a.c2)}; }
template <class F> PT_FN Fq6<F> f6_mul_v(const Fq6<F>& a) { return Fq6<F>{f2_mul_xi(a.c2), a.c0, a.c1}; }
template <class F> PT_FN bool f6_eq(const Fq6<F>& a, const Fq6<F>& b) { return f2_eq(a.c0, b.c0) && f2_eq(a.c1, b.c1) && f2_eq(a.c2, b.c2); }
// Karatsuba: six Fq2 products
template <class F>
PT_FN PT_NOINLINE Fq6<F> f6_mul(const Fq6<F>& a, const Fq6<F>& b) {
    const Fq2<F> v0 = f2_mul(a.c0, b.c0), v1 = f2_mul(a.c1, b.c1), v2 = f2_mul(a.c2, b.c2);
    const Fq2<F> t0 = f2_sub(f2_sub(f2_mul(f2_add(a.c1, a.c2), f2_add(b.c1, b.c2)), v1), v2);
    const Fq2<F> t1 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c1), f2_add(b.c0, b.c1)), v0), v1);
    const Fq2<F> t2 = f2_sub(f2_sub(f2_mul(f2_add(a.c0, a.c2), f2_add(b.c0, b.c2)), v0), v2);
    return Fq6<F>{f2_add(v0, f2_mul_xi(t0)), f2_add(t1, f2_mul_xi(v2)), f2_add(t2, v1)};
}
// (a0, a1, a2) * (A, B, 0): six Fq2 products
template <class F>
PT_FN PT_NOINLINE Fq6<F> f6_mul_ab(const Fq6<F>& a, const Fq2<F>& A, const Fq2<F>& B) {
    return Fq6<F>{f2_add(f2_mul(a.c0, A), f2_mul_xi(f2_mul(a.c2, B))), f2_add(f2_mul(a.c0, B), f2_mul(a.c1, A)),
                  f2_add(f2_mul(a.c1, B), f2_mul(a.c2, A))};
}
// (a0, a1, a2) * (0, C, 0), C in Fq: six base-field products
template <class F>
PT_FN Fq6<F> f6_mul_c(const Fq6<F>& a, const typename F::T& C) {
    return Fq6<F>{f2_mul_xi(f2_scale(a.c2, C)), f2_scale(a.c0, C), f2_scale(a.c1, C)};
}
template <class F>
PT_FN Fq6<F> f6_inverse(const Fq6<F>& a) {  // 0 -> 0
    const Fq2<F> t0 = f2_sub(f2_sqr(a.c0), f2_mul_xi(f2_mul(a.c1, a.c2)));
    const Fq2<F> t1 = f2_sub(f2_mul_xi(f2_sqr(a.c2)), f2_mul(a.c0, a.c1));
    const Fq2<F> t2 = f2_sub(f2_sqr(a.c1), f2_mul(a.c0, a.c2));
    const Fq2<F> n = f2_add(f2_mul(a.c0, t0), f2_mul_xi(f2_add(f2_mul(a.c2, t1), f2_mul(a.c1, t2))));
    const Fq2<F> ni = f2_inverse(n);
    return Fq6<F>{f2_mul(t0, ni), f2_mul(t1, ni), f2_mul(t2, ni)};
}

// ---- Fq12
template <class F> PT_FN Fq12<F> f12_one() { return Fq12<F>{f6_one<F>(), f6_zero<F>()}; }
template <class F> PT_FN Fq12<F> f12_conj(const Fq12<F>& a) { return Fq12<F>{a.c0, f6_neg(a.c1)}; }
template <class F> PT_FN bool f12_eq(const Fq12<F>& a, const Fq12<F>& b) { return f6_eq(a.c0, b.c0) && f6_eq(a.c1, b.c1); }
template <class F> PT_FN bool f12_is_one(const Fq12<F>& a) { return f12_eq(a, f12_one<F>()); }
// Karatsuba: three Fq6 products (54 base-field products)
template <class F>
PT_FN PT_NOINLINE Fq12<F> f12_mul(const Fq12<F>& a, const Fq12<F>& b) {
    const Fq6<F> v0 = f6_mul(a.c0, b.c0), v1 = f6_mul(a.c1, b.c1);
    const Fq6<F> s = f6_mul(f6_add(a.c0, a.c1), f6_add(b.c0, b.c1));
    return Fq12<F>{f6_add(v0, f6_mul_v(v1)), f6_sub(f6_sub(s, v0), v1)};
}
// complex squaring: two Fq6 products (36 base-field products)
template <class F>
PT_FN PT_NOINLINE Fq12<F> f12_sqr(const Fq12<F>& a) {
    const Fq6<F> t = f6_mul(a.c0, a.c1);
    const Fq6<F> s = f6_mul(f6_add(a.c0, a.c1), f6_add(a.c0, f6_mul_v(a.c1)));
    return Fq12<F>{f6_sub(f6_sub(s, t), f6_mul_v(t)), f6_add(t, t)};
}
// (c0 - c1 w) / (c0^2 - v c1^2): the Fq6 norm, then Fq2, then ONE base-field inversion.  0 -> 0.
template <class F>
PT_FN PT_NOINLINE Fq12<F> f12_inverse(const Fq12<F>& a) {
    const Fq6<F> ni = f6_inverse(f6_sub(f6_mul(a.c0, a.c0), f6_mul_v(f6_mul(a.c1, a.c1))));
    return Fq12<F>{f6_mul(a.c0, ni), f6_neg(f6_mul(a.c1, ni))};
}
// f * ((A, B, 0), (0, C, 0)) with C in Fq: the shape of a Miller line (pairing_host.hpp line_eval).  48 base-field products.
template <class F>
PT_FN PT_NOINLINE Fq12<F> f12_mul_line(const Fq12<F>& f, const Fq2<F>& A, const Fq2<F>& B, const typename F::T& C) {
    return Fq12<F>{f6_add(f6_mul_ab(f.c0, A, B), f6_mul_v(f6_mul_c(f.c1, C))), f6_add(f6_mul_c(f.c0, C), f6_mul_ab(f.c1, A, B))};
}

// ---- Frobenius.  a_(j,i) v^i w^j = a_(j,i) w^(2i+j)  ->  conj^K(a_(j,i)) gamma_(K,2i+j) w^(2i+j),  gamma_(K,m) = xi^(m (p^K - 1) / 6).
// The constants: tools/gen_pairing_consts.py prints this block from tests/model/bigmodel.py; tests/test_pairing_tower_cpu.py checks it.
template <class F, int K, int M>
PT_FN Fq2<F> frobenius_gamma() {
    constexpr int m = M;
    // GENERATED BEGIN (tools/gen_pairing_consts.py)
    if (K == 1 && m == 1) return Fq2<F>{F::lit(0x07089552b319d465ull, 0xc6695f92b50a8313ull, 0x97e83cccd117228full, 0xa35baecab2dc29eeull, 0x1ce393ea5daace4dull, 0x08f2220fb0fb66ebull),
                                        F::lit(0xb2f66aad4ce5d646ull, 0x5842a06bfc497cecull, 0xcf4895d42599d394ull, 0xc11b9cba40a8e8d0ull, 0x2e3813cbe5a0de89ull, 0x110eefda88847fafull)};
    if (K == 1 && m == 2) return Fq2<F>{F::lit(0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull),
                                        F::lit(0xcd03c9e48671f071ull, 0x5dab22461fcda5d2ull, 0x587042afd3851b95ull, 0x8eb60ebe01bacb9eull, 0x03f97d6e83d050d2ull, 0x18f0206554638741ull)};
    if (K == 1 && m == 3) return Fq2<F>{F::lit(0x7bcfa7a25aa30fdaull, 0xdc17dec12a927e7cull, 0x2f088dd86b4ebef1ull, 0xd1ca2087da74d4a7ull, 0x2da2596696cebc1dull, 0x0e2b7eedbbfd87d2ull),
                                        F::lit(0x7bcfa7a25aa30fdaull, 0xdc17dec12a927e7cull, 0x2f088dd86b4ebef1ull, 0xd1ca2087da74d4a7ull, 0x2da2596696cebc1dull, 0x0e2b7eedbbfd87d2ull)};
    if (K == 1 && m == 4) return Fq2<F>{F::lit(0x890dc9e4867545c3ull, 0x2af322533285a5d5ull, 0x50880866309b7e2cull, 0xa20d1b8c7e881024ull, 0x14e4f04fe2db9068ull, 0x14e56d3f1564853aull),
                                        F::lit(0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull)};
    if (K == 1 && m == 5) return Fq2<F>{F::lit(0x82d83cf50dbce43full, 0xa2813e53df9d018full, 0xc6f0caa53c65e181ull, 0x7525cf528d50fe95ull, 0x4a85ed50f4798a6bull, 0x171da0fd6cf8eebdull),
                                        F::lit(0x3726c30af242c66cull, 0x7c2ac1aad1b6fe70ull, 0xa04007fbba4b14a2ull, 0xef517c3266341429ull, 0x0095ba654ed2226bull, 0x02e370eccc86f7ddull)};
    if (K == 2 && m == 1) return Fq2<F>{F::lit(0xecfb361b798dba3aull, 0xc100ddb891865a2cull, 0x0ec08ff1232bda8eull, 0xd5c13cc6f1ca4721ull, 0x47222a47bf7b5c04ull, 0x0110f184e51c5f59ull),
                                        F::lit(0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull)};
    if (K == 2 && m == 2) return Fq2<F>{F::lit(0x30f1361b798a64e8ull, 0xf3b8ddab7ece5a2aull, 0x16a8ca3ac61577f7ull, 0xc26a2ff874fd029bull, 0x3636b76660701c6eull, 0x051ba4ab241b6160ull),
                                        F::lit(0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull)};
    if (K == 2 && m == 3) return Fq2<F>{F::lit(0x43f5fffffffcaaaeull, 0x32b7fff2ed47fffdull, 0x07e83a49a2e99d69ull, 0xeca8f3318332bb7aull, 0xef148d1ea0f4c069ull, 0x040ab3263eff0206ull),
                                        F::lit(0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull)};
    if (K == 2 && m == 4) return Fq2<F>{F::lit(0xcd03c9e48671f071ull, 0x5dab22461fcda5d2ull, 0x587042afd3851b95ull, 0x8eb60ebe01bacb9eull, 0x03f97d6e83d050d2ull, 0x18f0206554638741ull),
                                        F::lit(0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull)};
    if (K == 2 && m == 5) return Fq2<F>{F::lit(0x890dc9e4867545c3ull, 0x2af322533285a5d5ull, 0x50880866309b7e2cull, 0xa20d1b8c7e881024ull, 0x14e4f04fe2db9068ull, 0x14e56d3f1564853aull),
                                        F::lit(0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull)};
    if (K == 3 && m == 1) return Fq2<F>{F::lit(0x3e2f585da55c9ad1ull, 0x4294213d86c18183ull, 0x382844c88b623732ull, 0x92ad2afd19103e18ull, 0x1d794e4fac7cf0b9ull, 0x0bd592fc7d825ec8ull),
                                        F::lit(0x7bcfa7a25aa30fdaull, 0xdc17dec12a927e7cull, 0x2f088dd86b4ebef1ull, 0xd1ca2087da74d4a7ull, 0x2da2596696cebc1dull, 0x0e2b7eedbbfd87d2ull)};
    if (K == 3 && m == 2) return Fq2<F>{F::lit(0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull),
                                        F::lit(0x760900000002fffdull, 0xebf4000bc40c0002ull, 0x5f48985753c758baull, 0x77ce585370525745ull, 0x5c071a97a256ec6dull, 0x15f65ec3fa80e493ull)};
    if (K == 3 && m == 3) return Fq2<F>{F::lit(0x3e2f585da55c9ad1ull, 0x4294213d86c18183ull, 0x382844c88b623732ull, 0x92ad2afd19103e18ull, 0x1d794e4fac7cf0b9ull, 0x0bd592fc7d825ec8ull),
                                        F::lit(0x3e2f585da55c9ad1ull, 0x4294213d86c18183ull, 0x382844c88b623732ull, 0x92ad2afd19103e18ull, 0x1d794e4fac7cf0b9ull, 0x0bd592fc7d825ec8ull)};
    if (K == 3 && m == 4) return Fq2<F>{F::lit(0x43f5fffffffcaaaeull, 0x32b7fff2ed47fffdull, 0x07e83a49a2e99d69ull, 0xeca8f3318332bb7aull, 0xef148d1ea0f4c069ull, 0x040ab3263eff0206ull),
                                        F::lit(0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull, 0x0000000000000000ull)};
    if (K == 3 && m == 5) return Fq2<F>{F::lit(0x7bcfa7a25aa30fdaull, 0xdc17dec12a927e7cull, 0x2f088dd86b4ebef1ull, 0xd1ca2087da74d4a7ull, 0x2da2596696cebc1dull, 0x0e2b7eedbbfd87d2ull),
                                        F::lit(0x3e2f585da55c9ad1ull, 0x4294213d86c18183ull, 0x382844c88b623732ull, 0x92ad2afd19103e18ull, 0x1d794e4fac7cf0b9ull, 0x0bd592fc7d825ec8ull)};
    // GENERATED END
    return f2_one<F>();
}
// conj^K(a) gamma_(K,M); the p^2 constants lie in Fq (two scalings instead of an Fq2 product)
template <class F, int K, int M>
PT_FN Fq2<F> frobenius_coeff(const Fq2<F>& a) {
    const Fq2<F> c = (K & 1) ? f2_conj(a) : a;
    if (M == 0) return c;
    const Fq2<F> g = frobenius_gamma<F, K, M>();
    if (K == 2) return f2_scale(c, g.c0);
    return f2_mul(c, g);
}
template <class F, int K>
PT_FN PT_NOINLINE Fq12<F> f12_frobenius(const Fq12<F>& a) {
    static_assert(K >= 1 && K <= 3, "p, p^2 or p^3");
    return Fq12<F>{Fq6<F>{frobenius_coeff<F, K, 0>(a.c0.c0), frobenius_coeff<F, K, 2>(a.c0.c1), frobenius_coeff<F, K, 4>(a.c0.c2)},
                   Fq6<F>{frobenius_coeff<F, K, 1>(a.c1.c0), frobenius_coeff<F, K, 3>(a.c1.c1), frobenius_coeff<F, K, 5>(a.c1.c2)}};
}

// ---- the cyclotomic subgroup (where an element is after the easy part): Granger-Scott squaring, 18 base-field products
template <class F>
PT_FN void cyclo_sq2(const Fq2<F>& x, const Fq2<F>& y, Fq2<F>& re, Fq2<F>& im) {  // (x + y s)^2, s^2 = xi
    const Fq2<F> xx = f2_sqr(x), yy = f2_sqr(y);
    im = f2_sub(f2_sub(f2_sqr(f2_add(x, y)), xx), yy);
    re = f2_add(xx, f2_mul_xi(yy));
}
template <class F> PT_FN Fq2<F> cyclo_3t_minus_2z(const Fq2<F>& t, const Fq2<F>& z) { return f2_add(f2_dbl(f2_sub(t, z)), t); }
template <class F> PT_FN Fq2<F> cyclo_3t_plus_2z(const Fq2<F>& t, const Fq2<F>& z) { return f2_add(f2_dbl(f2_add(t, z)), t); }
template <class F>
PT_FN PT_NOINLINE Fq12<F> f12_cyclotomic_sqr(const Fq12<F>& a) {
    Fq2<F> t0, t1, t2, t3, t4, t5;
    cyclo_sq2(a.c0.c0, a.c1.c1, t0, t1);
    cyclo_sq2(a.c1.c0, a.c0.c2, t2, t3);
    cyclo_sq2(a.c0.c1, a.c1.c2, t4, t5);
    Fq12<F> r;
    r.c0.c0 = cyclo_3t_minus_2z(t0, a.c0.c0);
    r.c1.c1 = cyclo_3t_plus_2z(t1, a.c1.c1);
    r.c1.c0 = cyclo_3t_plus_2z(f2_mul_xi(t5), a.c1.c0);
    r.c0.c2 = cyclo_3t_minus_2z(t4, a.c0.c2);
    r.c0.c1 = cyclo_3t_minus_2z(t2, a.c0.c1);
    r.c1.c2 = cyclo_3t_plus_2z(t3, a.c1.c2);
    return r;
}
// a^x for a in the cyclotomic subgroup: 63 cyclotomic squarings and 5 products, then the conjugate (x < 0; the inverse there)
template <class F>
PT_FN PT_NOINLINE Fq12<F> f12_exp_x(const Fq12<F>& a) {
    Fq12<F> r = a;
    for (int b = 62; b >= 0; b--) {
        r = f12_cyclotomic_sqr(r);
        if ((X_ABS >> b) & 1) r = f12_mul(r, a);
    }
    return f12_conj(r);
}

// f^((p^6 - 1)(p^2 + 1)); 0 -> 0
template <class F>
PT_FN Fq12<F> final_exp_easy(const Fq12<F>& f) {
    const Fq12<F> t = f12_mul(f12_conj(f), f12_inverse(f));
    return f12_mul(f12_frobenius<F, 2>(t), t);
}
// E(f) = f^(3 (p^12 - 1) / r): see the head of this file
template <class F>
PT_FN Fq12<F> final_exp(const Fq12<F>& f) {
    const Fq12<F> m = final_exp_easy(f);
    Fq12<F> b = m;
    for (int i = 0; i < 2; i++) b = f12_mul(f12_exp_x(b), f12_conj(b));                       // m^((x-1)^2) = m^lambda_3
    const Fq12<F> c = f12_exp_x(b);                                                          // m^lambda_2
    const Fq12<F> d = f12_mul(f12_exp_x(c), f12_conj(b));                                    // m^lambda_1
    const Fq12<F> e = f12_mul(f12_exp_x(d), f12_mul(f12_cyclotomic_sqr(m), m));              // m^lambda_0
    return f12_mul(f12_mul(e, f12_frobenius<F, 1>(d)), f12_mul(f12_frobenius<F, 2>(c), f12_frobenius<F, 3>(b)));
}

// ---- the Miller loop over PREPARED lines.  A G2 point's walk is done once (pairing_host.inc: the affine code of pairing_host.hpp) and
// leaves, per step, the pair (lambda, lambda x_T - y_T); the line at P = (xP, yP) is then ((a, -xP lambda, 0), (0, yP, 0)).
template <class F>
struct PreparedLine {
    Fq2<F> lambda, a;
};
// One step of a check with k pairs: square once (a doubling step), then one sparse product per live pair.
// line(j) gives pair j's prepared line of this step, px_neg(j) = -xP_j, py(j) = yP_j, live(j) false for an identity P_j or Q_j.
template <class F, class Line, class CoordX, class CoordY, class Live>
PT_FN void miller_step(Fq12<F>& f, int step, int k, Line line, CoordX px_neg, CoordY py, Live live) {
    if (miller_step_is_doubling(step)) f = f12_sqr(f);
    for (int j = 0; j < k; j++) {
        if (!live(j)) continue;
        const PreparedLine<F> l = line(j);
        f = f12_mul_line(f, l.a, f2_scale(l.lambda, px_neg(j)), py(j));
    }
}

}  // namespace tower
}  // namespace zkp

// ---- the host instantiation: HFq of host_ff.hpp (included only where that header is)
#ifdef ZKP_PAIRING_TOWER_HOST
#include "host_ff.hpp"
namespace zkp {
namespace tower {
struct HostFqOps {
    typedef host::HFq T;
    static T zero() { return T::zero(); }
    static T one() { return T::one(); }
    static T lit(uint64_t w0, uint64_t w1, uint64_t w2, uint64_t w3, uint64_t w4, uint64_t w5) {
        const uint64_t w[6] = {w0, w1, w2, w3, w4, w5};
        return T::load(w);
    }
    static T add(const T& a, const T& b) { return a + b; }
    static T sub(const T& a, const T& b) { return a - b; }
    static T mul(const T& a, const T& b) { return a * b; }
    static T neg(const T& a) { return a.neg(); }
    static T inverse(const T& a) { return a.inverse(); }
    static bool is_zero(const T& a) { return a.is_zero(); }
    static bool eq(const T& a, const T& b) { return a == b; }
};
// 72 words, arkworks memory order (Fq12::store of pairing_host.hpp)
inline Fq12<HostFqOps> f12_load(const uint64_t* p) {
    Fq12<HostFqOps> r;
    Fq2<HostFqOps>* f[6] = {&r.c0.c0, &r.c0.c1, &r.c0.c2, &r.c1.c0, &r.c1.c1, &r.c1.c2};
    for (int i = 0; i < 6; i++) {
        f[i]->c0 = host::HFq::load(p + 12 * i);
        f[i]->c1 = host::HFq::load(p + 12 * i + 6);
    }
    return r;
}
inline void f12_store(const Fq12<HostFqOps>& a, uint64_t* p) {
    const Fq2<HostFqOps>* f[6] = {&a.c0.c0, &a.c0.c1, &a.c0.c2, &a.c1.c0, &a.c1.c1, &a.c1.c2};
    for (int i = 0; i < 6; i++) {
        f[i]->c0.store(p + 12 * i);
        f[i]->c1.store(p + 12 * i + 6);
    }
}
}  // namespace tower
}  // namespace zkp
#endif
