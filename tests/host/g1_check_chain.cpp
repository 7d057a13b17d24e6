// The subgroup test of csrc/g1_check.hpp on the host, g++ only: tests/test_g1_validate_cpu.py.
// g1_in_subgroup<G1CheckHost> ([z^2]P = P + phi(P) over HXyzz) on points that must pass -- G, -G, 2^k G, 200 pseudo-random multiples of
// G, [h]Q for a curve point Q outside G1 -- and on points that must not: the ten curve points with the smallest x, the points (0, 2) and
// (0, p - 2) of order 3, G + (0, 2), and [r]Q (of order dividing the cofactor h).  Every case is printed with its coordinates and
// verdict, so that the Python side can recompute the verdict with big integers; then the counts.
// Also a program to run under -fsanitize=address,undefined.
#include <cstdio>
#include <random>
#include <string>
#include <vector>

#include "g1_check.hpp"
using namespace zkp;
using namespace zkp::host;

typedef G1CheckHost::Affine Aff;

static Aff g1_generator() {
    static const uint64_t gx[6] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL,
                                   0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL};
    static const uint64_t gy[6] = {0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL,
                                   0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    return Aff{HFq::load(gx).to_mont(), HFq::load(gy).to_mont()};
}
static HXyzz lift(const Aff& a) { return HXyzz{a.x, a.y, HFq::one(), HFq::one()}; }
static Aff affine(const HXyzz& p) {  // p finite
    uint64_t xy[12];
    uint8_t inf = 0;
    p.to_affine(xy, &inf);
    return Aff{HFq::load(xy), HFq::load(xy + 6)};
}
static bool on_curve(const Aff& a) { return a.y.sqr() == a.x.sqr() * a.x + HFq::from_u64(4); }

// the curve point with this x and y = (x^3 + 4)^((p + 1) / 4), if x^3 + 4 is a square
static bool lift_x(uint64_t x, Aff* out) {
    const Mont<6>& m = FqTag::ctx();
    uint64_t e[6], one[6] = {1};
    Mont<6>::add(e, m.p, one);  // p + 1 (no carry: the modulus leaves the top bits clear)
    for (int i = 0; i < 6; i++) e[i] = (e[i] >> 2) | (i < 5 ? e[i + 1] << 62 : 0);
    const HFq fx = HFq::from_u64(x), rhs = fx.sqr() * fx + HFq::from_u64(4);
    const HFq y = rhs.pow(e, 6);
    *out = Aff{fx, y};
    return y.sqr() == rhs;
}

static int cases = 0, failures = 0;
static void run(const std::string& name, const Aff& a, bool expect) {
    const bool got = on_curve(a) && g1_in_subgroup<G1CheckHost>(a);
    const HFq x = a.x.from_mont(), y = a.y.from_mont();
    printf("case %s x=", name.c_str());
    for (int i = 5; i >= 0; i--) printf("%016llx", (unsigned long long)x.l[i]);
    printf(" y=");
    for (int i = 5; i >= 0; i--) printf("%016llx", (unsigned long long)y.l[i]);
    printf(" in_g1=%d\n", got ? 1 : 0);
    cases++;
    if (got != expect) {
        failures++;
        printf("WRONG %s: expected %d\n", name.c_str(), expect ? 1 : 0);
    }
}

int main() {
    const Aff g = g1_generator();
    run("G", g, true);
    run("-G", G1CheckHost::neg(g), true);
    HXyzz pw = lift(g);
    for (int k = 1; k <= 16; k++) {
        pw = pw.dbl();
        run("2^" + std::to_string(k) + "G", affine(pw), true);
    }
    std::mt19937_64 rng(0x61c5);
    for (int i = 0; i < 200; i++) {
        const uint64_t k[4] = {rng(), rng(), rng(), rng() >> 1};  // not reduced mod r: HXyzz::mul walks the bits it is given
        run("rand" + std::to_string(i), affine(lift(g).mul(k)), true);
    }
    std::vector<Aff> small;
    for (uint64_t x = 0; small.size() < 10; x++) {
        Aff a;
        if (lift_x(x, &a)) small.push_back(a);
    }
    for (size_t i = 0; i < small.size(); i++) run("small" + std::to_string(i), small[i], false);
    const Aff t3{HFq::zero(), HFq::from_u64(2)};
    run("(0,2)", t3, false);
    run("(0,p-2)", G1CheckHost::neg(t3), false);
    run("G+(0,2)", affine(lift(g).add(lift(t3))), false);
    const Aff q = small[1];  // x = 4
    run("[r]Q", affine(lift(q).mul(FrTag::ctx().p)), false);
    // h = (z - 1)^2 / 3 = 0x396c8c005555e1568c00aaab0000aaab
    const uint64_t h[4] = {0x8c00aaab0000aaabULL, 0x396c8c005555e156ULL, 0, 0};
    run("[h]Q", affine(lift(q).mul(h)), true);
    printf("g1_check: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
