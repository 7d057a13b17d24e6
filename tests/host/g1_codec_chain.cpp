// The square-root chain and the sign rule of csrc/g1_codec.hpp on the host, g++ only: tests/test_g1_codec_cpu.py.
// g1_codec_lift_x<G1CodecHost> (y = (x^3 + 4)^((p + 1) / 4) by the 2-bit window, then the choice between y and p - y) over HFq on the
// x of the generator, the curve points of small x outside G1 (0, 4, 5, 6), the non-residues 1, 2, 3, 7, p - 1, and 300 pseudo-random
// x, each with the s flag clear and set.  Every case is printed with its x, flag, verdict and y, so that the Python side can recompute
// the line with big integers.  Also a program to run under -fsanitize=address,undefined.
#include <cstdio>
#include <random>
#include <string>

#include "g1_codec.hpp"
using namespace zkp;
using namespace zkp::host;

static void print_hex(const HFq& v) {
    for (int i = 5; i >= 0; i--) printf("%016llx", (unsigned long long)v.l[i]);
}

static int cases = 0;
static void run(const std::string& name, const HFq& x_canonical) {
    for (int s = 0; s < 2; s++) {
        HFq root;
        bool negate = false;
        const bool on = g1_codec_lift_x<G1CodecHost>(x_canonical.to_mont(), s != 0, &root, &negate);
        const HFq y = negate ? G1CodecHost::neg(root) : root;
        printf("case %s x=", name.c_str());
        print_hex(x_canonical);
        printf(" s=%d on=%d y=", s, on ? 1 : 0);
        print_hex(on ? y.from_mont() : HFq::zero());
        printf("\n");
        cases++;
    }
}

int main() {
    static const uint64_t gx[6] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL,
                                   0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL};
    run("G", HFq::load(gx));
    for (uint64_t x : {0, 4, 5, 6, 1, 2, 3, 7}) {
        HFq v = HFq::zero();
        v.l[0] = x;
        run("x" + std::to_string(x), v);
    }
    HFq pm1 = HFq::load(FqTag::ctx().p);
    pm1.l[0] -= 1;
    run("p-1", pm1);
    std::mt19937_64 rng(0x61c6);
    for (int i = 0; i < 300; i++) {
        HFq v;
        for (int k = 0; k < 6; k++) v.l[k] = rng();
        v.l[5] &= 0x0fffffffffffffffULL;  // below 2^380, so below p
        run("rand" + std::to_string(i), v);
    }
    printf("g1_codec: %d cases\n", cases);
    return 0;
}
