// The tower of csrc/pairing_tower.hpp over the host's HFq, driven by commands on standard input (tests/test_pairing_tower_cpu.py
// writes them and compares every answer with tests/model/pairing_fast_model.py word for word).  One command per line, every operand
// as hexadecimal 64-bit words in memory order; one line of words answers each.
//   mul A B | sqr A | line A L | inv A | frob1 A | frob2 A | frob3 A | cyc A | easy A | fexp A     (A, B, L: 72 words; L a line:
//                                                                    its (c0.c0, c0.c1, c1.c1.c0) are read)
//   steps                                       -> the doubling mask of the 68 Miller steps as two words (low, high)
//   miller K {Q(24 words) qinf P(12 words) pinf} x K   -> the Miller value of the K pairs over prepared lines, 72 words
#define ZKP_PAIRING_TOWER_HOST
#include "pairing_tower.hpp"
#include "pairing_host.hpp"

#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

using namespace zkp;
using namespace zkp::host;
typedef tower::HostFqOps H;
typedef tower::Fq12<H> F12;

static bool read_words(std::istringstream& in, uint64_t* w, int n) {
    for (int i = 0; i < n; i++) {
        std::string t;
        if (!(in >> t)) return false;
        w[i] = std::stoull(t, nullptr, 16);
    }
    return true;
}
static void print_f12(const F12& a) {
    uint64_t w[72];
    tower::f12_store(a, w);
    for (int i = 0; i < 72; i++) std::printf("%016llx%c", (unsigned long long)w[i], i == 71 ? '\n' : ' ');
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string op;
        if (!(in >> op)) continue;
        if (op == "steps") {
            uint64_t lo = 0, hi = 0;
            for (int s = 0; s < tower::MILLER_STEPS; s++)
                if (tower::miller_step_is_doubling(s)) (s < 64 ? lo : hi) |= 1ull << (s & 63);
            std::printf("%016llx %016llx\n", (unsigned long long)lo, (unsigned long long)hi);
            continue;
        }
        if (op == "miller") {
            int k = 0;
            in >> k;
            if (k < 1 || k > 8) return 2;
            std::vector<uint64_t> lines((size_t)k * PREPARED_G2_WORDS), pxy((size_t)k * 12);
            std::vector<int> dead(k);
            std::vector<HFq> pxn(k), py(k);
            for (int j = 0; j < k; j++) {
                uint64_t q[24];
                int qinf = 0, pinf = 0;
                if (!read_words(in, q, 24) || !(in >> qinf) || !read_words(in, &pxy[12 * j], 12) || !(in >> pinf)) return 2;
                if (!qinf) prepare_g2_lines(G2Aff::load(q, false), &lines[(size_t)j * PREPARED_G2_WORDS]);
                dead[j] = qinf || pinf;
                pxn[j] = HFq::load(&pxy[12 * j]).neg();
                py[j] = HFq::load(&pxy[12 * j + 6]);
            }
            F12 f = tower::f12_one<H>();
            for (int s = 0; s < tower::MILLER_STEPS; s++)
                tower::miller_step<H>(
                    f, s, k,
                    [&](int j) {
                        const uint64_t* l = &lines[(size_t)j * PREPARED_G2_WORDS + 24 * s];
                        return tower::PreparedLine<H>{{HFq::load(l), HFq::load(l + 6)}, {HFq::load(l + 12), HFq::load(l + 18)}};
                    },
                    [&](int j) { return pxn[j]; }, [&](int j) { return py[j]; }, [&](int j) { return !dead[j]; });
            print_f12(tower::f12_conj(f));
            continue;
        }
        uint64_t a[72], b[72];
        if (!read_words(in, a, 72)) return 2;
        const F12 A = tower::f12_load(a);
        const bool two = op == "mul" || op == "line";
        if (two && !read_words(in, b, 72)) return 2;
        if (op == "mul") print_f12(tower::f12_mul(A, tower::f12_load(b)));
        else if (op == "sqr") print_f12(tower::f12_sqr(A));
        else if (op == "line") {
            const F12 L = tower::f12_load(b);
            print_f12(tower::f12_mul_line(A, L.c0.c0, L.c0.c1, L.c1.c1.c0));
        } else if (op == "inv") print_f12(tower::f12_inverse(A));
        else if (op == "frob1") print_f12(tower::f12_frobenius<H, 1>(A));
        else if (op == "frob2") print_f12(tower::f12_frobenius<H, 2>(A));
        else if (op == "frob3") print_f12(tower::f12_frobenius<H, 3>(A));
        else if (op == "cyc") print_f12(tower::f12_cyclotomic_sqr(A));
        else if (op == "easy") print_f12(tower::final_exp_easy(A));
        else if (op == "fexp") print_f12(tower::final_exp(A));
        else return 2;
    }
    return 0;
}
