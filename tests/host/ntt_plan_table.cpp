// plan_ntt / pass0_uses_matrix / plan_ntt_axis0 / four_step_exponent_ok (csrc/ntt_plan.hpp) against tests/golden/ntt_plans.txt (its
// header says where the table comes from), plus the invariants every plan keeps.  g++ only:
// tests/test_ntt_plan_cpu.py.
//   ntt_plan_table <table>   one line per case: "<inputs> -> <expected shape>"; prints the cases that differ
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>

#include "ntt_plan.hpp"
using namespace zkp;

static std::string fmt(const char* f, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0, unsigned long long d = 0,
                       unsigned long long e = 0, unsigned long long g = 0, unsigned long long h = 0, unsigned long long i = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, f, a, b, c, d, e, g, h, i);
    return buf;
}

static std::string show(const NttShape& s, bool matrix) {
    std::string out = fmt("passes=%llu r=%llu,%llu,%llu,%llu h=%llu nlo=%llu nhi=%llu", s.passes, s.r[0], s.r[1], s.r[2], s.r[3], s.h, s.nlo, s.nhi) +
                      fmt(" lo_ninv=%llu", s.lo_ninv);
    for (int p = 0; p + 1 < s.passes; p++) {
        const NttStridedShape& t = s.strided[p];
        out += fmt(" p%llu=%llu,%llu,%llu,%llu,%llu,%llu", p, t.log_outer, t.inner, t.log_t, t.lds, t.tiles, t.direct_len);
    }
    const auto& l = s.last;
    return out + fmt(" matrix=%llu last=%llu,%llu,%llu,%llu,%llu,%llu,%llu", matrix, l.log_r, l.log_r0, l.log_m, l.log_r1, l.t_log, l.stride, l.lds) +
           fmt(",%llu", l.tiles);
}

// what run_ntt relies on, whatever the knobs
static const char* broken(const NttShape& s) {
    const uint64_t n = 1ull << s.log_n;
    int sum = 0;
    for (int p = 0; p < 4; p++) sum += s.r[p];
    if (s.passes < 1 || s.passes > 4 || sum != (int)s.log_n) return "the radices do not sum to log_n";
    for (int p = 0; p + 1 < s.passes; p++) {
        const NttStridedShape& t = s.strided[p];
        if (t.lds > 160 * 1024) return "a strided pass needs more than 160 KiB of LDS";
        if (((t.tiles << t.log_t) << t.log_r) != n || (t.inner << (t.log_outer + t.log_r)) != n) return "strided tiles do not cover n";
    }
    if (s.last.lds > 160 * 1024) return "the last pass needs more than 160 KiB of LDS";
    if (((s.last.tiles << s.last.log_r) << s.last.t_log) != n) return "last-pass tiles do not cover n";
    return nullptr;
}

static std::string show(const NttAxis0Shape& s) {
    if (s.error) return std::string("refused: ") + s.error;
    std::string out = fmt("P=%llu r=%llu,%llu col_bits=%llu", s.passes, s.pass[0].log_r, s.pass[1].log_r, s.col_bits);
    for (int p = 0; p < s.passes; p++)
        out += fmt(" pass=%llu,%llu,%llu,%llu,%llu", s.pass[p].log_r, s.pass[p].inner, p + 1 == s.passes ? 1ull << s.pass[p].log_outer : 0, s.pass[p].lds, s.pass[p].tiles);
    return out;
}

int main(int argc, char** argv) {
    std::ifstream in(argc > 1 ? argv[1] : "tests/golden/ntt_plans.txt");
    int cases = 0, bad = 0;
    std::string line;
    while (std::getline(in, line)) {
        if (line.empty() || line[0] == '#') continue;
        const size_t arrow = line.find(" -> ");
        char f[8] = {0};
        unsigned a = 0, wide = 0, inv = 0, nowide = 0, mmax = 0;
        unsigned long long x = 0, y = 0;
        std::string got;
        const char* why = nullptr;
        if (arrow == std::string::npos) {
            printf("unreadable line: %s\n", line.c_str());
            return 2;
        }
        const bool fr = line.find("f=fr ") != std::string::npos;
        if (sscanf(line.c_str(), "ntt f=%7s log_n=%u wide=%u inv=%u nowide=%u mmax=%u", f, &a, &wide, &inv, &nowide, &mmax) == 6) {
            const NttShape s = fr ? plan_ntt<NttFrConsts>(a, (int)inv, wide != 0, nowide != 0) : plan_ntt<NttGlConsts>(a, (int)inv, wide != 0, nowide != 0);
            got = show(s, fr ? pass0_uses_matrix<NttFrConsts>(a, s.passes, mmax) : pass0_uses_matrix<NttGlConsts>(a, s.passes, mmax));
            why = broken(s);
        } else if (sscanf(line.c_str(), "axis0 f=%7s log_len=%u cols=%llu", f, &a, &x) == 3) {
            got = show(fr ? plan_ntt_axis0<NttFrConsts>(a, (size_t)x) : plan_ntt_axis0<NttGlConsts>(a, (size_t)x));
        } else if (sscanf(line.c_str(), "twrow tw_log_n=%u row0=%llu batch=%llu log_n=%u", &a, &x, &y, &mmax) == 4 ||
                   sscanf(line.c_str(), "twcol tw_log_n=%u col0=%llu cols=%llu log_len=%u", &a, &x, &y, &mmax) == 4) {
            got = four_step_exponent_ok(a, x, y, mmax) ? "1" : "0";
        } else {
            printf("unreadable line: %s\n", line.c_str());
            return 2;
        }
        const std::string want = line.substr(arrow + 4);
        cases++;
        if (got != want || why) {
            bad++;
            printf("%s\n  got  %s\n  want %s\n  %s\n", line.substr(0, arrow).c_str(), got.c_str(), want.c_str(), why ? why : "");
        }
    }
    printf("ntt plans: %d cases, %d failures\n", cases, bad);
    return bad || cases == 0 ? 1 : 0;
}
