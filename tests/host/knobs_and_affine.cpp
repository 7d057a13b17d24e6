// Two host-only pieces of the drivers, g++ alone (tests/test_host_drivers_cpu.py):
//   batch_to_affine (csrc/host_ff.hpp) byte for byte against HXyzz::to_affine of every point, with infinity first, in the middle and
//   last and one finite point twice;
//   the knob readers (csrc/knobs.hpp) against the readers they replaced -- msm_env_int, the bare getenv flag and the clamped atoi,
//   kept below word for word -- and against the values written down from those, for a knob that is unset, in range, below, above
//   and not a number.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "host_ff.hpp"
#include "knobs.hpp"
using namespace zkp;
using namespace zkp::host;

static int bad = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            bad++;                        \
            printf("FAILED: " __VA_ARGS__); \
            printf("\n");                 \
        }                                 \
    } while (0)

// ---- batch_to_affine ----------------------------------------------------------------------------------------------------------
static void affine_case(const char* name, const std::vector<HXyzz>& pts) {
    const size_t count = pts.size();
    std::vector<uint64_t> got(12 * count + 12, 0xAAAAAAAAAAAAAAAAull), want(12 * count + 12, 0xAAAAAAAAAAAAAAAAull);  // one point of guard
    std::vector<uint8_t> got_inf(count + 1, 0xAA), want_inf(count + 1, 0xAA);
    for (size_t i = 0; i < count; i++) pts[i].to_affine(&want[12 * i], &want_inf[i]);
    batch_to_affine(pts.data(), count, got.data(), got_inf.data());
    CHECK(std::memcmp(got.data(), want.data(), 8 * got.size()) == 0, "batch_to_affine %s: coordinates differ from to_affine", name);
    CHECK(std::memcmp(got_inf.data(), want_inf.data(), got_inf.size()) == 0, "batch_to_affine %s: infinity flags differ", name);
    for (size_t i = 0; i < count; i++)
        if (pts[i].is_inf()) {
            bool zero = got_inf[i] == 1;
            for (int k = 0; k < 12; k++) zero = zero && got[12 * i + k] == 0;
            CHECK(zero, "batch_to_affine %s: infinity at %zu is not 96 zero bytes and flag 1", name, i);
        }
}

static void affine_cases() {
    // the BLS12-381 G1 generator (canonical limbs, brought to Montgomery form)
    const uint64_t gx[6] = {0xfb3af00adb22c6bbULL, 0x6c55e83ff97a1aefULL, 0xa14e3a3f171bac58ULL,
                            0xc3688c4f9774b905ULL, 0x2695638c4fa9ac0fULL, 0x17f1d3a73197d794ULL};
    const uint64_t gy[6] = {0x0caa232946c5e7e1ULL, 0xd03cc744a2888ae4ULL, 0x00db18cb2c04b3edULL,
                            0xfcf5e095d5d00af6ULL, 0xa09e30ed741d8ae4ULL, 0x08b3f481e3aaa0f1ULL};
    uint64_t gxy[12];
    HFq::load(gx).to_mont().store(gxy);
    HFq::load(gy).to_mont().store(gxy + 6);
    const HXyzz G = HXyzz::from_affine(gxy, false), O = HXyzz::infinity();
    const uint64_t k1[4] = {1, 0, 0, 0}, k2[4] = {2, 0, 0, 0}, k3[4] = {0x123456789abcdefULL, 0, 0, 0},
                   k4[4] = {0xfedcba9876543210ULL, 0x0f1e2d3c4b5a6978ULL, 0x1122334455667788ULL, 0x0123456789abcdefULL}, k0[4] = {0, 0, 0, 0};
    const HXyzz P1 = G.mul(k1), P2 = G.mul(k2), P3 = G.mul(k3), P4 = G.mul(k4);
    CHECK(!P1.is_inf() && !P2.is_inf() && !P3.is_inf() && !P4.is_inf() && G.mul(k0).is_inf(), "the test points");
    CHECK(!(P3.zzz == HFq::one()) && !(P4.zzz == HFq::one()), "the multiples are expected in projective form");
    affine_case("count 0", {});
    affine_case("count 1, finite", {P3});
    affine_case("count 1, infinity", {O});
    affine_case("count 2, infinity first", {O, P4});
    affine_case("count 2, infinity last", {P3, G.mul(k0)});
    affine_case("count 2, one point twice", {P4, P4});
    affine_case("count 2, both infinite", {O, O});
    affine_case("count 8", {O, P1, P2, O, P2, P3, P4, P3.add(P3.negate())});
    affine_case("count 8, all finite", {P4, P3, P2, P1, P1, P2, P3, P4});
}

// ---- knob readers -------------------------------------------------------------------------------------------------------------
// the readers before knobs.hpp, word for word
static int msm_env_int(const char* name, int lo, int hi, int dflt) {
    const int v = getenv(name) ? atoi(getenv(name)) : dflt;
    return v >= lo && v <= hi ? v : dflt;
}
static bool flag_set(const char* name) { return getenv(name) != nullptr; }
static bool flag_one(const char* name) {
    const char* e = getenv(name);
    return e && e[0] == '1';
}
static unsigned shard_min_log() {
    const char* e = getenv("ZKP_NTT_SHARD_MIN_LOG");
    return e ? (unsigned)std::max(4, atoi(e)) : 24u;
}
static unsigned tw_matrix_max_log() {
    const char* e = getenv("ZKP_NTT_TW_MATRIX_MAX_LOG");
    return e ? (unsigned)std::min(30, std::max(0, atoi(e))) : 24u;
}

static void put(const char* name, const char* value) {  // nullptr: unset
    if (value) setenv(name, value, 1);
    else unsetenv(name);
}
static const char* shown(const char* v) { return v ? v : "(unset)"; }

static void knob_cases() {
    for (int i = 0; i < KNOB_COUNT; i++) {
        const KnobRow& r = kKnobs[i];
        CHECK(std::strncmp(r.name, "ZKP_", 4) == 0 && r.doc && r.doc[0] && r.lo <= r.hi, "row %d (%s) is incomplete", i, r.name);
        if (r.form == KNOB_SET || r.form == KNOB_ONE) CHECK(r.lo == 0 && r.hi == 1 && r.dflt == 0, "row %d (%s): a flag is 0..1, off by default", i, r.name);
        for (int j = 0; j < i; j++) CHECK(std::strcmp(r.name, kKnobs[j].name) != 0, "%s is listed twice", r.name);
        unsetenv(r.name);
    }
    CHECK(kKnobs[KNOB_TEST_TAIL_STARVE].kind == KNOB_TEST_HOOK, "ZKP_TEST_TAIL_STARVE is a test hook");
    for (int i = 0; i < KNOB_COUNT; i++) CHECK((kKnobs[i].kind == KNOB_TEST_HOOK) == (i == KNOB_TEST_TAIL_STARVE), "%s: test hooks", kKnobs[i].name);

    struct IntCase { const char* value; int want; };
    // ZKP_MSM_NCHUNK: 1..4096, default 0
    const IntCase nchunk[] = {{nullptr, 0}, {"512", 512}, {"1", 1}, {"4096", 4096}, {"0", 0}, {"-3", 0}, {"4097", 0}, {"abc", 0}, {"", 0}, {"12abc", 12}};
    for (const IntCase& c : nchunk) {
        put("ZKP_MSM_NCHUNK", c.value);
        const int old = msm_env_int("ZKP_MSM_NCHUNK", 1, 4096, 0);
        CHECK(old == c.want, "msm_env_int ZKP_MSM_NCHUNK=%s: %d, written down %d", shown(c.value), old, c.want);
        CHECK(knob_int(KNOB_MSM_NCHUNK) == c.want, "knob_int ZKP_MSM_NCHUNK=%s: %lld, want %d", shown(c.value), knob_int(KNOB_MSM_NCHUNK), c.want);
    }
    unsetenv("ZKP_MSM_NCHUNK");
    // ZKP_MSM_C: 8..16, the default computed by the caller (16 here)
    const IntCase wbits[] = {{nullptr, 16}, {"12", 12}, {"8", 8}, {"7", 16}, {"17", 16}, {"x", 16}};
    for (const IntCase& c : wbits) {
        put("ZKP_MSM_C", c.value);
        const int old = msm_env_int("ZKP_MSM_C", 8, 16, 16);
        CHECK(old == c.want, "msm_env_int ZKP_MSM_C=%s: %d, written down %d", shown(c.value), old, c.want);
        CHECK(knob_int(KNOB_MSM_C, 16) == c.want, "knob_int ZKP_MSM_C=%s: %lld, want %d", shown(c.value), knob_int(KNOB_MSM_C, 16), c.want);
    }
    unsetenv("ZKP_MSM_C");
    // ZKP_MSM_FEED_FIRST_PCT: 0..90, computed default (25 here): not a number reads as 0, which is in range
    const IntCase pct[] = {{nullptr, 25}, {"40", 40}, {"0", 0}, {"-1", 25}, {"91", 25}, {"abc", 0}};
    for (const IntCase& c : pct) {
        put("ZKP_MSM_FEED_FIRST_PCT", c.value);
        const int old = msm_env_int("ZKP_MSM_FEED_FIRST_PCT", 0, 90, 25);
        CHECK(old == c.want, "msm_env_int ZKP_MSM_FEED_FIRST_PCT=%s: %d, written down %d", shown(c.value), old, c.want);
        CHECK(knob_int(KNOB_MSM_FEED_FIRST_PCT, 25) == c.want, "knob_int ZKP_MSM_FEED_FIRST_PCT=%s: %lld, want %d", shown(c.value),
              knob_int(KNOB_MSM_FEED_FIRST_PCT, 25), c.want);
    }
    unsetenv("ZKP_MSM_FEED_FIRST_PCT");
    // the clamped ones
    const IntCase shard[] = {{nullptr, 24}, {"20", 20}, {"4", 4}, {"2", 4}, {"-7", 4}, {"abc", 4}, {"40", 40}};
    for (const IntCase& c : shard) {
        put("ZKP_NTT_SHARD_MIN_LOG", c.value);
        CHECK((int)shard_min_log() == c.want, "old ZKP_NTT_SHARD_MIN_LOG=%s: %u, written down %d", shown(c.value), shard_min_log(), c.want);
        CHECK(knob_int(KNOB_NTT_SHARD_MIN_LOG) == c.want, "knob_int ZKP_NTT_SHARD_MIN_LOG=%s: %lld, want %d", shown(c.value),
              knob_int(KNOB_NTT_SHARD_MIN_LOG), c.want);
    }
    unsetenv("ZKP_NTT_SHARD_MIN_LOG");
    const IntCase tw[] = {{nullptr, 24}, {"0", 0}, {"26", 26}, {"-1", 0}, {"31", 30}, {"abc", 0}};
    for (const IntCase& c : tw) {
        put("ZKP_NTT_TW_MATRIX_MAX_LOG", c.value);
        CHECK((int)tw_matrix_max_log() == c.want, "old ZKP_NTT_TW_MATRIX_MAX_LOG=%s: %u, written down %d", shown(c.value), tw_matrix_max_log(), c.want);
        CHECK(knob_int(KNOB_NTT_TW_MATRIX_MAX_LOG) == c.want, "knob_int ZKP_NTT_TW_MATRIX_MAX_LOG=%s: %lld, want %d", shown(c.value),
              knob_int(KNOB_NTT_TW_MATRIX_MAX_LOG), c.want);
    }
    unsetenv("ZKP_NTT_TW_MATRIX_MAX_LOG");

    struct FlagCase { const char* value; bool want_set, want_one; };
    const FlagCase flags[] = {{nullptr, false, false}, {"1", true, true}, {"0", true, false}, {"", true, false}, {"yes", true, false}, {"10", true, true}};
    for (const FlagCase& c : flags) {
        put("ZKP_MSM_NO_POLL", c.value);
        put("ZKP_FRI_ZERO_AS_0", c.value);
        CHECK(flag_set("ZKP_MSM_NO_POLL") == c.want_set && flag_one("ZKP_FRI_ZERO_AS_0") == c.want_one, "old flags for %s", shown(c.value));
        CHECK(knob_flag(KNOB_MSM_NO_POLL) == c.want_set, "knob_flag ZKP_MSM_NO_POLL=%s", shown(c.value));
        CHECK(knob_flag(KNOB_FRI_ZERO_AS_0) == c.want_one, "knob_flag ZKP_FRI_ZERO_AS_0=%s", shown(c.value));
    }
    unsetenv("ZKP_MSM_NO_POLL");
    unsetenv("ZKP_FRI_ZERO_AS_0");
    // a knob whose range the caller checks comes through as it is
    put("ZKP_PYR_TAIL_THREADS", "100");
    CHECK(knob_int(KNOB_PYR_TAIL_THREADS) == 100, "ZKP_PYR_TAIL_THREADS=100 reaches the caller's check");
    put("ZKP_PYR_TAIL_THREADS", nullptr);
    CHECK(knob_int(KNOB_PYR_TAIL_THREADS) == 256, "ZKP_PYR_TAIL_THREADS unset");
}

int main() {
    affine_cases();
    knob_cases();
    printf("host drivers: %d failures\n", bad);
    return bad ? 1 : 0;
}
