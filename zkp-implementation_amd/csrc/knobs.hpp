// knobs.hpp -- every environment knob the library reads: one table, one reader for integers, one for flags.  The only getenv of
// csrc/.  Plain C++17 without HIP (msm_plan.hpp includes it; tests/host/ builds it with g++ alone).  A knob is named by its
// enumerator, so one that is not in the table does not compile.  Every knob is read on every call that uses it: none is frozen at
// first use, and the order of calls never decides whether a knob is honoured.
#pragma once
#include <climits>
#include <cstdlib>

namespace zkp {

enum Knob {
    // read by plan_msm / plan_reduce / msm_feed_ranges (msm_plan.hpp): the rows before KNOB_MSM_PLAN_END
    KNOB_MSM_C, KNOB_MSM_FEED_RANGES, KNOB_MSM_FEED_FIRST_PCT, KNOB_MSM_FEED_SECOND_PCT, KNOB_MSM_RANGE_LOG, KNOB_MSM_FIRST_PCT,
    KNOB_MSM_NCHUNK, KNOB_SORT_LO_BITS, KNOB_MSM_NO_OVERLAP, KNOB_MSM_SPLIT_LOG, KNOB_FOLD_LANE_MIN, KNOB_PYR_TAIL_THREADS,
    KNOB_PYR_TAIL_BLOCKS, KNOB_PYR_TAIL_HALF,
    KNOB_MSM_PLAN_END,
    KNOB_TEST_TAIL_STARVE = KNOB_MSM_PLAN_END, KNOB_MSM_NO_POLL, KNOB_POOL_NO_WARM, KNOB_MSM_BALANCE_FROM, KNOB_SRS_EXPAND_MAX_BYTES, KNOB_NTT_TW_MATRIX_MAX_LOG,
    KNOB_NTT_NO_WIDE_PASS, KNOB_NTT_SHARD_MIN_LOG, KNOB_PLONK_NO_POLL, KNOB_FRI_ZERO_AS_0, KNOB_FRI_FR_TAIL_LOG,
    KNOB_KZG_COSET_GROUP_LOG, KNOB_KZG_OPENER_MAX_BYTES, KNOB_KZG_RECOVER_LEAF_LOG, KNOB_KZG_RECOVER_MAX_BYTES,
    KNOB_KZG_CELLS_CHUNK_LOG,
    KNOB_KZG_EVALS_INVERSE, KNOB_KZG_EVALS_MAX_BYTES,
    KNOB_PAIRING_FINAL_EXP,
    KNOB_COUNT
};

enum KnobKind { KNOB_TUNING, KNOB_POLICY, KNOB_TEST_HOOK };  // a measuring aid; part of what a caller may rely on; for the test suite only
enum KnobForm {
    KNOB_INT,         // atoi-style integer in [lo, hi]; outside: the default
    KNOB_INT_CLAMP,   // the same; outside: the nearer bound
    KNOB_INT_REFUSE,  // the same; outside: the caller refuses the call with ZKP_E_ARG and its own message (the reader hands the value on)
    KNOB_SET,         // flag: on when the variable exists, whatever it holds
    KNOB_ONE,         // flag: on when the value begins with '1'
    KNOB_WORD         // a choice between words: knob_is(k, word) is true when the value is exactly that word; anything else is the default
};
constexpr long long KNOB_COMPUTED = LLONG_MIN;  // the default depends on the problem: the caller passes it to knob_int

struct KnobRow {
    Knob id;
    const char* name;
    KnobKind kind;
    KnobForm form;
    long long lo, hi, dflt;  // (flags: 0, 1, 0)
    const char* doc;
};

constexpr KnobRow kKnobs[KNOB_COUNT] = {
    {KNOB_MSM_C, "ZKP_MSM_C", KNOB_TUNING, KNOB_INT, 8, 16, KNOB_COMPUTED,
     "window bits of an MSM over unexpanded bases (16 from 2048 terms, else 8): profiles/r01_window_sweep.txt"},
    {KNOB_MSM_FEED_RANGES, "ZKP_MSM_FEED_RANGES", KNOB_TUNING, KNOB_INT, 1, 64, 0,
     "host-fed scalars in this many equal ranges (0: the unequal split): profiles/r04_i_host_scalars_unequal_ranges.md"},
    {KNOB_MSM_FEED_FIRST_PCT, "ZKP_MSM_FEED_FIRST_PCT", KNOB_TUNING, KNOB_INT, 0, 90, KNOB_COMPUTED,
     "share of the first host-fed range (25, from 2^21 terms 10; 0: equal ranges): profiles/r04_i_host_scalars_unequal_ranges.md"},
    {KNOB_MSM_FEED_SECOND_PCT, "ZKP_MSM_FEED_SECOND_PCT", KNOB_TUNING, KNOB_INT, 0, 80, KNOB_COMPUTED,
     "share of a second short host-fed range (30 from 2^21 terms, else none): profiles/r05_o_range_handover.md"},
    {KNOB_MSM_RANGE_LOG, "ZKP_MSM_RANGE_LOG", KNOB_TUNING, KNOB_INT, 10, 30, 0,
     "scalar ranges of at most 2^v terms in shared-bucket mode (0: 2^24, or 2^23 above 12 insertions per scalar): "
     "profiles/r02_a_accumulate_prefetch_and_range_sweep.md"},
    {KNOB_MSM_FIRST_PCT, "ZKP_MSM_FIRST_PCT", KNOB_TUNING, KNOB_INT, 1, 90, 0,
     "resident scalars, single MSM: a short first range of this share (0: none): profiles/r05_o_range_handover.md"},
    {KNOB_MSM_NCHUNK, "ZKP_MSM_NCHUNK", KNOB_TUNING, KNOB_INT, 1, 4096, 0, "chunks per bucket set of the counting sort (0: 512 over the bucket sets)"},
    {KNOB_SORT_LO_BITS, "ZKP_SORT_LO_BITS", KNOB_TUNING, KNOB_INT, 6, 10, 0,
     "bins of the sort's second pass, 2^v (0: 8..10 by window width): profiles/r04_m_sort_tiles.md"},
    {KNOB_MSM_NO_OVERLAP, "ZKP_MSM_NO_OVERLAP", KNOB_TUNING, KNOB_SET, 0, 1, 0,
     "sort of range r+1 after, not under, the accumulate of range r: profiles/r02_j_sort_under_accumulate.md"},
    {KNOB_MSM_SPLIT_LOG, "ZKP_MSM_SPLIT_LOG", KNOB_TUNING, KNOB_INT, 0, 2, KNOB_COMPUTED,
     "2^v lanes (quads) share a bucket's run in a single-range MSM (default: by bucket count): profiles/r02_n_split_runs.md"},
    {KNOB_FOLD_LANE_MIN, "ZKP_FOLD_LANE_MIN", KNOB_TUNING, KNOB_INT, 0, LLONG_MAX, 1ll << 15,
     "adds in one fold launch from which one lane per add is used: profiles/r05_m_fold_lane.md"},
    {KNOB_PYR_TAIL_THREADS, "ZKP_PYR_TAIL_THREADS", KNOB_TUNING, KNOB_INT_REFUSE, 64, 512, 256,
     "workgroup size of the bucket reduction's last-levels launch, a multiple of 64: profiles/r04_e_bucket_reduce_counters.md"},
    {KNOB_PYR_TAIL_BLOCKS, "ZKP_PYR_TAIL_BLOCKS", KNOB_TUNING, KNOB_INT_REFUSE, 1, 256, 16,
     "workgroups per bucket set of that launch: profiles/r04_e_bucket_reduce_counters.md"},
    {KNOB_PYR_TAIL_HALF, "ZKP_PYR_TAIL_HALF", KNOB_TUNING, KNOB_INT_REFUSE, 1, UINT_MAX, 64,
     "pairs per array from which that launch takes over: profiles/r04_e_bucket_reduce_counters.md"},
    {KNOB_TEST_TAIL_STARVE, "ZKP_TEST_TAIL_STARVE", KNOB_TEST_HOOK, KNOB_SET, 0, 1, 0,
     "every MSM FAILS: the last-levels barrier waits for a workgroup that does not exist (tests/test_gpu_parity.py)"},
    {KNOB_MSM_NO_POLL, "ZKP_MSM_NO_POLL", KNOB_TUNING, KNOB_SET, 0, 1, 0,
     "stream wait instead of polling the MSM's result flags: profiles/r05_k_result_flag_polling.md"},
    {KNOB_POOL_NO_WARM, "ZKP_POOL_NO_WARM", KNOB_TUNING, KNOB_SET, 0, 1, 0,
     "do not wake the host pool before a batch's tails: profiles/r05_q_host_pool_warm.md"},
    {KNOB_MSM_BALANCE_FROM, "ZKP_MSM_BALANCE_FROM", KNOB_TUNING, KNOB_INT, 0, INT_MAX, 1,
     "expansion: slices of floor/ceil(256 / planes) bits from this many bits of overshoot: profiles/r03_j_balanced_slices.md"},
    {KNOB_SRS_EXPAND_MAX_BYTES, "ZKP_SRS_EXPAND_MAX_BYTES", KNOB_POLICY, KNOB_INT, 0, LLONG_MAX, LLONG_MAX,
     "an SRS expansion larger than this is refused with ZKP_E_NOMEM; the bases stay unexpanded"},
    {KNOB_NTT_TW_MATRIX_MAX_LOG, "ZKP_NTT_TW_MATRIX_MAX_LOG", KNOB_TUNING, KNOB_INT_CLAMP, 0, 30, 24,
     "largest transform whose pass-0 twiddles are kept as a matrix: profiles/r02_m_ntt_twiddle_matrix.md"},
    {KNOB_NTT_NO_WIDE_PASS, "ZKP_NTT_NO_WIDE_PASS", KNOB_TUNING, KNOB_SET, 0, 1, 0,
     "no radix-2^9 / 2^10 passes in transform plans built from now on (a plan is cached per size): profiles/r02_l_ntt_wide_pass.md"},
    {KNOB_NTT_SHARD_MIN_LOG, "ZKP_NTT_SHARD_MIN_LOG", KNOB_POLICY, KNOB_INT_CLAMP, 4, INT_MAX, 24,
     "host transforms from 2^v elements are spread over the device slots"},
    {KNOB_PLONK_NO_POLL, "ZKP_PLONK_NO_POLL", KNOB_TUNING, KNOB_SET, 0, 1, 0,
     "stream wait instead of the polled sequence number behind a proof's read-backs: profiles/r05_q_host_pool_warm.md"},
    {KNOB_FRI_ZERO_AS_0, "ZKP_FRI_ZERO_AS_0", KNOB_POLICY, KNOB_ONE, 0, 1, 0,
     "1: a zero field element enters hashes and the transcript as \"0\" instead of the empty string"},
    {KNOB_FRI_FR_TAIL_LOG, "ZKP_FRI_FR_TAIL_LOG", KNOB_TUNING, KNOB_INT_CLAMP, 0, 10, 9,
     "FRI over Fr: layers of up to 2^v points run in the tail kernel (0: none)"},
    {KNOB_KZG_COSET_GROUP_LOG, "ZKP_KZG_COSET_GROUP_LOG", KNOB_TUNING, KNOB_INT, 0, 3, KNOB_COMPUTED,
     "openers created from now on sum 2^v terms per lane of the multiply-accumulate pass (default: G1_COSET_GROUP_LOG; an opener of "
     "all n points, log_l = 0, has one term per lane whatever v): profiles/kzg_open_cosets.md"},
    {KNOB_KZG_OPENER_MAX_BYTES, "ZKP_KZG_OPENER_MAX_BYTES", KNOB_POLICY, KNOB_INT, 0, LLONG_MAX, LLONG_MAX,
     "an opener (zkp_kzg_opener_create*, any log_l) whose slices and workspaces are larger than this is refused with ZKP_E_NOMEM "
     "before anything is allocated"},
    {KNOB_KZG_RECOVER_LEAF_LOG, "ZKP_KZG_RECOVER_LEAF_LOG", KNOB_TUNING, KNOB_INT, 1, 8, KNOB_COMPUTED,
     "recoverers created from now on multiply 2^v factors of the vanishing polynomial per leaf workgroup before the transform levels "
     "take over (default: KZG_RECOVER_LEAF_LOG): profiles/kzg_recover.md"},
    {KNOB_KZG_RECOVER_MAX_BYTES, "ZKP_KZG_RECOVER_MAX_BYTES", KNOB_POLICY, KNOB_INT, 0, LLONG_MAX, LLONG_MAX,
     "a recoverer (zkp_kzg_recoverer_create) whose device workspace is larger than this is refused with ZKP_E_NOMEM before anything "
     "is allocated"},
    {KNOB_KZG_CELLS_CHUNK_LOG, "ZKP_KZG_CELLS_CHUNK_LOG", KNOB_TUNING, KNOB_INT, 0, 16, KNOB_COMPUTED,
     "cell verifiers created from now on sum at most 2^v cells of a coset (weights of a commitment) per lane before the sums of the "
     "chunks are combined (default: KZG_CELLS_CHUNK_LOG): profiles/kzg_verify_cells.md"},
    {KNOB_KZG_EVALS_INVERSE, "ZKP_KZG_EVALS_INVERSE", KNOB_TUNING, KNOB_INT, 0, 1, KNOB_COMPUTED,
     "the one inversion per workgroup of zkp_kzg_open_evals_*: 0 division steps (fr_inv.hpp), 1 the Fermat power (default: "
     "KZG_EVALS_INVERSE): profiles/kzg_open_evals.md"},
    {KNOB_KZG_EVALS_MAX_BYTES, "ZKP_KZG_EVALS_MAX_BYTES", KNOB_POLICY, KNOB_INT, 0, LLONG_MAX, LLONG_MAX,
     "an evaluation-form opener (zkp_kzg_eval_opener_create) whose device workspace is larger than this is refused with ZKP_E_NOMEM "
     "before anything is allocated"},
    {KNOB_PAIRING_FINAL_EXP, "ZKP_PAIRING_FINAL_EXP", KNOB_TUNING, KNOB_WORD, 0, 1, 0,
     "the final exponentiation of the host pairing check every verifier ends in: chain (default) the x-chain of pairing_tower.hpp, "
     "plain the one 4314-bit power; the verdicts are the same, zkp_pairing's value is always the plain one: profiles/pairing_dev.md"},
};

constexpr bool knob_rows_in_enum_order() {
    for (int i = 0; i < KNOB_COUNT; i++)
        if (kKnobs[i].id != i) return false;
    return true;
}
static_assert(knob_rows_in_enum_order(), "kKnobs: one row per enumerator, in the enum's order");

// An integer knob, `dflt` when it is unset (the caller's, for a KNOB_COMPUTED row).  Not a number reads as 0, as atoi has it.
inline long long knob_int(Knob k, long long dflt) {
    const KnobRow& r = kKnobs[k];
    const char* e = getenv(r.name);
    if (!e) return dflt;
    const long long v = strtoll(e, nullptr, 10);
    if (r.form == KNOB_INT_REFUSE || (v >= r.lo && v <= r.hi)) return v;
    return r.form == KNOB_INT_CLAMP ? (v < r.lo ? r.lo : r.hi) : dflt;
}
inline long long knob_int(Knob k) { return knob_int(k, kKnobs[k].dflt); }

// A KNOB_WORD knob: set to exactly `word`
inline bool knob_is(Knob k, const char* word) {
    const char* e = getenv(kKnobs[k].name);
    if (!e) return false;
    while (*e && *e == *word) e++, word++;
    return *e == 0 && *word == 0;
}

inline bool knob_flag(Knob k) {
    const char* e = getenv(kKnobs[k].name);
    return e && (kKnobs[k].form == KNOB_SET || e[0] == '1');
}

}  // namespace zkp
