// g1_ntt_plan.hpp -- the index arithmetic of the transform over G1 POINTS (g1_ntt.hpp, g1_ntt_host.inc): which two points and which
// twiddle a butterfly lane takes, where the SRS points and the coefficients of an opener's call sit in its slices and rows (all
// openings: one of each), where the quotient slice h comes out, how large the workspaces are and how the lanes of a pass are cut into launches.  Plain
// C++17 without HIP, so that tests/host/g1_ntt_plan.cpp checks it with g++ alone; under hipcc (ff.hpp included first) the kernels
// call the same functions.
//
// The transform is a radix-2 decimation in time, in place: the load puts point i at bitrev(i), stage s = 0 .. log_n - 1 joins blocks
// of half = 2^s points, the output is in natural order.  Y_i = sum_j [w^(ij)] P_j with w = omega_n (inverse: omega_n^-1, and n^-1
// folded into the LAST stage: its left operands are the first n / 2 points, which one multiplication pass scales beforehand, and its
// twiddles start from n^-1 instead of 1).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace zkp {

#ifdef ZKP_HD
#define ZKP_G1NTT_FN ZKP_HD
#else
#define ZKP_G1NTT_FN inline
#endif

constexpr unsigned G1_NTT_MAX_LOG = 24;              // zkp_g1_ntt*, zkp_g1_bases_lagrange; an opener transforms 2n points: 23
constexpr uint64_t G1_NTT_LAUNCH = (uint64_t)1 << 18;  // multiplying lanes per launch: no single kernel holds a shared device for long (profiles/g1_ntt.md)
constexpr uint64_t G1_NTT_IO_LAUNCH = (uint64_t)1 << 22;  // lanes per launch of the load and store kernels (one inversion per lane at most), as G1_CHECK_LAUNCH
constexpr unsigned G1_NTT_THREADS = 64;              // workgroup of the multiplying kernels: one wave (they run one wave per SIMD)
constexpr size_t G1_NTT_POINT_BYTES = 256;           // an XYZZ point of g1_28.hpp, plane-major: 16 chunks of 16 B, `capacity` apart
// per (log_n, direction) the kernels read a row of Montgomery Fr constants: w^(2^b) for b < 24, then 1, then n^-1
constexpr unsigned G1_NTT_TW_ONE = 24, G1_NTT_TW_NINV = 25, G1_NTT_TW_ROW = 26;

ZKP_G1NTT_FN uint32_t g1_ntt_bitrev(uint32_t i, unsigned log_n) {
    if (!log_n) return 0;
    i = ((i & 0x55555555u) << 1) | ((i >> 1) & 0x55555555u);
    i = ((i & 0x33333333u) << 2) | ((i >> 2) & 0x33333333u);
    i = ((i & 0x0f0f0f0fu) << 4) | ((i >> 4) & 0x0f0f0f0fu);
    i = ((i & 0x00ff00ffu) << 8) | ((i >> 8) & 0x00ff00ffu);
    i = (i << 16) | (i >> 16);
    return i >> (32 - log_n);
}

// Butterfly `i` (< n / 2) of stage `stage` (< log_n):  (P[lo], P[hi]) <- (P[lo] + [w^exp] P[hi], P[lo] - [w^exp] P[hi]).
// Stages whose blocks are shorter than a wave number their butterflies twiddle-major -- the 64 lanes of a wave then share one
// twiddle, and the waves of twiddle 1 skip the multiplication together -- the others block-major, where neighbouring lanes take
// neighbouring points.  Either way every pair of a stage is taken exactly once and a lane touches its own two points only.
struct G1NttButterfly {
    uint32_t lo, hi, exp;
};
ZKP_G1NTT_FN G1NttButterfly g1_ntt_butterfly(unsigned log_n, unsigned stage, uint32_t i) {
    const unsigned group_log = log_n - 1 - stage;  // 2^group_log blocks of 2 half points
    const uint32_t half = 1u << stage, groups = 1u << group_log;
    const bool twiddle_major = half < 64 && groups >= 64;
    const uint32_t j = twiddle_major ? i >> group_log : i & (half - 1);
    const uint32_t blk = twiddle_major ? i & (groups - 1) : i >> stage;
    G1NttButterfly b;
    b.lo = (blk << (stage + 1)) + j;
    b.hi = b.lo + half;
    b.exp = j << group_log;
    return b;
}

// What a load kernel puts into slot i of a vector of `count` points: source point src0 + step * i for i < finite, the identity
// behind them; the slot is stored at bitrev(i, rev_log) (rev_log = 0: at i).
struct G1NttLoadMap {
    uint64_t count, finite;
    int64_t src0;
    int32_t step;
    uint32_t rev_log;
};
ZKP_G1NTT_FN int64_t g1_ntt_load_source(const G1NttLoadMap& m, uint64_t i) { return i < m.finite ? m.src0 + (int64_t)m.step * (int64_t)i : -1; }
inline G1NttLoadMap g1_ntt_load_plain(unsigned log_n) {
    const uint64_t n = (uint64_t)1 << log_n;
    return G1NttLoadMap{n, n, 0, 1, log_n};
}

// Launches of a pass of `lanes` multiplying lanes: launch k covers [k * G1_NTT_LAUNCH, ...) and is the only one that may be short
inline uint64_t g1_ntt_launches(uint64_t lanes) { return (lanes + G1_NTT_LAUNCH - 1) / G1_NTT_LAUNCH; }
inline uint64_t g1_ntt_launch_lanes(uint64_t lanes, uint64_t k) {
    const uint64_t first = k * G1_NTT_LAUNCH;
    return first >= lanes ? 0 : lanes - first < G1_NTT_LAUNCH ? lanes - first : G1_NTT_LAUNCH;
}

// Bytes of the workspaces.  Every multiplying lane of a launch parks P + phi(P) in its own entry of `table`.
struct G1NttSizes {
    size_t points;  // the vector itself, 2^log_n XYZZ points
    size_t table;   // one entry per lane of the longest launch
    size_t total;
};
inline G1NttSizes g1_ntt_sizes(unsigned log_n, uint64_t mul_lanes) {  // mul_lanes: the longest multiplying pass the caller runs
    G1NttSizes s;
    s.points = G1_NTT_POINT_BYTES << log_n;
    s.table = G1_NTT_POINT_BYTES * (size_t)(mul_lanes < G1_NTT_LAUNCH ? (mul_lanes ? mul_lanes : 1) : G1_NTT_LAUNCH);
    s.total = s.points + s.table;
    return s;
}

// The n / l multi-point proofs of f (len <= n coefficients), one per coset of l = 2^log_l points (include/zkp_hip.h,
// zkp_kzg_open_cosets): r = n / l >= 2 cosets, coset k = {w^(k + j r) : j < l}, the roots of X^l - x_k^l with x_k = w^k; proof k is the
// commitment of the quotient of f by that binomial.  One convolution per slice b < l of the SRS and of f, in vectors of 2r:
//   s^(b)_j = S_{(r-2-j) l + b} for j < r - 1, identity behind;   g^(b)_t = f_{(t+1) l + b} for t < r - 1 and below len, zero behind;
//   U_k = sum_{b<l} [NTT_2r(g^(b))_k] NTT_2r(s^(b))_k for k < 2r;   u = iNTT_2r(U);   h_i = u_{r-2+i} for i < r - 1, h_{r-1} = O;
//   proofs = NTT_r(h), whose root is w^l.
// (u_m = sum_b sum_{j+t=m} [g^(b)_t] s^(b)_j, so h_i = sum_b sum_t [f_{(t+1) l + b}] S_{(t-i) l + b} = sum_c [f_{(i+1) l + c}] S_c: the
// coefficient of x_k^(l i) in the quotient's commitment, q_k = sum_i x_k^(l i) sum_c f_{(i+1) l + c} X^c.)  SRS points S_0 .. S_{n-l-1}
// are read.
// l = 1 is all n openings of f (zkp_kzg_open_all), over SRS points S_0 .. S_{d-1}, d = n - 1 -- one slice, r = n:
//   s_j = S_{d-1-j} for j < d, identity for d <= j < 2n;   g_t = f_{t+1} for t + 1 < len, zero behind;
//   u = iNTT_2n(NTT_2n(s) . NTT_2n(g));   h_i = u_{d-1+i} for i < d, h_d = O;   proofs = NTT_n(h).
// (u_m = sum_{j+t=m} [g_t] s_j, so u_{d-1+i} = sum_t [f_{t+1}] S_{t-i} = sum_k [f_{i+1+k}] S_k; the largest index is 2d - 2 < 2n.)  Proof m
// is the single-point opening at w^m; the sizes are 512n / 512n / 256n / 64n bytes and the table, no partial sums.
constexpr unsigned G1_COSET_MAX_GROUP_LOG = 3;  // a lane of the multiply-accumulate pass sums at most 8 terms
// B = 2^G1_COSET_GROUP_LOG terms share the 128 doublings of one lane.  0 is the per-term multiplication plus the fold; it stays 0
// until profiles/kzg_open_cosets.md holds a measurement in which a larger group wins.
constexpr unsigned G1_COSET_GROUP_LOG = 0;

inline bool g1_coset_shape_ok(unsigned log_n, unsigned log_l) { return log_l < log_n && log_n + 1 <= G1_NTT_MAX_LOG; }
ZKP_G1NTT_FN G1NttLoadMap g1_coset_srs_map(unsigned log_n, unsigned log_l, uint64_t b) {  // slice b < l of the SRS, a vector of 2r
    const uint64_t r = (uint64_t)1 << (log_n - log_l), l = (uint64_t)1 << log_l;
    return G1NttLoadMap{2 * r, r - 1, (int64_t)((r - 2) * l + b), -(int32_t)l, log_n - log_l + 1};
}
ZKP_G1NTT_FN int64_t g1_coset_coeff_source(unsigned log_n, unsigned log_l, uint64_t len, uint64_t b, uint64_t t) {  // slot t of row b of g, -1: zero
    const uint64_t r = (uint64_t)1 << (log_n - log_l), src = ((t + 1) << log_l) + b;
    return t + 1 < r && src < len ? (int64_t)src : -1;
}
inline G1NttLoadMap g1_coset_slice_map(unsigned log_n, unsigned log_l) {  // h out of u, loaded for the transform of r
    const uint64_t r = (uint64_t)1 << (log_n - log_l);
    return G1NttLoadMap{r, r - 1, (int64_t)r - 2, 1, log_n - log_l};
}

// The multiply-accumulate pass: 2r outputs of l terms each.  Group q of output k holds the `terms` slices b = q terms + j, j < terms
// (all l of them where l is below the group size), and belongs to lane q 2r + k -- neighbouring lanes take neighbouring points of a
// slice.  Term j of that lane is element ((q terms + j) 2r + k) of the transformed SRS and of the transformed rows of g.  A launch
// takes at most G1_NTT_LAUNCH terms, for each of them parks P + phi(P) in the table.
struct G1CosetMac {
    uint32_t terms;        // per lane
    uint64_t groups;       // per output: l / terms partial sums
    uint64_t lanes;        // groups * 2r
    uint64_t launch_lanes; // lanes of every launch but the last
};
inline G1CosetMac g1_coset_mac(unsigned log_n, unsigned log_l, unsigned group_log) {
    const unsigned t_log = group_log < log_l ? group_log : log_l;
    G1CosetMac m;
    m.terms = 1u << t_log;
    m.groups = (uint64_t)1 << (log_l - t_log);
    m.lanes = m.groups << (log_n - log_l + 1);
    m.launch_lanes = G1_NTT_LAUNCH >> t_log;
    return m;
}
inline uint64_t g1_coset_mac_launches(const G1CosetMac& m) { return (m.lanes + m.launch_lanes - 1) / m.launch_lanes; }
inline uint64_t g1_coset_mac_launch_lanes(const G1CosetMac& m, uint64_t k) {
    const uint64_t first = k * m.launch_lanes;
    return first >= m.lanes ? 0 : m.lanes - first < m.launch_lanes ? m.lanes - first : m.launch_lanes;
}
ZKP_G1NTT_FN uint64_t g1_coset_mac_element(unsigned log_m, uint32_t terms, uint64_t lane, uint32_t j) {  // log_m: of 2r
    return (((lane >> log_m) * terms + j) << log_m) + (lane & (((uint64_t)1 << log_m) - 1));
}

// The fold of the `groups` partial sums of every output, pairwise: step i halves what is left, partial q += partial q + half for
// q < half, over half * 2r lanes; the last step (half == 1) writes into the vector the stages run on.  No step when groups == 1:
// the multiply-accumulate pass then writes there itself.
struct G1CosetFoldStep {
    uint64_t half, lanes;
    bool last;
};
inline unsigned g1_coset_fold_steps(const G1CosetMac& m) {
    unsigned s = 0;
    while (((uint64_t)1 << s) < m.groups) s++;
    return s;
}
inline G1CosetFoldStep g1_coset_fold_step(unsigned log_n, unsigned log_l, const G1CosetMac& m, unsigned i) {
    G1CosetFoldStep f;
    f.half = m.groups >> (i + 1);
    f.lanes = f.half << (log_n - log_l + 1);
    f.last = f.half == 1;
    return f;
}

// A batch of n_polys polynomials in one call (zkp_kzg_open_cosets_batch): every vector of a call is max_polys times as long and
// polynomial p has what one polynomial has, p times that vector's length further on -- its rows of g at p 2n, its partial sums at
// p lanes1 (lanes1: G1CosetMac.lanes of one polynomial), its u at p 2r, its h at p r -- while the transformed SRS is shared.  Lanes
// per polynomial, 2n, 2r and r are powers of two, so a lane finds its polynomial by a shift; n_polys is any number.  One polynomial
// is the batch of one: p = 0 in everything below.
constexpr uint64_t G1_COSET_MAX_POLYS = 4096;
inline unsigned g1_coset_lanes_log(unsigned log_n, unsigned log_l, unsigned group_log) {  // log2 of lanes1
    return log_n + 1 - (group_log < log_l ? group_log : log_l);
}
// Entries of the lanes' table of an opener for up to max_polys polynomials.  A launch of the multiply-accumulate pass parks one
// entry per TERM, the transforms of u and h one per lane of a grid row: neither may be cut by G1_NTT_LAUNCH alone, since for small n
// the table has fewer entries than that.
inline uint64_t g1_coset_table_entries(unsigned log_n, uint64_t max_polys) {
    const uint64_t terms = max_polys << (log_n + 1);
    return terms < G1_NTT_LAUNCH ? terms : G1_NTT_LAUNCH;
}
// The multiply-accumulate pass of n_polys polynomials: lane L < lanes belongs to polynomial L / lanes1 and is lane L mod lanes1 of
// it.  A launch takes as many lanes as the table of `tcap` entries holds terms for, G1_NTT_LAUNCH terms at most; with tcap of
// g1_coset_table_entries(log_n, 1) and one polynomial these are the launches of g1_coset_mac.
struct G1CosetBatch {
    G1CosetMac one;         // of one polynomial
    unsigned lanes_log;     // log2 one.lanes
    uint64_t n_polys, lanes, launch_lanes;
};
inline G1CosetBatch g1_coset_batch(unsigned log_n, unsigned log_l, unsigned group_log, uint64_t n_polys, uint64_t tcap) {
    G1CosetBatch b;
    b.one = g1_coset_mac(log_n, log_l, group_log);
    b.lanes_log = g1_coset_lanes_log(log_n, log_l, group_log);
    b.n_polys = n_polys;
    b.lanes = n_polys << b.lanes_log;
    b.launch_lanes = (tcap < G1_NTT_LAUNCH ? tcap : G1_NTT_LAUNCH) / b.one.terms;
    return b;
}
inline uint64_t g1_coset_batch_launches(const G1CosetBatch& b) { return b.launch_lanes ? (b.lanes + b.launch_lanes - 1) / b.launch_lanes : 0; }
inline uint64_t g1_coset_batch_launch_lanes(const G1CosetBatch& b, uint64_t k) {
    const uint64_t first = k * b.launch_lanes;
    return first >= b.lanes ? 0 : b.lanes - first < b.launch_lanes ? b.lanes - first : b.launch_lanes;
}
// what the kernels take of a batch: lane L or slot i of a vector of 2^log per polynomial is slot `in` of polynomial p
struct G1CosetOf {
    uint64_t p, in;
};
ZKP_G1NTT_FN G1CosetOf g1_coset_of(unsigned log, uint64_t i) { return G1CosetOf{i >> log, i & (((uint64_t)1 << log) - 1)}; }
// Term j of batch lane L = p lanes1 + i: since lanes1 terms = 2n, g1_coset_mac_element(log_m, terms, L, j) is p 2n + the element of
// lane i of one polynomial -- the term's scalar in the batch's rows of g as it stands.  Its point, in the transformed SRS that all
// polynomials share, is g1_coset_mac_element of lane i = g1_coset_of(lanes_log, L).in, which is that element mod 2n: the kernel
// takes the former (the address of a point then advances with j as it does for one polynomial, and the compiler schedules the
// loads of a point as it did: profiles/kzg_open_cosets_batch.md), tests/host/g1_coset_batch_plan.cpp pins the two against each other
ZKP_G1NTT_FN uint64_t g1_coset_batch_srs(unsigned log_n, uint64_t e) { return e & (((uint64_t)2 << log_n) - 1); }
// output k < 2r of polynomial p in the batch's u, where the stages expect it
ZKP_G1NTT_FN uint64_t g1_coset_batch_u(unsigned log_m, uint64_t p, uint64_t k) { return (p << log_m) + g1_ntt_bitrev((uint32_t)k, log_m); }
// slot t of g of polynomial p: where its coefficient sits in rows `stride` scalars apart, -1: zero
ZKP_G1NTT_FN int64_t g1_coset_batch_coeff_source(unsigned log_n, unsigned log_l, uint64_t len, uint64_t stride, uint64_t p, uint64_t t) {
    const unsigned log_m = log_n - log_l + 1;
    const int64_t s = g1_coset_coeff_source(log_n, log_l, len, t >> log_m, t & (((uint64_t)1 << log_m) - 1));
    return s < 0 ? s : (int64_t)(p * stride) + s;
}
// Lane j < n_polys f.lanes of fold step f (f.lanes = 2^step_log per polynomial): partial `lo` += partial `lo + f.lanes`, both inside
// polynomial p's lanes1 partial sums; the last step writes to g1_coset_batch_u(log_m, p, in)
struct G1CosetFoldLane {
    uint64_t p, in, lo, hi;
};
ZKP_G1NTT_FN G1CosetFoldLane g1_coset_fold_lane(unsigned lanes_log, unsigned step_log, uint64_t j) {
    const G1CosetOf o = g1_coset_of(step_log, j);
    G1CosetFoldLane f;
    f.p = o.p;
    f.in = o.in;
    f.lo = (o.p << lanes_log) + o.in;
    f.hi = f.lo + ((uint64_t)1 << step_log);
    return f;
}
inline unsigned g1_coset_fold_step_log(unsigned log_n, unsigned log_l, const G1CosetMac& m, unsigned i) {  // log2 of g1_coset_fold_step(..).lanes
    unsigned g = 0;
    while (((uint64_t)1 << g) < m.groups) g++;
    return g - (i + 1) + (log_n - log_l + 1);
}
// Slot i < n_polys r of the batch's h (all polynomials contiguous, r apart, each bit-reversed for its transform of r): its source in
// the batch's u, -1: the identity
struct G1CosetSlice {
    int64_t src;
    uint64_t dst;
};
ZKP_G1NTT_FN G1CosetSlice g1_coset_batch_slice(const G1NttLoadMap& map, unsigned log_m, uint64_t i) {  // map: g1_coset_slice_map, count = 2^rev_log
    const G1CosetOf o = g1_coset_of(map.rev_log, i);
    const int64_t s = g1_ntt_load_source(map, o.in);
    G1CosetSlice c;
    c.src = s < 0 ? s : (int64_t)(o.p << log_m) + s;
    c.dst = (o.p << map.rev_log) + g1_ntt_bitrev((uint32_t)o.in, map.rev_log);
    return c;
}

// Per polynomial of a batch: 256 B x lanes1 of partial sums (where there is a fold; 512 n at the committed group size), 768 r of u and
// h, 64 n of scalars.
struct G1CosetSizes {
    size_t srs_hat, partial, work, slice, scalars, table, total;  // the l transformed slices (kept); the partial sums, u, h, g, the lanes' table
};
inline G1CosetSizes g1_coset_sizes(unsigned log_n, unsigned log_l, unsigned group_log, uint64_t max_polys = 1) {
    const uint64_t n = (uint64_t)1 << log_n, r = n >> log_l;
    const G1CosetMac m = g1_coset_mac(log_n, log_l, group_log);
    G1CosetSizes s;
    s.srs_hat = G1_NTT_POINT_BYTES * 2 * n;
    s.partial = m.groups > 1 ? G1_NTT_POINT_BYTES * m.lanes * max_polys : 0;
    s.work = G1_NTT_POINT_BYTES * 2 * r * max_polys;
    s.slice = G1_NTT_POINT_BYTES * r * max_polys;
    s.scalars = 32 * 2 * n * max_polys;
    s.table = G1_NTT_POINT_BYTES * g1_coset_table_entries(log_n, max_polys);  // one entry per term of the longest launch; the stages need fewer
    s.total = s.srs_hat + s.partial + s.work + s.slice + s.scalars + s.table;
    return s;
}

}  // namespace zkp
