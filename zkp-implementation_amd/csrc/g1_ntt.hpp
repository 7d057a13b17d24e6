// g1_ntt.hpp -- the transform over G1 POINTS, Y_i = sum_j [w^(ij)] P_j, and the variable-base scalar multiplication under it
// (zkp_g1_ntt*, zkp_g1_scale_dev, zkp_g1_bases_lagrange, zkp_kzg_open_all: include/zkp_hip.h; driver: g1_ntt_host.inc; every index:
// g1_ntt_plan.hpp).
//
// Between the load and the store a vector lives in the workspace as XYZZ points on 28-bit limbs (g1_28.hpp) in the plane-major
// layout of the bucket arrays: chunk q of point e at ws[q * capacity + e].  The kernels:
//   g1_ntt_load_kernel<RAW>   96-byte ABI points or the 128-byte points of a handle -> the workspace, bit-reversed when asked
//   g1_ntt_butterfly_kernel   one lane per butterfly of a stage: (a, b) <- (a + [w]b, a - [w]b)
//   g1_ntt_mul_kernel         one lane per point, in place: P_i <- [k_i] P_i (zkp_g1_scale_dev, the n^-1 of an inverse)
//   g1_ntt_slice_kernel       a run of points of u per polynomial of a batch into its h, identities behind it
//   g1_ntt_store_kernel<RAW>  the workspace -> affine, one safegcd inversion per lane
// and for the openers (zkp_kzg_open_cosets and, as its l = 1 case, zkp_kzg_open_all), at the end of this file:
//   g1_ntt_load_slices_kernel the points of a handle -> the l slices of an opener, each bit-reversed
//   g1_ntt_gather_kernel      the strided coefficients -> the l rows of scalars
//   g1_ntt_split_kernel       every transformed scalar, times (2r)^-1, -> its two endomorphism halves
//   g1_ntt_mac_kernel         one lane per output and group of terms: sum_j [k_j] P_j by one joint double-and-add
//   g1_ntt_fold_kernel        the groups' partial sums of an output, pairwise
//
// [k]P for a variable P (g1_28_mul_glv): k = k1 + lambda k2 (glv_split, both halves below 2^128), then ONE joint MSB-first
// double-and-add over {P, phi(P), P + phi(P)}: 128 doublings and ~96 additions instead of 255 and ~128.  The table does not fit the
// register file next to the accumulator and the temporaries of an addition, so it stays in memory: P is the lane's own operand in the
// workspace (nothing overwrites it before the lane's final store), phi(P) is P with X multiplied by beta when it is loaded, and
// P + phi(P) goes to the lane's entry of a launch-sized table.  That sum is made by the loop's own addition in an iteration of its
// own, so the kernel holds one copy of the addition and one of the doubling.  Every addition is the complete one (g1_28_add): ordinary
// inputs make butterflies add equal and opposite points (a constant vector, a padded one).
//
// Operand bounds: as g1_28.hpp, with one extension -- a negated Y is 8p - Y (sub8), at most 8p with limbs below 2^28 after
// normalise().  Every use of a stored Y in g1_28_add / g1_28_double / xyzz_finish holds for 8p: Y ZZZ is 8 * 2 of the 2520 p^2 a
// product may reach, 2Y < 16p squares to 256, and sub8's constant 8p still dominates it.
// Garbage input (points off the curve, non-canonical limbs) gives garbage output; no index and no trip count depends on the data.
#pragma once
#include "fr29.hpp"
#include "msm.hpp"
#include "g1_check.hpp"  // G1Check28::beta()
#include "g1_ntt_plan.hpp"

namespace zkp {

// tight (< 2p) -> canonical (< p), 28-bit limbs: through the 30-bit form whose conditional subtraction exists (fq28_inv.hpp)
ZKP_DEV S30 s30_canonical(const Fq28& a) {
    S30 g = s30_from_fq28(a);
    s30_reduce_once(g);
    return g;
}
ZKP_DEV Fq28 fq28_canonical(const Fq28& a) { return fq28_from_s30(s30_canonical(a)); }
// canonical integer, 13 x 30 bits -> 12 x 32 bits
ZKP_DEV Fq s30_to_sat(const S30& d) {
    Fq y;
#pragma unroll
    for (int w = 0; w < 12; w++) {
        const int bit = 32 * w, lo = bit / 30, sh = bit % 30;
        uint64_t v = (uint64_t)(uint32_t)d.v[lo] >> sh;
        if (lo + 1 < NL30) v |= (uint64_t)(uint32_t)d.v[lo + 1] << (30 - sh);
        if (lo + 2 < NL30) v |= (uint64_t)(uint32_t)d.v[lo + 2] << (60 - sh);
        y.l[w] = (uint32_t)v;
    }
    return y;
}
// tight internal residue (radix 2^392) -> the ABI's saturated canonical residue (radix 2^384): x 2^392 * 2^384 / 2^392
ZKP_DEV Fq fq28_to_abi(const Fq28& a) { return s30_to_sat(s30_canonical(a * fq28_from_sat(Fq::one()))); }

// [k]P: k canonical (8 words, below r), P finite at p[q * pst]; t[q * tst] is the lane's table entry.  See the head of this file.
ZKP_DEV X28 g1_28_mul_glv(const uint32_t* k, const uint4* p, uint64_t pst, uint4* t, uint64_t tst) {
    const GlvHalves h = glv_split(k);
    uint32_t a0 = h.k1[0], a1 = h.k1[1], a2 = h.k1[2], a3 = h.k1[3];
    uint32_t b0 = h.k2[0], b1 = h.k2[1], b2 = h.k2[2], b3 = h.k2[3];
    const Fq28 beta = G1Check28::beta();
    X28 acc = X28::infinity();
#pragma unroll 1
    for (int i = -1; i < 128; i++) {
        uint32_t sel;
        if (i < 0) {  // the iteration that makes the third table entry: P + phi(P)
            acc = X28::load_s(p, pst);
            sel = 2;
        } else {
            if (!acc.is_inf()) acc = g1_28_double(acc);
            sel = (a3 >> 31) | ((b3 >> 31) << 1);  // bit 127 - i of k1 and of k2; the halves shift left by one bit per iteration
            a3 = (a3 << 1) | (a2 >> 31); a2 = (a2 << 1) | (a1 >> 31); a1 = (a1 << 1) | (a0 >> 31); a0 <<= 1;
            b3 = (b3 << 1) | (b2 >> 31); b2 = (b2 << 1) | (b1 >> 31); b1 = (b1 << 1) | (b0 >> 31); b0 <<= 1;
        }
        if (sel) {
            const bool third = sel == 3;
            X28 q = X28::load_s(third ? t : p, third ? tst : pst);
            if (sel == 2) q.x = q.x * beta;  // phi(X, Y, ZZ, ZZZ) = (beta X, Y, ZZ, ZZZ); 14 * 1 of 2520, tight
            g1_28_add(acc, q);
        }
        if (i < 0) {
            acc.store_s(t, tst);
            acc = X28::infinity();
        }
    }
    return acc;
}

// w = start * prod_{bit b of e} row[b], out of Montgomery form (row: G1_NTT_TW_ROW constants of one size and direction)
ZKP_DEV Fr g1_ntt_twiddle(const Fr* __restrict__ row, uint32_t e, bool scaled) {
    Fr w = row[scaled ? G1_NTT_TW_NINV : G1_NTT_TW_ONE];
#pragma unroll 1
    for (uint32_t b = 0; e; b++, e >>= 1)
        if (e & 1) w = w * row[b];
    return from_mont(w);
}

template <bool RAW>
__global__ __launch_bounds__(MSM_THREADS) void g1_ntt_load_kernel(const uint4* __restrict__ in, const uint8_t* __restrict__ is_inf,
                                                                 G1NttLoadMap map, uint64_t first, uint4* __restrict__ ws,
                                                                 uint64_t cap) {
    const uint64_t i = first + (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;  // slots [first, ...) of the map in this launch
    if (i >= map.count) return;
    const int64_t s = g1_ntt_load_source(map, i);
    X28 p = X28::infinity();
    if (s >= 0 && !(is_inf && is_inf[s])) {
        A28 q;
        if (RAW) {  // as g1_to_internal_kernel: eight modular doublings, then the bits re-sliced
            G1Affine a = G1Affine::load(in + (uint64_t)s * 6);
#pragma unroll 1
            for (int k = 0; k < 8; k++) {
                a.x = dbl(a.x);
                a.y = dbl(a.y);
            }
            q.x = fq28_from_sat(a.x);
            q.y = fq28_from_sat(a.y);
        } else {
            q = A28::load(in + (uint64_t)s * 8);
        }
        p = X28::from_affine(q);
    }
    p.store_s(ws + (map.rev_log ? g1_ntt_bitrev((uint32_t)i, map.rev_log) : i), cap);
}

// lanes [first, first + count) of stage `stage` of a transform of 2^log_n points; scaled: the last stage of an inverse.  Row y of the
// grid runs the same lanes of the y-th of several vectors that lie 2^log_n points apart in one workspace (the slices of a coset
// opener); its table entries follow those of row y - 1.
__global__ __launch_bounds__(G1_NTT_THREADS) void g1_ntt_butterfly_kernel(uint4* ws, uint64_t cap, uint32_t log_n, uint32_t stage,
                                                                          uint32_t first, uint32_t count, const Fr* __restrict__ row,
                                                                          uint32_t scaled, uint4* table, uint64_t tcap) {
    const uint32_t lane = blockIdx.x * G1_NTT_THREADS + threadIdx.x;
    if (lane >= count) return;
    ws += (uint64_t)blockIdx.y << log_n;
    table += (uint64_t)blockIdx.y * count;
    const G1NttButterfly bf = g1_ntt_butterfly(log_n, stage, first + lane);
    uint4* pa = ws + bf.lo;
    uint4* pb = ws + bf.hi;
    const bool b_inf = Fq28::load_s(pb + 8 * cap, cap).all_zero();
    if (!b_inf && (bf.exp != 0 || scaled)) {  // [1]b and [w]O cost nothing
        const Fr w = g1_ntt_twiddle(row, bf.exp, scaled != 0);
        g1_28_mul_glv(w.l, pb, cap, table + lane, tcap).store_s(pb, cap);
    }
    const X28 a = X28::load_s(pa, cap);
    X28 b = X28::load_s(pb, cap);
#pragma unroll 1
    for (int t = 0; t < 2; t++) {  // a + b to the left, a - b to the right: one copy of the addition
        X28 s = a;
        g1_28_add(s, b);
        s.store_s(t ? pb : pa, cap);
        b.y = normalise(sub8(Fq28::zero(), b.y));
    }
}

// P_i <- [k_i] P_i in place for i in [first, first + count): P_i at ws[i], k_i = scalars[i * scalar_step] (Montgomery; step 0: one
// constant)
__global__ __launch_bounds__(G1_NTT_THREADS) void g1_ntt_mul_kernel(uint4* ws, uint64_t cap, const Fr* __restrict__ scalars, uint32_t scalar_step,
                                                                    uint64_t first, uint32_t count, uint4* table, uint64_t tcap) {
    const uint32_t lane = blockIdx.x * G1_NTT_THREADS + threadIdx.x;
    if (lane >= count) return;
    const uint64_t i = first + lane;
    const Fr k = from_mont(scalars[i * scalar_step]);
    const bool p_inf = Fq28::load_s(ws + i + 8 * cap, cap).all_zero();
    X28 r = X28::infinity();
    if (!p_inf && !k.is_zero()) r = g1_28_mul_glv(k.l, ws + i, cap, table + lane, tcap);
    r.store_s(ws + i, cap);
}

// slot i in [first, polys * map.count) of the slices h of a batch <- its source in the batch's u (g1_coset_batch_slice: slot
// i mod r of polynomial i / r), the identity where there is none
__global__ __launch_bounds__(MSM_THREADS) void g1_ntt_slice_kernel(const uint4* __restrict__ src, uint64_t scap, G1NttLoadMap map, uint32_t log_m,
                                                                  uint64_t polys, uint64_t first, uint4* __restrict__ dst, uint64_t dcap) {
    const uint64_t i = first + (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    if (i >= polys * map.count) return;
    const G1CosetSlice c = g1_coset_batch_slice(map, log_m, i);
    uint4* d = dst + c.dst;
#pragma unroll
    for (int q = 0; q < 16; q++) d[q * dcap] = c.src >= 0 ? src[q * scap + (uint64_t)c.src] : make_uint4(0u, 0u, 0u, 0u);
}

// points [first, n) of the workspace to affine (as many as the launch has lanes): RAW the ABI's 96 bytes (zeros for the identity), else a handle's 128 bytes, canonical
template <bool RAW>
__global__ __launch_bounds__(MSM_THREADS) void g1_ntt_store_kernel(const uint4* __restrict__ ws, uint64_t cap, uint64_t first, uint64_t n,
                                                                  uint4* __restrict__ out, uint8_t* __restrict__ out_inf) {
    const uint64_t i = first + (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    if (i >= n) return;
    const X28 p = X28::load_s(ws + i, cap);
    const bool inf = p.is_inf();
    const Fq28 zi3 = fq28_inverse_gcd(p.zzz);  // 0 -> 0
    const Fq28 zi = zi3 * p.zz;                // ZZ / ZZZ = 1 / Z
    const Fq28 x = p.x * (zi * zi), y = p.y * zi3;  // tight
    if (RAW) {
        G1Affine r;
        r.x = fq28_to_abi(x);
        r.y = fq28_to_abi(y);
        if (inf) {
            r.x = Fq::zero();
            r.y = Fq::zero();
        }
        r.store(out + i * 6);
    } else {
        A28 r;
        r.x = inf ? Fq28::zero() : fq28_canonical(x);
        r.y = inf ? Fq28::zero() : fq28_canonical(y);
        r.store(out + i * 8);
    }
    if (out_inf) out_inf[i] = inf ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------------------------- the openers
// (zkp_kzg_open_cosets, zkp_kzg_open_all at l = 1: g1_ntt_plan.hpp has the construction and every index below)

// the l slices of a handle's points (128 bytes each, plane 0 of an expansion) into one workspace of 2n: slot i in [first, ...) is slot
// j = i mod 2r of slice b = i / 2r (g1_coset_srs_map), stored bit-reversed within its slice
__global__ __launch_bounds__(MSM_THREADS) void g1_ntt_load_slices_kernel(const uint4* __restrict__ in, const uint8_t* __restrict__ is_inf,
                                                                        uint32_t log_n, uint32_t log_l, uint64_t first, uint4* __restrict__ ws,
                                                                        uint64_t cap) {
    const uint64_t i = first + (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    if (i >> (log_n + 1)) return;
    const uint32_t log_m = log_n - log_l + 1;
    const uint64_t b = i >> log_m, j = i & (((uint64_t)1 << log_m) - 1);
    const int64_t s = g1_ntt_load_source(g1_coset_srs_map(log_n, log_l, b), j);
    X28 p = X28::infinity();
    if (s >= 0 && !(is_inf && is_inf[s])) p = X28::from_affine(A28::load(in + (uint64_t)s * 8));
    p.store_s(ws + (b << log_m) + g1_ntt_bitrev((uint32_t)j, log_m), cap);
}

// the l rows of g of every polynomial of a batch, 2r slots each, out of the strided coefficients (rows of `len`, `stride` scalars
// apart): slot i of the polys * 2n in [first, ...)
__global__ __launch_bounds__(MSM_THREADS) void g1_ntt_gather_kernel(const Fr* __restrict__ coeffs, uint64_t len, uint64_t stride, uint64_t polys,
                                                                   uint32_t log_n, uint32_t log_l, uint64_t first, Fr* __restrict__ g) {
    const uint64_t i = first + (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    const G1CosetOf o = g1_coset_of(log_n + 1, i);
    if (o.p >= polys) return;
    const int64_t s = g1_coset_batch_coeff_source(log_n, log_l, len, stride, o.p, o.in);
    (s >= 0 ? Fr::load(coeffs + s) : Fr::zero()).store(g + i);
}

// g_i <- the halves of c g_i (glv_split), in place over the 32 bytes of the element: words 0..3 k1, words 4..7 k2
__global__ __launch_bounds__(MSM_THREADS) void g1_ntt_split_kernel(Fr* g, const Fr* __restrict__ factor, uint64_t first, uint64_t count) {
    const uint64_t i = first + (uint64_t)blockIdx.x * MSM_THREADS + threadIdx.x;
    if (i >= count) return;
    const Fr k = from_mont(Fr::load(g + i) * *factor);
    const GlvHalves h = glv_split(k.l);
    Fr o;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        o.l[w] = h.k1[w];
        o.l[4 + w] = h.k2[w];
    }
    o.store(g + i);
}

// Lane `first + lane` of the multiply-accumulate pass: sum_{j < terms} [k_j] P_j over its group (g1_coset_mac_element), by ONE joint
// MSB-first double-and-add -- 128 doublings for the whole group, and per bit and term one complete addition from {P_j, phi(P_j),
// P_j + phi(P_j)} as in g1_28_mul_glv.  halves: what g1_ntt_split_kernel left, 8 words per element.  The lane keeps the current word
// of every half in its column of `words` (indexed by j: registers cannot be), the rest stays in memory; P_j + phi(P_j) goes to entry
// j * count + lane of the table, made by the loop's own addition in step -1.  Terms with a zero scalar or an identity point are
// masked out before the loop.  In a batch (g1_coset_batch) the 2^lanes_log lanes of polynomial p follow those of p - 1: the scalar
// of a term is the element of the batch lane, which lies in p's rows of g, and the point it multiplies the element of the lane within
// its polynomial -- the transformed SRS is the same for every p.  The sum goes to slot bitrev(k, rev_log) of p's u when rev_log is
// given (one group per output), else to dst[first + lane], the partial sums the fold takes.
__global__ __launch_bounds__(G1_NTT_THREADS) void g1_ntt_mac_kernel(const uint4* __restrict__ srs, uint64_t scap, const uint32_t* __restrict__ halves,
                                                                    uint32_t log_m, uint32_t terms, uint32_t lanes_log, uint64_t first,
                                                                    uint32_t count, uint4* dst, uint64_t dcap, uint32_t rev_log, uint4* table,
                                                                    uint64_t tcap) {
    __shared__ uint32_t words[2 << G1_COSET_MAX_GROUP_LOG][G1_NTT_THREADS];
    const uint32_t lane = blockIdx.x * G1_NTT_THREADS + threadIdx.x;
    if (lane >= count) return;
    const uint64_t i = first + lane, in = g1_coset_of(lanes_log, i).in;  // the batch lane (scalars); the lane within its polynomial (points)
    uint32_t live = 0;
#pragma unroll 1
    for (uint32_t j = 0; j < terms; j++) {
        const uint64_t e = g1_coset_mac_element(log_m, terms, i, j);
        const uint4* kk = reinterpret_cast<const uint4*>(halves + 8 * e);
        const uint4 a = kk[0], b = kk[1];
        const bool zero = (a.x | a.y | a.z | a.w | b.x | b.y | b.z | b.w) == 0;
        if (!zero && !Fq28::load_s(srs + g1_coset_mac_element(log_m, terms, in, j) + 8 * scap, scap).all_zero()) live |= 1u << j;
    }
    const Fq28 beta = G1Check28::beta();
    X28 acc = X28::infinity();
#pragma unroll 1
    for (int s = -1; s < 128 && live; s++) {
        if (s >= 0) {
            if (!acc.is_inf()) acc = g1_28_double(acc);
            if ((s & 31) == 0) {  // the next word of every half, most significant first
                const uint32_t w = 3 - (s >> 5);
#pragma unroll 1
                for (uint32_t j = 0; j < terms; j++) {
                    const uint32_t* kk = halves + 8 * g1_coset_mac_element(log_m, terms, i, j);
                    words[2 * j][threadIdx.x] = kk[w];
                    words[2 * j + 1][threadIdx.x] = kk[4 + w];
                }
            }
        }
        const uint32_t bit = 31 - (s & 31);
#pragma unroll 1
        for (uint32_t j = 0; j < terms; j++) {
            if (!((live >> j) & 1)) continue;
            const uint4* p = srs + g1_coset_mac_element(log_m, terms, in, j);
            uint4* t = table + (uint64_t)j * count + lane;
            uint32_t sel = 2;
            if (s < 0) acc = X28::load_s(p, scap);  // the step that makes the third table entry: P + phi(P)
            else sel = ((words[2 * j][threadIdx.x] >> bit) & 1) | (((words[2 * j + 1][threadIdx.x] >> bit) & 1) << 1);
            if (sel) {
                const bool third = sel == 3;
                X28 q = X28::load_s(third ? t : p, third ? tcap : scap);
                if (sel == 2) q.x = q.x * beta;
                g1_28_add(acc, q);
            }
            if (s < 0) {
                acc.store_s(t, tcap);
                acc = X28::infinity();
            }
        }
    }
    acc.store_s(dst + (rev_log ? g1_coset_batch_u(rev_log, g1_coset_of(lanes_log, i).p, in) : i), dcap);
}

// One step of the fold (g1_coset_fold_step, g1_coset_fold_lane): lane j in [first, polys << step_log) adds, within the 2^lanes_log
// partial sums of its polynomial, partial `hi` into partial `lo`; the last step (rev_log given, 2^step_log = 2r) writes the sum to
// its slot of that polynomial's u instead
__global__ __launch_bounds__(G1_NTT_THREADS) void g1_ntt_fold_kernel(uint4* part, uint64_t pcap, uint32_t lanes_log, uint32_t step_log, uint64_t polys,
                                                                     uint64_t first, uint4* dst, uint64_t dcap, uint32_t rev_log) {
    const uint64_t j = first + (uint64_t)blockIdx.x * G1_NTT_THREADS + threadIdx.x;
    const G1CosetFoldLane f = g1_coset_fold_lane(lanes_log, step_log, j);
    if (f.p >= polys) return;
    X28 a = X28::load_s(part + f.lo, pcap);
    const X28 b = X28::load_s(part + f.hi, pcap);
    g1_28_add(a, b);
    if (rev_log) a.store_s(dst + g1_coset_batch_u(rev_log, f.p, f.in), dcap);
    else a.store_s(part + f.lo, pcap);
}

}  // namespace zkp
