/*
 * zkp_hip.h -- C ABI of libzkp_hip.so, the MI355X (gfx950) backend for the MSM / NTT hot path of
 * sota-zk-labs/zkp-implementation.
 *
 * The reference has no FFI: the surfaces below are what a Rust `-sys` binding would call from inside the
 * reference's own functions (INTEGRATION.md shows the stubs).  Each entry cites the reference code it replaces
 * (file:line under the reference repository root).
 *
 * Data formats = arkworks 0.4 in-memory forms, so a Rust caller passes `&[Fr]` / coordinates untouched:
 *   Fr          uint64_t[4]   Montgomery residue (R = 2^256), little-endian limbs        kzg/src/types.rs:7
 *   Fq (base)   uint64_t[6]   Montgomery residue (R = 2^384)                             kzg/src/types.rs:6
 *   Goldilocks  uint64_t[1]   Montgomery residue (R = 2^64)                              fri/src/fields/goldilocks.rs:4-8
 *   G1 affine   uint64_t[12]  x || y; the point at infinity is carried in a separate byte (1 = infinity),
 *                             never as magic coordinates                                 kzg/src/types.rs:6
 *
 * Conventions: every function returns ZKP_OK (0) or a negative error code and never aborts or unwinds
 * across the ABI; zkp_last_error() gives a thread-local message.  Host buffers are owned by the caller for the
 * duration of the call.  `*_dev` variants take DEVICE pointers (hipMalloc'd or torch CUDA tensors) and a
 * hipStream_t passed as void* (NULL = the default stream); they enqueue work and return without synchronising
 * unless documented otherwise.  Calls may use different streams: workspaces and cached tables are per slot, and an entry
 * that arrives on another stream than the previous one first waits (on the device, hipStreamWaitEvent) for the work the
 * previous entry enqueued.  There is no CPU implementation of the hot path behind this ABI: if no gfx950 device is
 * usable, zkp_init() fails with ZKP_E_DEVICE and every MSM / NTT / Merkle / prover entry fails the same way.  The entries
 * marked "host" (transcripts, verifiers, pairings) are host code by nature and need no device.
 *
 * Environment (read by the library; none of them changes a result): ZKP_MSM_C (window bits of the per-window MSM over
 * unexpanded bases, 8..16), ZKP_MSM_RANGE_LOG (log2 of the scalar range of one pass of the shared-bucket MSM; default 24 over an SRS expanded into at most 12 planes -- the automatic 22-bit windows -- and 23 over more planes),
 * ZKP_MSM_NCHUNK (chunks of the counting sort), ZKP_SORT_LO_BITS (bins of its second pass, log2), ZKP_MSM_FEED_FIRST_PCT (zkp_msm_g1 uploads host scalars in two ranges, the first one this share of them, default 20; 0 = equal ranges), ZKP_MSM_FEED_RANGES (that many EQUAL ranges instead),
 * ZKP_MSM_SPLIT_LOG (0..2: log2 of the lanes that share a bucket's run in a small single-pass MSM; default: chosen per launch),
 * ZKP_MSM_NO_OVERLAP=1 (digits + sort of the next scalar range on the launch stream instead of a second one), ZKP_NTT_NO_WIDE_PASS=1 (Fr
 * transforms with radix <= 2^8 passes only), ZKP_NTT_TW_MATRIX_MAX_LOG (largest Fr transform whose first-pass twiddles are kept as a
 * 32-byte-per-element matrix, default 24, 0 = never) -- tuning and test aids; ZKP_FRI_ZERO_AS_0=1 prints the field element zero as "0"
 * instead of the empty string in the FRI hash input (the one third-party formatting detail that could not be confirmed offline);
 * ZKP_SRS_EXPAND_MAX_BYTES (zkp_g1_bases_precompute refuses, with ZKP_E_NOMEM and the sizes in zkp_last_error(), an expansion larger
 * than this many bytes -- it is also refused when it exceeds the device's free memory; the handle then stays usable unexpanded),
 * ZKP_MSM_BALANCE_FROM (overshoot in bits from which the slices of an expansion are balanced, default 1 = always; tuning aid),
 * ZKP_PYR_TAIL_THREADS / ZKP_PYR_TAIL_BLOCKS / ZKP_PYR_TAIL_HALF (geometry of the launch that runs the last levels of the bucket reduction:
 * workgroup size 64..512, workgroups per bucket set 1..256, pairs per array from which it takes over; defaults 256 / 16 / 64; tuning aids),
 * ZKP_FRI_FR_TAIL_LOG (0..10: log2 of the largest layer zkp_fri_prove_fr runs in its one-workgroup tail kernel, default 9, 0 = none;
 * tuning aid), ZKP_KZG_COSET_GROUP_LOG (0..3: log2 of the terms one lane of an opener's multiply-accumulate pass sums, read by
 * zkp_kzg_opener_create_cosets, default 0, without effect at log_l = 0; tuning aid), ZKP_KZG_OPENER_MAX_BYTES (zkp_kzg_opener_create
 * and zkp_kzg_opener_create_cosets refuse, with ZKP_E_NOMEM and the sizes in zkp_last_error(), an opener that needs more device
 * memory than this many bytes; default: no limit), ZKP_KZG_RECOVER_LEAF_LOG (1..8: log2 of the factors of the vanishing polynomial
 * a leaf workgroup of a recoverer multiplies, read by zkp_kzg_recoverer_create; tuning aid), ZKP_KZG_RECOVER_MAX_BYTES
 * (zkp_kzg_recoverer_create refuses, with ZKP_E_NOMEM and the sizes in zkp_last_error(), a recoverer whose device workspace is larger
 * than this many bytes; default: no limit), ZKP_KZG_CELLS_CHUNK_LOG (0..16: log2 of the cells of a coset, or weights of a commitment,
 * one lane of a cell verifier sums before the chunk sums are combined, read by zkp_kzg_cell_verifier_create, default 4; tuning aid),
 * ZKP_KZG_EVALS_INVERSE (the one inversion per workgroup of zkp_kzg_open_evals_*: 0 = division steps, 1 = the Fermat power; read by
 * every call; tuning aid), ZKP_KZG_EVALS_MAX_BYTES (zkp_kzg_eval_opener_create refuses, with ZKP_E_NOMEM and the sizes in
 * zkp_last_error(), an opener whose device workspace is larger than this many bytes; default: no limit).
 */
#ifndef ZKP_HIP_H
#define ZKP_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZKP_OK 0
#define ZKP_E_ARG (-1)    /* bad argument (null pointer, log_n out of range, ...) */
#define ZKP_E_NOMEM (-2)  /* host or device allocation failed */
#define ZKP_E_DEVICE (-3) /* no usable gfx950 device / HIP runtime error */
#define ZKP_E_SIZE (-4)   /* more scalars than bases: the reference's assert at kzg/src/scheme.rs:86 */

typedef struct zkp_bases zkp_bases; /* opaque: G1 base points resident in HBM */

/* ---- library ----
 * Device slots.  The library keeps one context (workspaces, cached twiddle tables, a launch stream, one mutex) per device
 * SLOT; entries on different slots run concurrently, entries on one slot are serialised.
 *   zkp_init(device)             one slot on HIP device `device` (-1 = the current HIP device).  Idempotent.  This is also what
 *                                the first compute entry does by itself if nothing was initialised.
 *   zkp_init_devices(devs, n)    n slots, slot i on HIP device devs[i]; devs == NULL: devices 0..n-1; n == 0: every visible
 *                                device.  A device may be listed more than once (separate slots on one GPU: how a 1-GPU box
 *                                rehearses the multi-device entries).  With more than one slot:
 *                                  - zkp_g1_bases_create SHARDS the points by contiguous chunk, one chunk resident per slot,
 *                                    unless the calling thread chose a slot with zkp_set_device;
 *                                  - zkp_msm_g1 / zkp_msm_g1_partial / zkp_kzg_commit / zkp_kzg_open over sharded bases run
 *                                    the whole Pippenger on every device's chunk concurrently (one resident host thread per
 *                                    slot uploads that chunk's scalars over its own PCIe link) and add the per-device
 *                                    partial sums (192 B each) on the host -- EC addition is not a collective's reduction
 *                                    operator, so "all-reduce of partial sums" is gather + add, here without leaving the
 *                                    process;
 *                                  - zkp_g1_bases_precompute expands every chunk on its own device;
 *                                  - `*_dev` entries and the PLONK prover take single-slot handles (device memory belongs
 *                                    to one device; a 2^16-gate proof does not shard: one prover per device).
 *   zkp_set_device(slot)         slot used by THIS thread's entries that carry no handle (NTT, FRI, fixed-base, *_create);
 *                                -1 = default: slot 0, and zkp_g1_bases_create shards over all slots.
 *   zkp_device_count()           number of slots (0 before initialisation). */
int zkp_init(int device);
int zkp_init_devices(const int *devices, int n_devices);
int zkp_device_count(void);
int zkp_set_device(int slot);
void zkp_shutdown(void);
const char *zkp_last_error(void);
/* ABI version of this header (bumped on incompatible change). */
int zkp_abi_version(void);

/* ---- optional per-phase timing (used by bench.py for the roofline object).  When enabled the library brackets
 *      each kernel phase with HIP events on the launch stream.  Phase names: "msm_digits", "msm_sort",
 *      "msm_accumulate", "msm_bucket_reduce", "msm_tail_host" (host, wall clock), "ntt_fr_pass", "ntt_gl_pass",
 *      "fri_merkle".
 *      zkp_profile_read waits for the recorded events and returns the summed milliseconds and the number of
 *      records with that name since the last reset.  zkp_profile_enable(2) records the dominant kernel only ("msm_accumulate",
 *      events and clock stamps): every recorded phase boundary is a marker on the stream, a bubble of ~5 us inside the region a
 *      benchmark times; 1 records every phase, 0 none. ---- */
void zkp_profile_enable(int on);
void zkp_profile_reset(void);
int zkp_profile_read(const char *name, double *total_ms, uint64_t *count);
/* The shader clock a kernel family ran at.  The chip lowers its clock under load and boxes differ, so the same cycle count takes a
 * different time from box to box; while profiling is enabled, wave 0 of every workgroup of the instrumented kernels ("msm_accumulate")
 * stamps s_memtime (shader cycles) and s_memrealtime (constant 100 MHz) at its start and end.  *cycles / *ref_ticks x 100 MHz = the
 * clock held under that kernel's own load, weighted by wave lifetime, since the last zkp_profile_reset; *waves = stamped workgroups. */
int zkp_profile_clock_read(const char *name, uint64_t *cycles, uint64_t *ref_ticks, uint64_t *waves);
/* Issue rate of v_mad_u64_u32 -- the instruction a 381-bit Montgomery product is made of (392 per product) -- on this device, now:
 * `launches` back-to-back launches (~1 ms each) of a probe kernel at full occupancy.  *lane_mads_per_s is the measured peak the
 * multiply-add rate of msm_accumulate is priced against (bench.py: roofline.integer_issue), *clock_mhz the shader clock the probe
 * held.  A measurement aid, not part of the hot path. */
int zkp_probe_mad_rate(unsigned launches, double *lane_mads_per_s, double *clock_mhz, double *ms_per_launch);

/* ---- G1 bases: the SRS `Vec<G1Affine>` of kzg/src/srs.rs:14-21 uploaded ONCE (the reference clones it per
 *      commit, srs.rs:78-80).  `xy` is n x 12 limbs; `is_inf` may be NULL (no infinity points). ---- */
int zkp_g1_bases_create(const uint64_t *xy, const uint8_t *is_inf, size_t n, zkp_bases **out);
/* Same, from n x 12 limbs already in device memory (copied; the caller keeps its buffer). */
int zkp_g1_bases_create_dev(const void *d_xy, const uint8_t *d_is_inf, size_t n, void *stream, zkp_bases **out);
/* Optional one-off expansion of resident bases for the shared-bucket MSM: stores the ceil(256 / window_bits) multiples
 * 2^(window_bits * s) * P_i of every point (128 B each), so that all windows of a scalar fall into ONE bucket set: a wider
 * window (fewer bucket insertions per scalar), one bucket reduction instead of one per window, and no window combination.
 * Costs ceil(256/window_bits) x the memory (13 x at 20 bits: 1.7 GB for 2^20 points; 12 x at 22 bits: 103 GB for 2^26 of the
 * 288 GB) and ~650 field products per stored point, once per SRS.  Results of zkp_msm_g1* are unchanged (same group element).
 * window_bits: 9..24, or 0 = automatic (22 from 2^22 points, 20 from 2^19, 16 above 2^13, 14 above 2^11, 12 from 64, otherwise
 * left as is; below 2^19 points the MSM is latency-bound and the narrow windows go with bucket runs split over several lanes).  A
 * scalar is cut into ceil(256 / window_bits) slices; when that many windows overshoot the 256 bits (every width but 16) the
 * slices are balanced to floor/ceil(256 / slices) bits instead (19 -> 14 slices of 18/19 bits, 2^18 buckets; 20 -> 13 slices of
 * 19/20 bits, 2^19 buckets; 22 -> 12 slices of 21/22 bits, 2^21 buckets), so that no slice is short and no group of buckets
 * collects a multiple of the others' points.  Once expanded, every MSM over these bases
 * uses the shared bucket set (2^10 terms: 0.28 ms against 0.85 ms per-window, whose host-side window combination alone is
 * 0.4 ms).  For a sharded handle every chunk is expanded on its own device, all chunks alike (automatic width: that of the largest
 * chunk) and all-or-nothing: every device is asked for room before any chunk allocates, so a ZKP_E_NOMEM refusal leaves the whole
 * handle unexpanded and a later call with another width is accepted.
 * zkp_g1_bases_precompute_glv below stores about half as many planes for the same MSM results: choose it when the footprint or the
 * one-off expansion time matters (a 2^26 or 2^27 SRS, an SRS expanded per KzgScheme::new); this entry stays the default. */
int zkp_g1_bases_precompute(zkp_bases *b, unsigned window_bits);
/* zkp_g1_bases_precompute for the endomorphism-split MSM: ceil(129 / window_bits) planes instead of ceil(256 / window_bits);
 * results of every MSM / KZG / PLONK / Nova entry over the handle are unchanged (same group element).
 * BLS12-381 G1 has phi(x, y) = (beta x, y) = [lambda](x, y) with lambda = z^2 - 1 of 128 bits.  A scalar k < r is split on the device
 * into k = k1 + lambda k2 (k2 = k div lambda; both halves at most lambda + 1 < 0.674 * 2^128, csrc/glv.hpp), the two halves are run as
 * two scalar vectors over the same planes with one bucket set each, and the host returns V1 + phi(V2).  The planes therefore only
 * cover 129 bits: 22 bits -> 6 planes of 21/22 bits instead of 12, 20 -> 7 of 18/19 (2^18 buckets per set) instead of 13, 16 -> 9
 * of 14/15, 12 -> 11 of 11/12.  Saves: half the expansion memory (2^26 points at 22 bits: 51.5 GB instead of 103 GB; a 2^27 SRS fits
 * one device) and half the expansion work.  Costs: two bucket sets -- two bucket reductions and two host tails -- per MSM, 2 x planes
 * insertions per scalar (12 at 22 bits as before, 14 instead of 13 at 20), and a batch (zkp_msm_g1_batch_dev) of at most 32 MSMs
 * instead of 64 (ZKP_E_ARG above).  Measured on one MI355X: expansion 15.9 instead of 33.9 ms at 2^20 points and 242
 * instead of 511 ms at 2^24; a warm MSM 2.97 instead of 2.39 ms at 2^20, 9.4 instead of 8.6 ms at 2^22, 31.8 instead of 31.2 ms at 2^24.  Same arguments, automatic widths and refusals as zkp_g1_bases_precompute (ZKP_E_NOMEM with the
 * sizes, ZKP_SRS_EXPAND_MAX_BYTES, all-or-nothing over the chunks of a sharded handle).  A handle is expanded one way: asking for the
 * other mode on an expanded handle is ZKP_E_ARG, like another width; the same mode and width again is ZKP_OK.
 * phi(P) = [lambda]P holds in G1 and nowhere else on the curve, so the results equal those of the plain expansion only for bases in
 * the prime-order subgroup: neither entry checks that -- zkp_g1_bases_validate below does. */
int zkp_g1_bases_precompute_glv(zkp_bases *b, unsigned window_bits);
size_t zkp_g1_bases_len(const zkp_bases *b);
/* How the bases are expanded: *window_bits = the width asked for (0 = not expanded), *slices = insertions per scalar. */
int zkp_g1_bases_info(const zkp_bases *b, unsigned *window_bits, unsigned *slices);
/* The expansion in full: planes stored per point, glv = 1 for zkp_g1_bases_precompute_glv planes (slices = 2 x planes then, else
 * planes), the widest slice in bits (2^(widest - 1) buckets per set).  All zero when the bases are not expanded. */
typedef struct {
    unsigned window_bits, slices, planes, glv, widest_slice_bits;
    size_t bytes;   /* device bytes of the planes, summed over shards */
} zkp_bases_expansion;
int zkp_g1_bases_expansion(const zkp_bases *b, zkp_bases_expansion *out);
void zkp_g1_bases_destroy(zkp_bases *b);

/* ---- G1 validity on the GPU.  This ABI is the deserialisation boundary: the reference holds typed arkworks points that were
 *      validated when they were built, a caller of this library hands over raw limbs.  The verifiers check their few G1 inputs on the
 *      host ([r]P, csrc/verify_host.inc); these entries check whole arrays -- an SRS -- with one lane per point.  Per point that is not
 *      flagged as infinity, in this order, the first failure being the point's status:
 *        1 non-canonical     a coordinate's six limbs are not below p as stored
 *        2 off the curve     y^2 != x^3 + 4
 *        3 outside G1        [z^2]P != P + phi(P), z = -0xd201000000010000, phi(x, y) = (beta x, y): 2 x (63 doublings + 5 additions)
 *                            instead of the 255 doublings of [r]P; sound and complete (csrc/g1_check.hpp)
 *      and 0 for a valid point.  A point flagged as infinity is valid and its coordinates are not looked at.
 *      A bad point is a finding, not an error: the entries return ZKP_OK with the report filled; ZKP_E_ARG is for null arguments.
 *      n == 0 gives an all-zero report.  The status arrays (one byte per point) may be NULL.
 *      Nothing else in the library calls these: zkp_g1_bases_create* and the expansions take the points as they come. ---- */
typedef struct {
    uint64_t checked, bad;                               /* points looked at (infinity flags included), points with status != 0 */
    uint64_t non_canonical, off_curve, outside_subgroup; /* sums to bad */
    uint64_t first_bad;                                  /* lowest bad index, or n when bad == 0 */
    int first_status;                                    /* its status, or 0 */
} zkp_g1_validation;
/* n x 12 limbs in device memory (the slot is chosen from the pointer as in zkp_g1_bases_create_dev); d_status: device memory.
 * Synchronises `stream` before it returns. */
int zkp_g1_validate_dev(const void *d_xy, const uint8_t *d_is_inf, size_t n, uint8_t *d_status, void *stream, zkp_g1_validation *out);
/* The same from host memory, uploaded in pieces of 2^18 points (24 MiB of staging); indices in the report are global.  Runs on the
 * thread's zkp_set_device() slot, or slot 0. */
int zkp_g1_validate(const uint64_t *xy, const uint8_t *is_inf, size_t n, uint8_t *status, zkp_g1_validation *out);
/* The points of a handle: plain, expanded either way, or sharded (every chunk on its own device).  `status` is HOST memory of
 * zkp_g1_bases_len(b) bytes.  The handle holds the device-internal form, which has lost the raw limbs: this entry reports statuses
 * 0, 2 and 3 only, and a point whose raw limbs were not canonical comes out as 2 or 3 -- use zkp_g1_validate* on the raw points
 * where that distinction matters.  Call it on any SRS that did not come from typed, checked values, and always before
 * zkp_g1_bases_precompute_glv. */
int zkp_g1_bases_validate(const zkp_bases *b, uint8_t *status, zkp_g1_validation *out);
/* Are the first n points of the handle [s^i]G, i < n, for the s behind g2s = [s]_2?  *accepted = 1 or 0.
 *   P_0 must be the G1 generator (KzgScheme::verify multiplies G1Point::generator(), kzg/src/scheme.rs:165: an SRS scaled by a constant
 *   would commit consistently and never verify), and e(sum r_i P_i, [s]_2) = e(sum r_i P_{i+1}, G_2) over i < n - 1.
 * r: (n - 1) x 4 limbs, Fr memory form, the caller's randomness -- as r_primes of zkp_kzg_batch_verify, which stand for the reference's
 * Fr::from(rng.gen::<u128>()).  The sums are two MSMs over the handle (sharded and expanded handles work), the pairings run on the
 * host.  ASSUMES VALID POINTS: call zkp_g1_bases_validate first.  n == 0 or a g2s that is not a valid G2 point: ZKP_E_ARG;
 * n above the handle's length: ZKP_E_SIZE; n == 1 checks P_0 only. */
int zkp_srs_check(const zkp_bases *srs, const uint64_t g2s_xy[24], size_t n, const uint64_t *r, int *accepted);

/* ---- Compressed G1 points and scalars as bytes, decoded and encoded on the GPU (csrc/g1_codec.hpp).  A ceremony SRS, a commitment
 *      and a cell proof travel as 48-byte points: bits 7, 6 and 5 of byte 0 are the flags c (compressed, must be 1), i (infinity) and
 *      s (y is the larger of {y, p - y} as canonical integers: y > (p - 1) / 2), the remaining 381 bits are the canonical x, big-endian;
 *      infinity is c0 followed by 47 zero bytes.  This is what ark-bls12-381 0.4 serialize_compressed writes.  Decoding costs one
 *      square root per point, y = (x^3 + 4)^((p + 1) / 4), one lane per point.  It is strict; per point, in this order, the first
 *      failure being the point's status:
 *        4 malformed         c = 0, or i = 1 with s = 1 or any other bit set
 *        1 non-canonical     x >= p
 *        2 off the curve     x^3 + 4 is not a square
 *        3 outside G1        only with ZKP_G1_DECODE_SUBGROUP in `flags` (the test of zkp_g1_validate, a second launch over the decoded points)
 *      and 0 for a valid point, a well-formed infinity included.  A point with status != 0 is written as twelve zero limbs with
 *      is_inf = 0 -- (0, 0) is off the curve, so whoever ignores the report cannot carry it further unnoticed.
 *      A bad point is a finding, not an error: the decompress entries return ZKP_OK with the report filled.  ZKP_E_ARG is for a null
 *      required argument, an unknown bit in `flags`, and a device pointer to bytes or limbs that is not 16-byte aligned.  n == 0 is
 *      ZKP_OK with an all-zero report, before the device is touched.  Encoding does not validate: limbs that are no point give bytes
 *      that are no encoding, never a fault. ---- */
#define ZKP_G1_DECODE_SUBGROUP 1u
typedef struct {
    uint64_t checked, bad;                                          /* points looked at, points with status != 0 */
    uint64_t malformed, non_canonical, off_curve, outside_subgroup; /* sums to bad */
    uint64_t first_bad;                                             /* lowest bad index, or n when bad == 0 */
    int first_status;                                               /* its status, or 0 */
} zkp_g1_decoding;
/* n x 48 bytes in device memory -> n x 12 limbs and n infinity bytes in device memory (the slot is chosen from d_bytes as in
 * zkp_g1_validate_dev); d_status: n bytes of device memory, or NULL.  Synchronises `stream` before it returns. */
int zkp_g1_decompress_dev(const void *d_bytes, size_t n, unsigned flags, void *d_out_xy, uint8_t *d_out_is_inf, uint8_t *d_status,
                          void *stream, zkp_g1_decoding *out);
/* The same from and to host memory, uploaded in pieces of 2^18 points; indices in the report are global.  `status` may be NULL.  Runs
 * on the thread's zkp_set_device() slot, or slot 0. */
int zkp_g1_decompress(const uint8_t *bytes, size_t n, unsigned flags, uint64_t *out_xy, uint8_t *out_is_inf, uint8_t *status,
                      zkp_g1_decoding *out);
/* n x 12 limbs (d_is_inf may be NULL: every point finite) -> n x 48 bytes, all in device memory.  Does not synchronise. */
int zkp_g1_compress_dev(const void *d_xy, const uint8_t *d_is_inf, size_t n, void *d_out_bytes, void *stream);
/* The same from and to host memory, on the thread's zkp_set_device() slot or slot 0. */
int zkp_g1_compress(const uint64_t *xy, const uint8_t *is_inf, size_t n, uint8_t *out_bytes);
/* zkp_g1_bases_create from n x 48 bytes of host memory: decoded on the calling thread's slot (zkp_set_device; slot 0 by default) into
 * device memory that goes straight to the path of zkp_g1_bases_create_dev -- the 96-byte points never visit the host.  IT NEVER
 * SHARDS: with several slots the handle lives on that one slot.  Any bad point is ZKP_E_ARG with no handle left, the report
 * (nullable) filled, and zkp_last_error() naming the lowest bad index and one of the words "encoding", "canonical", "curve",
 * "subgroup". */
int zkp_g1_bases_create_compressed(const uint8_t *bytes, size_t n, unsigned flags, zkp_g1_decoding *report, zkp_bases **out);
/* Scalars: n x 32 bytes holding canonical integers below r, big-endian (big_endian != 0: Ethereum's KZG convention) or little-endian
 * (ark's serialize of Fr), <-> n x 4 limbs in the Fr memory form, all in device memory (16-byte aligned).  A value >= r is counted in
 * *bad and its slot zeroed; *first_bad (nullable) = the lowest such index, or n.  zkp_fr_from_bytes_dev synchronises `stream`,
 * zkp_fr_to_bytes_dev does not. */
int zkp_fr_from_bytes_dev(const void *d_bytes, size_t n, int big_endian, void *d_out, void *stream, uint64_t *bad, uint64_t *first_bad);
int zkp_fr_to_bytes_dev(const void *d_in, size_t n, int big_endian, void *d_out_bytes, void *stream);

/* ---- MSM: replaces the body of KzgScheme::evaluate_in_s, kzg/src/scheme.rs:84-96 (reached from commit :49,
 *      commit_vector :63, open :108, open_vector :132 and the 9 commit sites of plonk/src/prover.rs:92,123,150,
 *      267-268).  out = sum_{i<n} scalars[i] * bases[i]; n == 0 gives the identity (scheme.rs:94).
 *      n > len(bases) returns ZKP_E_SIZE (the reference asserts, scheme.rs:86).
 *      `scalars` is host memory (pageable is fine) and is read only while the call runs: from 2^19 terms over expanded bases it is
 *      uploaded in two or three ranges, the later ones by a resident uploader thread of the library underneath the kernels of the
 *      earlier ones. ---- */
int zkp_msm_g1(const zkp_bases *bases, const uint64_t *scalars, size_t n, uint64_t out_xy[12], uint8_t *out_is_inf);
/* Scalars already in device memory (n x 4 limbs).  Synchronises `stream` before returning the host result. */
int zkp_msm_g1_dev(const zkp_bases *bases, const void *d_scalars, size_t n, void *stream, uint64_t out_xy[12],
                   uint8_t *out_is_inf);
/* `count` MSMs over the same bases with scalar vectors of the same length n (device pointers), processed as one pass
 * through the kernels: the commit_round1 / SlicePoly::commit / W_zeta, W_zeta_omega groups of plonk/src/prover.rs:92,150,
 * 267-268.  out_xy: count x 12 limbs; out_is_inf: count bytes. */
int zkp_msm_g1_batch_dev(const zkp_bases *bases, const void *const *d_scalars, size_t count, size_t n, void *stream,
                         uint64_t *out_xy, uint8_t *out_is_inf);
/* The three entries above for SHORT scalars: the caller states that every canonical scalar is below 2^bits (128-bit random weights of a
 * batched check, witness columns of bits, bytes or words), and the MSM runs only the slices such scalars fill: the first t slices of
 * the handle's offset table, t the smallest index with off[t] >= bits + 1 -- per-window mode: t of the 256 / c windows; an expansion:
 * its first t planes; split planes (zkp_g1_bases_precompute_glv) up to 127 bits: ONE bucket set over the first t planes with no
 * scalar split (a scalar below 2^127 < lambda is its own low half), so a batch may again hold 64 vectors; from 128 bits on a split
 * handle runs both bucket sets over all its slices.  The result is the point the unbounded entry gives, bit for bit.
 *   bits        1..256, else ZKP_E_ARG before anything is launched.  bits >= 255 IS the unbounded entry (r < 2^255).  One bound holds
 *               for every vector of a batch.
 *   violation   a scalar that is not below 2^bits: ZKP_E_ARG, zkp_last_error() names one offending vector and its index in that
 *               vector, and the bound; the outputs are not written.  The kernels check this themselves and the pass runs to its end,
 *               so the handle and the slot's workspaces serve the next call; an accepted call pays no launch and no wait for the check.
 *   refusals    a sharded handle is ZKP_E_ARG (also for zkp_msm_g1_bits: bounded MSMs take single-device bases); everything else as
 *               the unbounded entry: n > len(bases) ZKP_E_SIZE, the batch limits, null arguments.
 * zkp_msm_g1_bits feeds host scalars exactly as zkp_msm_g1 does, ranges from 2^19 terms over expanded bases included. */
int zkp_msm_g1_bits(const zkp_bases *bases, const uint64_t *scalars, size_t n, unsigned bits, uint64_t out_xy[12], uint8_t *out_is_inf);
int zkp_msm_g1_bits_dev(const zkp_bases *bases, const void *d_scalars, size_t n, unsigned bits, void *stream, uint64_t out_xy[12],
                        uint8_t *out_is_inf);
int zkp_msm_g1_batch_bits_dev(const zkp_bases *bases, const void *const *d_scalars, size_t count, size_t n, unsigned bits, void *stream,
                              uint64_t *out_xy, uint8_t *out_is_inf);
/* *out_bits = the largest bit length among n scalars in device memory (n x 4 limbs, the Fr memory form, 16-byte aligned): the smallest
 * `bits` the entries above accept for this vector; 0 for n == 0 or all zeros.  One memory-bound pass (32 bytes per scalar) on the
 * slot chosen from d_scalars as in zkp_g1_validate_dev.  BLOCKS: synchronises `stream` before it returns. */
int zkp_fr_bit_length_dev(const void *d_scalars, size_t n, void *stream, unsigned *out_bits);
/* Multi-GPU building block: the same sum left UNNORMALISED as an extended-Jacobian point
 * (X, Y, ZZ, ZZZ = 24 limbs, ZZ == 0 for the identity) so that per-GPU partial sums can be exchanged
 * (RCCL all-gather of 192 bytes per rank) and combined with zkp_g1_xyzz_sum. */
int zkp_msm_g1_partial_dev(const zkp_bases *bases, const void *d_scalars, size_t n, void *stream, uint64_t out_xyzz[24]);
/* The same from host scalars (sharded bases allowed: the partial is then already the sum over this process's devices; a
 * multi-node caller exchanges these between processes). */
int zkp_msm_g1_partial(const zkp_bases *bases, const uint64_t *scalars, size_t n, uint64_t out_xyzz[24]);
/* Sharded bases with the scalars already RESIDENT on the devices (a prover that keeps its polynomials in HBM): chunk i of the handle
 * (zkp_g1_bases_shard: its slot, HIP device, first point and length) multiplies the scalars at d_scalars[i], which must be memory of that
 * chunk's device; n is the TOTAL number of scalars (chunk i uses those of its range that are below n).  Every device runs its chunk
 * on its own stream concurrently; the call returns the affine sum.  A single-slot handle has one chunk (d_scalars[0]).
 * Ordering: the entry takes no stream argument and launches on each slot's own non-blocking stream (the legacy null stream for a
 * runtime with a single slot), neither of which is ordered after work on the caller's non-blocking streams.  zkp_msm_g1_sharded_dev
 * therefore waits for ALL work previously enqueued on each chunk's device before reading d_scalars[i] (hipDeviceSynchronize, single-
 * and multi-slot handles alike): a copy or kernel that produces the scalars on any stream of that device may still be in flight
 * when the call is made.  zkp_msm_g1_sharded_dev_after is the non-blocking form for resident pipelines: ready_events[i] is a
 * hipEvent_t the producer of d_scalars[i] recorded after enqueuing that work; the chunk's launch waits for it ON THE DEVICE
 * (hipStreamWaitEvent) and the host does not stall.  A null array or a null entry falls back to the device-wide wait for that chunk.
 * Work enqueued on the device concurrently with the call from another thread is not ordered against it. */
int zkp_g1_bases_shard_count(const zkp_bases *b);
int zkp_g1_bases_shard(const zkp_bases *b, size_t i, int *slot, int *device, size_t *offset, size_t *len);
int zkp_msm_g1_sharded_dev(const zkp_bases *bases, const void *const *d_scalars, size_t n, uint64_t out_xy[12],
                           uint8_t *out_is_inf);
int zkp_msm_g1_sharded_dev_after(const zkp_bases *bases, const void *const *d_scalars, void *const *ready_events, size_t n,
                                 uint64_t out_xy[12], uint8_t *out_is_inf);
/* Sum `count` extended-Jacobian partials (host memory, count x 24 limbs) and normalise to affine. */
int zkp_g1_xyzz_sum(const uint64_t *partials, size_t count, uint64_t out_xy[12], uint8_t *out_is_inf);

/* ---- KzgScheme mirror (host logic in csrc/kzg_host.hpp): commit / commit_vector, kzg/src/scheme.rs:49-67 --
 *      trailing zero coefficients are trimmed first, as DensePolynomial::from_coefficients_vec does; an SRS that
 *      is empty or shorter than the trimmed polynomial gives ZKP_E_SIZE (assert at scheme.rs:86). ---- */
int zkp_kzg_commit(const zkp_bases *srs, const uint64_t *coeffs, size_t len, uint64_t out_xy[12], uint8_t *out_is_inf);
/* open / open_vector, kzg/src/scheme.rs:108-142: out_eval = p(z), out = commit((p - p(z)) / (X - z)).
 * len == 0 returns ZKP_E_ARG (the reference panics with "at least 1", scheme.rs:112). */
int zkp_kzg_open(const zkp_bases *srs, const uint64_t *coeffs, size_t len, const uint64_t z[4], uint64_t out_xy[12],
                 uint8_t *out_is_inf, uint64_t out_eval[4]);

/* ---- Transform over G1 POINTS (beyond the reference's surface; csrc/g1_ntt.hpp).  n = 2^log_n, w = the root zkp_ntt_fr uses for
 *      the same log_n, natural order in and out:
 *        forward  Y_i = sum_{j<n} [w^(ij)] P_j          inverse  P_j = [n^-1] sum_{i<n} [w^(-ij)] Y_i
 *      Points are n x 12 limbs + n flag bytes as everywhere; the limbs of a point flagged as infinity are ignored on input and
 *      written as zeros on output.  Inputs are NOT validated (zkp_g1_validate* does that): garbage in, garbage out, never a fault.
 *      One lane per butterfly multiplies a variable point by a 255-bit twiddle: endomorphism split, joint double-and-add over
 *      {P, phi(P), P + phi(P)}, complete additions.  The cost is n/2 log_n such multiplications; nothing here is a memory-bound pass.
 *      log_n > 24 is ZKP_E_ARG; a workspace (256 B per point + at most 64 MiB) that does not fit is ZKP_E_NOMEM with the sizes in
 *      zkp_last_error() and nothing left allocated.  The *_dev entries return without synchronising, with two exceptions shared by
 *      all of them: the first call on a device slot uploads 41 KB of twiddle constants and waits for them, and a call that needs a
 *      larger workspace than the slot holds allocates it. ---- */
/* P_i <- [k_i] P_i in place: d_xy n x 12 limbs, d_scalars n x 4 limbs (Fr memory form), all device memory of one device (the slot
 * is chosen from d_xy as in zkp_g1_bases_create_dev).  d_is_inf may be NULL (every point finite; a product that is the identity is
 * then written as zeros only).  k = 0 and P = O give O without arithmetic.  n == 0 does nothing. */
int zkp_g1_scale_dev(void *d_xy, uint8_t *d_is_inf, const void *d_scalars, size_t n, void *stream);
/* In place on device memory; d_is_inf is required (a transform of finite points has infinite outputs). */
int zkp_g1_ntt_dev(void *d_xy, uint8_t *d_is_inf, unsigned log_n, int inverse, void *stream);
/* The same on host memory, on the thread's zkp_set_device() slot or slot 0. */
int zkp_g1_ntt(uint64_t *xy, uint8_t *is_inf, unsigned log_n, int inverse);
/* The Lagrange-basis SRS: the inverse transform of the first n points of `srs`, i.e. [L_i(s)]G for an SRS [s^i]G, as an ordinary
 * unexpanded handle of n points on the source's slot -- every MSM / KZG / PLONK entry, both expansions and zkp_g1_bases_validate
 * take it, and zkp_kzg_commit(lagrange, evals, n) is the commitment of the interpolant of `evals` on the domain.  The source may be
 * plain or expanded either way; a sharded source is ZKP_E_ARG (multi-device transforms are not built), fewer than n points ZKP_E_SIZE. */
int zkp_g1_bases_lagrange(const zkp_bases *srs, unsigned log_n, zkp_bases **out);
/* All n openings of one polynomial at the n roots of unity (Feist-Khovratovich): for f = sum_{k<len} f_k X^k, len <= n,
 *   out point m = [(f(s) - f(w^m)) / (s - w^m)]G = what zkp_kzg_open returns at z = w^m, and out_evals[m] = f(w^m),
 * from three point transforms (two of 2n, one of n) and one pointwise pass of 2n products instead of n MSMs.  This is the coset
 * construction below with cosets of one point: zkp_kzg_opener_create(srs, log_n, out) is zkp_kzg_opener_create_cosets(srs, log_n, 0,
 * out), and zkp_kzg_open_all* run what zkp_kzg_open_cosets* run on such an opener.  It holds the transform of the SRS (256 B x 2n)
 * and the workspaces of a call (832 B x n, plus a table of 256 B x min(2n, 2^18), at most 64 MiB); log_n is 1 .. 23 (else ZKP_E_ARG),
 * the source needs n - 1 points (ZKP_E_SIZE) on one device (sharded: ZKP_E_ARG) and may be destroyed afterwards; workspaces that do
 * not fit are ZKP_E_NOMEM as below.  len == 0 is ZKP_E_ARG as in zkp_kzg_open, len > n ZKP_E_SIZE; coefficients are used as given,
 * zero-padded (an all-zero or constant vector gives n identities).
 * out_xy n x 12 limbs, out_is_inf n bytes, out_evals n x 4 limbs or NULL.  Calls on one opener are serialised with its slot. */
typedef struct zkp_kzg_opener zkp_kzg_opener;
int zkp_kzg_opener_create(const zkp_bases *srs, unsigned log_n, zkp_kzg_opener **out);
void zkp_kzg_opener_destroy(zkp_kzg_opener *o);
int zkp_kzg_open_all(const zkp_kzg_opener *o, const uint64_t *coeffs, size_t len, uint64_t *out_xy, uint8_t *out_is_inf,
                     uint64_t *out_evals);
/* Everything in device memory of the opener's device, launched on `stream`.  Neither allocates nor synchronises: the opener owns
 * the workspaces, and its creation has already built the plans and tables of the two Fr transforms a call runs. */
int zkp_kzg_open_all_dev(const zkp_kzg_opener *o, const void *d_coeffs, size_t len, void *d_out_xy, uint8_t *d_out_is_inf,
                         void *d_out_evals, void *stream);
/* Coset openings: the n / l multi-point proofs of one polynomial, one per coset of l = 2^log_l points of the domain (the "cells" of
 * data-availability sampling).  With r = n / l and w the root zkp_ntt_fr uses for log_n, coset k < r is {w^(k + j r) : j < l}, the
 * roots of X^l - x_k^l for x_k = w^k, and
 *   out point k = [q_k(s)]G, q_k the quotient of f by X^l - x_k^l,
 * from the multi-point form of the same algorithm: per slice b < l of the SRS a transform of 2r points (kept by the opener), per
 * call one batched Fr transform of l rows of 2r, a multiply-accumulate pass over the 2n products (one joint double-and-add per
 * group of terms, then a pairwise fold), and point transforms of 2r and r only.  zkp_kzg_opener_create_cosets is the one creation
 * of a zkp_kzg_opener: it holds the l transformed slices (256 B x 2n in all) and the workspaces of a call (256 B x 2n / B of partial sums
 * where a lane sums B < l terms, 768 B x r, 64 B x n of scalars and a table of 256 B x min(2n, 2^18)), and has built every
 * plan and table a call uses.  1 <= log_n - log_l and log_n <= 23, else ZKP_E_ARG; the source needs n - l points (ZKP_E_SIZE) on one
 * device (sharded: ZKP_E_ARG); workspaces that do not fit -- more than the device has free, or more than ZKP_KZG_OPENER_MAX_BYTES
 * (default: no limit) -- are ZKP_E_NOMEM with the sizes in zkp_last_error() and nothing left allocated, for every log_l.
 * log_l = 0 is the case of all n openings, one slice and one row: a lane of the pass takes one product and writes it where the
 * inverse transform runs, nothing is folded, and proof k is the opening at w^k.
 * zkp_kzg_open_cosets: out_xy r x 12 limbs, out_is_inf r bytes, out_evals n x 4 limbs or NULL -- f on the whole domain in natural
 * order, so the values of coset k sit at k + j r.  len == 0 is ZKP_E_ARG, len > n ZKP_E_SIZE; len <= l gives r identities.  It
 * takes an opener of any log_l (with log_l = 0 it is zkp_kzg_open_all); zkp_kzg_open_all* on an opener with log_l > 0 is ZKP_E_ARG.
 * The device entry, like zkp_kzg_open_all_dev, neither allocates nor synchronises.
 * ZKP_KZG_COSET_GROUP_LOG (0..3, read when an opener is created; tuning aid; without effect at log_l = 0) sets how many terms a lane
 * of the multiply-accumulate pass sums: profiles/kzg_open_cosets.md. */
int zkp_kzg_opener_create_cosets(const zkp_bases *srs, unsigned log_n, unsigned log_l, zkp_kzg_opener **out);
int zkp_kzg_open_cosets(const zkp_kzg_opener *o, const uint64_t *coeffs, size_t len, uint64_t *out_xy, uint8_t *out_is_inf,
                        uint64_t *out_evals);
int zkp_kzg_open_cosets_dev(const zkp_kzg_opener *o, const void *d_coeffs, size_t len, void *d_out_xy, uint8_t *d_out_is_inf,
                            void *d_out_evals, void *stream);
/* The coset openings of a batch of polynomials in one call: every dependent step of zkp_kzg_open_cosets runs once for all of them,
 * so a batch costs about what one polynomial costs until the device is full (profiles/kzg_open_cosets_batch.md).
 * zkp_kzg_opener_create_cosets_batch makes an opener for up to max_polys (1 .. 4096, else ZKP_E_ARG) polynomials per call;
 * zkp_kzg_opener_create_cosets is this creation with max_polys = 1, and every other condition and refusal is the same.  The opener
 * owns the workspaces of a whole batch from creation on: per polynomial 256 B x 2n / B of partial sums (where a lane sums B < l
 * terms), 768 B x r and 64 B x n of scalars -- with the committed B = 1 about 512 n + 768 r + 64 n bytes, 4.7 MiB at (log_n, log_l) =
 * (13, 6), about 600 MiB at (20, 6) -- next to the 256 B x 2n of kept slices and a table of 256 B x min(max_polys 2n, 2^18).  What
 * does not fit, ZKP_KZG_OPENER_MAX_BYTES included, is ZKP_E_NOMEM with the kept slices, the per-call bytes and max_polys in
 * zkp_last_error() and nothing left allocated.  An opener of any max_polys serves zkp_kzg_open_cosets* (and zkp_kzg_open_all* at
 * log_l = 0); one of log_l = 0 serves the batch entries: all n openings of each polynomial.
 * zkp_kzg_open_cosets_batch: polynomial p < n_polys has its len coefficients at coeffs + 4 stride p; stride is in scalars, the
 * scalars between len and stride are not read (a shorter polynomial of a batch is a row with trailing zeros).  Outputs are
 * polynomial-major -- out_xy n_polys x r x 12 limbs, out_is_inf n_polys x r bytes, out_evals n_polys x n x 4 limbs or NULL -- and
 * row p of each is byte for byte what zkp_kzg_open_cosets returns for polynomial p.  Refused before anything is launched: a null
 * argument ZKP_E_ARG, len == 0 ZKP_E_ARG, len > n ZKP_E_SIZE, stride < len ZKP_E_ARG, n_polys > max_polys ZKP_E_SIZE (with both
 * numbers in zkp_last_error()); n_polys == 0 is ZKP_OK without touching the device.  The device entry, like
 * zkp_kzg_open_cosets_dev, neither allocates nor synchronises. */
int zkp_kzg_opener_create_cosets_batch(const zkp_bases *srs, unsigned log_n, unsigned log_l, size_t max_polys, zkp_kzg_opener **out);
int zkp_kzg_open_cosets_batch(const zkp_kzg_opener *o, const uint64_t *coeffs, size_t n_polys, size_t len, size_t stride,
                              uint64_t *out_xy, uint8_t *out_is_inf, uint64_t *out_evals);
int zkp_kzg_open_cosets_batch_dev(const zkp_kzg_opener *o, const void *d_coeffs, size_t n_polys, size_t len, size_t stride,
                                  void *d_out_xy, uint8_t *d_out_is_inf, void *d_out_evals, void *stream);
/* host + one commitment on the GPU: the check of one coset proof.  evals[j] = f(x w_l^j) for j < l = 2^log_l, w_l the root of
 * zkp_ntt_fr for log_l (for coset k of an opener: x = w^k, evals[j] = out_evals[k + j r]); g2_sl is [s^l]_2.  Accepts iff
 *   e(W, [s^l]_2 - [x^l]_2) == e(C - [I(s)]_1, G_2),
 * I the interpolant of the evaluations on the coset (its coefficients are computed on the host, [I(s)]_1 is zkp_kzg_commit over
 * the first l points of `srs`).  The G2 point and both G1 points are validated as in zkp_kzg_verify (off the curve, outside the
 * subgroup, limbs >= p: ZKP_E_ARG); fewer than l points in `srs` is ZKP_E_SIZE, x = 0 ZKP_E_ARG. */
int zkp_kzg_verify_coset(const zkp_bases *srs, const uint64_t g2_sl_xy[24], const uint64_t commit_xy[12], uint8_t commit_is_inf,
                         const uint64_t w_xy[12], uint8_t w_is_inf, const uint64_t x[4], unsigned log_l, const uint64_t *evals,
                         int *accepted);
/* Cell recovery: the polynomial f of `len` coefficients from the values of any (r - m) cosets with (r - m) l >= len, in the notation of
 * the coset openings (n = 2^log_n, l = 2^log_l, r = n / l; coset k < r holds the indices k + j r of a natural-order evaluation
 * vector).  Fr only, no SRS: with Zs(Y) = prod over the m missing cosets k of (Y - rho^k), rho = w^l, the vanishing polynomial of
 * the missing points is Zs(X^l); the values times Zs(rho^(i mod r)), zero on the missing cosets, are those of f Zs(X^l), whose
 * coefficients are divided by Zs((g X)^l) on the coset g = 7 of the domain.  Zs is built on the device as a product tree (leaves
 * of 2^ZKP_KZG_RECOVER_LEAF_LOG factors in a workgroup, batched transforms above: O(m log^2 m) products), and a call costs two
 * transforms of r and three of n (four with out_evals) besides.
 * zkp_kzg_recoverer_create: a handle on the calling thread's slot (zkp_set_device; slot 0 by default) that owns every workspace
 * (32 B x (n + 5 r) + 5 r bytes on the device, 5 r bytes pinned) and has built every plan and table a call uses.  1 <= log_n - log_l
 * and log_n <= 23, else ZKP_E_ARG; a workspace larger than the device has free or than ZKP_KZG_RECOVER_MAX_BYTES is ZKP_E_NOMEM
 * with the sizes in zkp_last_error() and nothing left allocated; no device: ZKP_E_DEVICE (there is no host path).
 * zkp_kzg_recover_cosets: evals n x 4 limbs in natural order, present r bytes (0: the coset is missing; the 32 bytes at its
 * positions are not read), out_coeffs len x 4 limbs, out_evals n x 4 limbs or NULL -- f on the whole domain, the missing cells filled
 * in (the transform of the zero-padded result).  *consistent = 1 iff the present values are those of a polynomial of `len`
 * coefficients (exact: no recovered coefficient at an index >= len is non-zero; with (r - m) l == len every input is consistent);
 * out_coeffs is the low part of the interpolant either way.  Present values are used as given.  len == 0 is ZKP_E_ARG, len > n
 * ZKP_E_SIZE, (r - m) l < len ZKP_E_SIZE naming the present cells, l and len.  m = 0 is one inverse transform and the check.
 * zkp_kzg_recover_cosets_dev: d_evals, d_out_coeffs, d_out_evals (or NULL) and the word *d_inconsistent (set to 0 or 1) are memory
 * of the recoverer's device, `present` is HOST memory (the schedule depends on m) and is read before the call returns.  It neither
 * allocates nor waits for the device, except for the previous call's copy of the mask out of the handle's staging buffer; calls
 * on one handle are serialised with its slot.  (The tables of its three shifted transforms sit in the slot's cache of 8 coset
 * tables: a call that finds them evicted by other shifted transforms of the slot rebuilds them first.)  While profiling is on a call records the phases "kzg_recover_zs" (the vanishing
 * polynomial and its values on both domains) and "kzg_recover_rest" (the transforms of n and the pointwise passes); the transforms
 * record "ntt_fr_pass" inside both. */
typedef struct zkp_kzg_recoverer zkp_kzg_recoverer;
int zkp_kzg_recoverer_create(unsigned log_n, unsigned log_l, zkp_kzg_recoverer **out);
void zkp_kzg_recoverer_destroy(zkp_kzg_recoverer *rc);
int zkp_kzg_recover_cosets(const zkp_kzg_recoverer *rc, const uint64_t *evals, const uint8_t *present, size_t len,
                           uint64_t *out_coeffs, uint64_t *out_evals, int *consistent);
int zkp_kzg_recover_cosets_dev(const zkp_kzg_recoverer *rc, const void *d_evals, const uint8_t *present, size_t len,
                               void *d_out_coeffs, void *d_out_evals, uint32_t *d_inconsistent, void *stream);
/* Recovery of a batch: every blob of a block misses the same cosets, so the vanishing polynomial, its values and their inverses
 * are built once per call and everything behind them -- the masked multiply, the three transforms of n, the divide, the tail -- runs
 * once over all rows (profiles/kzg_recover_batch.md).
 * zkp_kzg_recoverer_create_batch makes a handle for up to max_polys (1 .. 4096, else ZKP_E_ARG) polynomials per call;
 * zkp_kzg_recoverer_create is this creation with max_polys = 1, and every other condition and refusal is the same.  Only the
 * n-element vector of the workspace grows, to max_polys x n; the refusal of a workspace that does not fit names max_polys too.
 * A handle of any max_polys serves zkp_kzg_recover_cosets*.
 * zkp_kzg_recover_cosets_batch: evals n_polys x n x 4 limbs, contiguous rows; ONE mask of r bytes and one len for all rows;
 * out_coeffs n_polys x len x 4 limbs, out_evals n_polys x n x 4 limbs or NULL, consistent one byte (1 or 0) per row -- a bad row
 * does not taint its neighbours.  layout applies to evals and out_evals: ZKP_KZG_LAYOUT_NATURAL, value j of coset k at k + j r of
 * its row as above; ZKP_KZG_LAYOUT_CELLS, at k l + j -- a row is r cells of l contiguous values, what zkp_kzg_verify_cells takes.
 * The slots of missing cells are not read in either layout; the coefficients do not depend on it.  Row p of every output is byte
 * for byte what zkp_kzg_recover_cosets returns for row p (in cell layout: its transposition).  Refused before anything is launched:
 * whatever zkp_kzg_recover_cosets refuses, with the same codes and texts; stride < len and an unknown layout (ZKP_E_ARG);
 * n_polys > max_polys (ZKP_E_SIZE, both numbers in zkp_last_error()); n_polys == 0 is ZKP_OK without touching the device.
 * zkp_kzg_recover_cosets_batch_dev: as zkp_kzg_recover_cosets_dev -- `present` is host memory read before the call returns, it
 * neither allocates nor synchronises.  Row p of d_out_coeffs begins at `stride` scalars times p and the scalars between len and
 * stride are not written, so that the buffer feeds zkp_kzg_open_cosets_batch_dev with the same stride; d_inconsistent is n_polys
 * words, each set to 0 or 1 for its own row. */
#define ZKP_KZG_LAYOUT_NATURAL 0
#define ZKP_KZG_LAYOUT_CELLS 1
int zkp_kzg_recoverer_create_batch(unsigned log_n, unsigned log_l, size_t max_polys, zkp_kzg_recoverer **out);
int zkp_kzg_recover_cosets_batch(const zkp_kzg_recoverer *rc, const uint64_t *evals, size_t n_polys, const uint8_t *present,
                                 size_t len, int layout, uint64_t *out_coeffs, uint64_t *out_evals, uint8_t *consistent);
int zkp_kzg_recover_cosets_batch_dev(const zkp_kzg_recoverer *rc, const void *d_evals, size_t n_polys, const uint8_t *present,
                                     size_t len, size_t stride, int layout, void *d_out_coeffs, void *d_out_evals,
                                     uint32_t *d_inconsistent, void *stream);

/* ---- batched cell verification: any number of cells of any number of commitments, one pairing check ----
 * n = 2^log_n, l = 2^log_l, r = n / l as above; w the root zkp_ntt_fr uses for log_n.  Cell i < n_cells belongs to the commitment
 * C_m, m = commit_index[i] < n_commits, and to the coset k = coset_index[i] < r: its l evaluations e_i[j] = f(w^k w_l^j), in the order
 * zkp_kzg_verify_coset takes them, are evals[i l .. i l + l) (n_cells x l x 4 limbs, cell-major, Fr memory form), its proof W_i is
 * proofs_xy[i], its weight rho_i is weights[i] (n_cells x 4 limbs).  With c_i = w^(k l) and I_i the interpolant of e_i on its coset,
 * the batch is accepted iff
 *   e( sum rho_i W_i , [s^l]_2 ) == e( sum_m (sum_{i: m_i = m} rho_i) C_m - [(sum rho_i I_i)(s)]_1 + sum rho_i c_i W_i , G_2 ),
 * the equation of zkp_kzg_verify_coset summed with the weights: two Miller loops and one final exponentiation whatever n_cells.
 * THE WEIGHTS ARE THE CALLER'S RANDOMNESS (as r_primes of zkp_kzg_batch_verify and r of zkp_srs_check): independent, unpredictable
 * to whoever made the cells, 128 bits are enough.  A weight of 0 drops its cell from the check; equal (or otherwise related) weights
 * let the errors of different cells cancel, so a batch with a wrong cell can be accepted.  A cell may appear more than once.
 * Everything before the pairings runs on the device: the interpolant sum is one weighted scatter of the evaluations into a vector of
 * n, one inverse transform of n and l products (sum_k (F mod (X^l - w^(k l))) = r (F mod X^l) for deg F < n); the G1 sums are one batch
 * of two MSMs over the n_commits + n_cells points and one MSM of l terms over the SRS.  ALL commitments and proofs are validated on
 * the device first (canonical, on the curve, in G1; the kernels of zkp_g1_validate): the batched equation is unsound on points
 * outside G1, so this is not optional.  A bad point is ZKP_E_ARG and zkp_last_error() names the array ("commits" or "proofs"), the
 * lowest bad index and the status word "canonical", "curve" or "subgroup".  is_inf arrays may be NULL (no identity among them).
 * zkp_kzg_cell_verifier_create: g2_sl_xy = [s^l]_2 is validated (ZKP_E_ARG); log_l < log_n <= 23, max_cells and max_commits in
 * 1 .. 2^30, else ZKP_E_ARG; a sharded SRS handle is ZKP_E_ARG, one with fewer than l points ZKP_E_SIZE.  THE SRS IS BORROWED: the
 * handle must outlive the verifier (it may be expanded or not).  The verifier lives on the SRS's slot and owns every workspace sized
 * by n, max_cells and max_commits (about 32 l bytes per cell); the plan and table of its transform are built here.  A workspace that
 * does not fit is ZKP_E_NOMEM with the sizes in zkp_last_error() and nothing left allocated.  No device: ZKP_E_DEVICE; there is no
 * host path.
 * zkp_kzg_verify_cells / _dev: a null argument is ZKP_E_ARG, n_cells > max_cells or n_commits > max_commits ZKP_E_SIZE, a coset index
 * >= r or a commitment index >= n_commits ZKP_E_ARG naming the cell -- all before anything is launched; n_cells == 0 accepts without
 * touching the device.  Both end in host pairings, so both BLOCK; the _dev form differs only in where its inputs live: d_commits_xy,
 * d_commits_is_inf, d_evals, d_proofs_xy, d_proofs_is_inf and d_weights are memory of the verifier's device, the two index arrays
 * stay HOST memory (the grouping is planned on the host).  Either form may allocate: the transient point handle of the call, and the
 * slot's MSM workspaces when they have to grow.  While profiling is on a call records the phases "kzg_cells_field",
 * "kzg_cells_points" (validation and the MSMs) and "kzg_cells_pairing" (host).
 * zkp_kzg_cells_aggregate_dev: the field half alone, exact to the bit: d_out_interp (l x 4 limbs) the coefficients of sum rho_i I_i,
 * d_out_commit_weights (n_commits x 4) the sums of the weights per commitment, d_out_proof_scalars (n_cells x 4) rho_i c_i.  Same
 * refusals.  It neither allocates nor waits for the device, except for the previous call's copy of the index tables out of the
 * handle's staging buffer; calls on one handle are serialised with its slot. */
typedef struct zkp_kzg_cell_verifier zkp_kzg_cell_verifier;
int zkp_kzg_cell_verifier_create(const zkp_bases *srs, const uint64_t g2_sl_xy[24], unsigned log_n, unsigned log_l, size_t max_cells,
                                 size_t max_commits, zkp_kzg_cell_verifier **out);
void zkp_kzg_cell_verifier_destroy(zkp_kzg_cell_verifier *v);
int zkp_kzg_verify_cells(const zkp_kzg_cell_verifier *v, const uint64_t *commits_xy, const uint8_t *commits_is_inf, size_t n_commits,
                         size_t n_cells, const uint32_t *commit_index, const uint32_t *coset_index, const uint64_t *evals,
                         const uint64_t *proofs_xy, const uint8_t *proofs_is_inf, const uint64_t *weights, int *accepted);
int zkp_kzg_verify_cells_dev(const zkp_kzg_cell_verifier *v, const void *d_commits_xy, const uint8_t *d_commits_is_inf, size_t n_commits,
                             size_t n_cells, const uint32_t *commit_index, const uint32_t *coset_index, const void *d_evals,
                             const void *d_proofs_xy, const uint8_t *d_proofs_is_inf, const void *d_weights, void *stream, int *accepted);
int zkp_kzg_cells_aggregate_dev(const zkp_kzg_cell_verifier *v, size_t n_commits, size_t n_cells, const uint32_t *commit_index,
                                const uint32_t *coset_index, const void *d_evals, const void *d_weights, void *d_out_interp,
                                void *d_out_commit_weights, void *d_out_proof_scalars, void *stream);

/* ---- Evaluation-form KZG: commitments and openings of a batch of polynomials given by their VALUES on the domain, no transform ----
 * A row holds the n = 2^log_n values of a polynomial of degree < n on the roots of unity: position i holds the value at w^i
 * (ZKP_KZG_ORDER_NATURAL) or at w^bitrev(i) (ZKP_KZG_ORDER_BITREV, the order blobs are stored in), as n x 4 limbs in the Fr memory
 * form, used as given (values that are not canonical are reduced by the arithmetic).  With d_i = w^e(i) - z:
 *   f(z) = (1 - z^n) / n * sum_i f_i w^e(i) / d_i,    q_e(i) = (f_i - f(z)) / d_i,    proof = the MSM of q over the Lagrange-basis SRS;
 * for z = w^m in the domain f(z) = f at w^m and q_m = -w^(-m) sum_{j != m} q_j w^j.  The commitment is the MSM of the row itself.
 * Row p of every output is byte for byte what zkp_kzg_open(monomial_srs, coeffs_p, n, z_p) and zkp_kzg_commit(monomial_srs,
 * coeffs_p, n) return for the interpolant of row p.
 *
 * zkp_kzg_eval_opener_create: `lagrange` is BORROWED and must outlive the opener.  It is any single-device handle of at least n
 * points (plain, expanded or endomorphism-split) made by zkp_g1_bases_lagrange for the same log_n; that it really is that basis is
 * the caller's responsibility (nothing here can tell).  The opener lives on the bases' slot and owns a device workspace of about
 * 32 n (1 + 2 max_polys) bytes, refused with ZKP_E_NOMEM -- sizes in zkp_last_error(), nothing left allocated -- beyond the free
 * memory or ZKP_KZG_EVALS_MAX_BYTES.  ZKP_E_ARG: a null argument, log_n outside 1..24, an unknown order, max_polys outside 1..4096,
 * sharded bases; ZKP_E_SIZE: bases of fewer than n points.
 *
 * The calls take n_polys <= max_polys rows (more: ZKP_E_SIZE; none: ZKP_OK, the device is not touched), rows contiguous, and one
 * point per row (n_polys x 4 limbs).  Points (n_polys x 12 limbs, n_polys flag bytes; the identity has zero limbs and flag 1) and
 * values y_p = f_p(z_p) (n_polys x 4) come back to HOST memory, so the four commit / open entries BLOCK; the *_dev forms differ only
 * in where the rows and the points z live.  zkp_kzg_open_evals_field_dev is the field half alone: d_out_y (n_polys x 4) and
 * d_out_quotient (n_polys x n x 4, in NATURAL order whatever the opener's order) in device memory; it allocates nothing and does not
 * wait for the device.  There is no host path: without a device every entry is ZKP_E_DEVICE. */
#define ZKP_KZG_ORDER_NATURAL 0
#define ZKP_KZG_ORDER_BITREV  1   /* position i of a row holds the value at w^bitrev(i): the order blobs are stored in */
typedef struct zkp_kzg_eval_opener zkp_kzg_eval_opener;
int zkp_kzg_eval_opener_create(const zkp_bases *lagrange, unsigned log_n, int order, size_t max_polys, zkp_kzg_eval_opener **out);
void zkp_kzg_eval_opener_destroy(zkp_kzg_eval_opener *o);
int zkp_kzg_commit_evals_batch(const zkp_kzg_eval_opener *o, const uint64_t *evals, size_t n_polys, uint64_t *out_xy, uint8_t *out_is_inf);
int zkp_kzg_commit_evals_batch_dev(const zkp_kzg_eval_opener *o, const void *d_evals, size_t n_polys, void *stream, uint64_t *out_xy,
                                   uint8_t *out_is_inf);
int zkp_kzg_open_evals_batch(const zkp_kzg_eval_opener *o, const uint64_t *evals, size_t n_polys, const uint64_t *z, uint64_t *out_xy,
                             uint8_t *out_is_inf, uint64_t *out_y);
int zkp_kzg_open_evals_batch_dev(const zkp_kzg_eval_opener *o, const void *d_evals, size_t n_polys, const void *d_z, void *stream,
                                 uint64_t *out_xy, uint8_t *out_is_inf, uint64_t *out_y);
int zkp_kzg_open_evals_field_dev(const zkp_kzg_eval_opener *o, const void *d_evals, size_t n_polys, const void *d_z, void *d_out_y,
                                 void *d_out_quotient, void *stream);
/* ---- batched verification of point openings: any number of openings of any number of commitments, one pairing check ----
 * The device counterpart of zkp_kzg_batch_verify for what zkp_kzg_open, zkp_kzg_open_all and zkp_kzg_open_evals_batch hand out.
 * Opening i < n_openings claims f_m(z_i) = y_i for the commitment C_m, m = commit_index[i] < n_commits, with the proof W_i =
 * proofs_xy[i], the point z[i], the value y[i] and the weight r_i = weights[i] (each n_openings x 4 limbs, Fr memory form, used as
 * given: limbs that are not canonical are reduced by the arithmetic).  commit_index may be NULL: opening i then belongs to
 * commitment i and n_commits must equal n_openings (else ZKP_E_ARG); that is the shape of zkp_kzg_batch_verify.  The batch is
 * accepted iff
 *   e( sum_m (sum_{i: m_i = m} r_i) C_m + sum_i (r_i z_i) W_i - (sum_i r_i y_i) G , G_2 ) == e( sum_i r_i W_i , [s]_2 ),
 * the equation of zkp_kzg_verify summed with the weights: two Miller loops and one final exponentiation whatever n_openings.
 * Measured (profiles/kzg_verify_points.md): 34 ms for 1 .. 64 openings and 35 ms for 4096, 31 ms of it the host's pairing, against
 * 33 ms (N = 1), 35 ms (N = 4), 73 ms (N = 64) and 2.5 s (N = 4096) of zkp_kzg_batch_verify: slower by 1 ms at N = 1, level at 4.
 * THE WEIGHTS ARE THE CALLER'S RANDOMNESS (as r_primes of zkp_kzg_batch_verify and the weights of zkp_kzg_verify_cells): independent,
 * unpredictable to whoever made the openings, 128 bits are enough.  A weight of 0 drops its opening from the check; equal (or
 * otherwise related) weights let the errors of different openings cancel, so a batch with a wrong opening can be accepted.  An
 * opening may appear more than once; one proof shared by several openings is not supported (give it once per opening).
 * Everything before the pairings runs on the device: one lane per opening forms r_i z_i and r_i and adds r_i y_i up a tree, the
 * weights of a commitment are summed in chunks of 2^ZKP_KZG_CELLS_CHUNK_LOG openings (work per lane is bounded however the openings
 * are spread over the commitments), and both G1 sums are one batch of two MSMs over the n_commits + n_openings + 1 points
 * [C .., W .., G]: the generator term rides in that pass as one more point.  ALL commitments and proofs are validated on the
 * device first (canonical, on the curve, in G1; the kernels of zkp_g1_validate): the batched equation is unsound on points outside
 * G1, so this is not optional.  A bad point is ZKP_E_ARG and zkp_last_error() names the array ("commits" or "proofs"), the lowest
 * bad index and the status word "canonical", "curve" or "subgroup".  is_inf arrays may be NULL (no identity among them).
 * zkp_kzg_point_verifier_create: g2s_xy = [s]_2 is validated (ZKP_E_ARG); max_openings and max_commits in 1 .. 2^30, else
 * ZKP_E_ARG.  The verifier needs no SRS; it lives on the slot current at creation (zkp_set_device) and owns a workspace of about
 * 100 bytes per opening and 64 per commitment.  A workspace that does not fit is ZKP_E_NOMEM with the sizes in zkp_last_error() and
 * nothing left allocated.  No device: ZKP_E_DEVICE; there is no host path.
 * zkp_kzg_verify_points / _dev: a null argument is ZKP_E_ARG, n_openings > max_openings or n_commits > max_commits ZKP_E_SIZE, a
 * commitment index >= n_commits ZKP_E_ARG naming the opening -- all before anything is launched; n_openings == 0 accepts without
 * touching the device.  Both end in host pairings, so both BLOCK; the _dev form differs only in where its inputs live:
 * d_commits_xy, d_commits_is_inf, d_z, d_y, d_proofs_xy, d_proofs_is_inf and d_weights are memory of the verifier's device, the
 * index array stays HOST memory (the grouping is planned on the host).  Either form may allocate: the transient point handle of
 * the call, and the slot's MSM workspaces when they have to grow.  While profiling is on a call records the phases
 * "kzg_points_field", "kzg_points_points" (validation and the MSMs) and "kzg_points_pairing" (host), the last once per pairing check.
 * zkp_kzg_verify_points_find_bad / _dev: the same, and *first_bad = SIZE_MAX when the batch is accepted, else the lowest index
 * whose opening fails: the openings are bisected, always testing the lower half of the failing slice with the same weights and all
 * the commitments (one no opening of the slice names gets weight 0), in at most ceil(log2 n_openings) further pairing checks.  The
 * points are validated once for the whole batch.  (The index is exact for weights under which no failing slice cancels, the
 * condition the verdict itself rests on.)
 * zkp_kzg_points_aggregate_dev: the field half alone, exact to the bit, every word canonical: d_out_commit_weights (n_commits x 4
 * limbs) the sums of the weights per commitment, d_out_rz and d_out_r (n_openings x 4 each) r_i z_i and r_i, d_out_neg_sum (4) the
 * value -sum r_i y_i.  Same refusals.  It neither allocates nor waits for the device, except for the previous call's copy of the
 * index table out of the handle's staging buffer; calls on one handle are serialised with its slot.
 * zkp_kzg_verify_evals_batch_dev: the blob form.  Row p of d_evals (the rows zkp_kzg_open_evals_batch_dev takes, in the opener's
 * order) is opened at d_z[p]; no value is supplied: y_p = f_p(z_p) is formed by the opener's field half (z_p in the domain
 * included) and checked against commitment p and proof p with weight p.  The opener and the verifier must live on the same slot
 * (ZKP_E_ARG); n_polys beyond the opener's max_polys or the verifier's capacities is ZKP_E_SIZE.  Blocks. */
typedef struct zkp_kzg_point_verifier zkp_kzg_point_verifier;
int zkp_kzg_point_verifier_create(const uint64_t g2s_xy[24], size_t max_openings, size_t max_commits, zkp_kzg_point_verifier **out);
void zkp_kzg_point_verifier_destroy(zkp_kzg_point_verifier *v);
int zkp_kzg_verify_points(const zkp_kzg_point_verifier *v, const uint64_t *commits_xy, const uint8_t *commits_is_inf, size_t n_commits,
                          size_t n_openings, const uint32_t *commit_index, const uint64_t *z, const uint64_t *y, const uint64_t *proofs_xy,
                          const uint8_t *proofs_is_inf, const uint64_t *weights, int *accepted);
int zkp_kzg_verify_points_dev(const zkp_kzg_point_verifier *v, const void *d_commits_xy, const uint8_t *d_commits_is_inf, size_t n_commits,
                              size_t n_openings, const uint32_t *commit_index, const void *d_z, const void *d_y, const void *d_proofs_xy,
                              const uint8_t *d_proofs_is_inf, const void *d_weights, void *stream, int *accepted);
int zkp_kzg_verify_points_find_bad(const zkp_kzg_point_verifier *v, const uint64_t *commits_xy, const uint8_t *commits_is_inf,
                                   size_t n_commits, size_t n_openings, const uint32_t *commit_index, const uint64_t *z, const uint64_t *y,
                                   const uint64_t *proofs_xy, const uint8_t *proofs_is_inf, const uint64_t *weights, int *accepted,
                                   size_t *first_bad);
int zkp_kzg_verify_points_find_bad_dev(const zkp_kzg_point_verifier *v, const void *d_commits_xy, const uint8_t *d_commits_is_inf,
                                       size_t n_commits, size_t n_openings, const uint32_t *commit_index, const void *d_z, const void *d_y,
                                       const void *d_proofs_xy, const uint8_t *d_proofs_is_inf, const void *d_weights, void *stream,
                                       int *accepted, size_t *first_bad);
int zkp_kzg_points_aggregate_dev(const zkp_kzg_point_verifier *v, size_t n_commits, size_t n_openings, const uint32_t *commit_index,
                                 const void *d_z, const void *d_y, const void *d_weights, void *d_out_commit_weights, void *d_out_rz,
                                 void *d_out_r, void *d_out_neg_sum, void *stream);
int zkp_kzg_verify_evals_batch_dev(const zkp_kzg_point_verifier *v, const zkp_kzg_eval_opener *o, const void *d_evals, size_t n_polys,
                                   const void *d_z, const void *d_commits_xy, const uint8_t *d_commits_is_inf, const void *d_proofs_xy,
                                   const uint8_t *d_proofs_is_inf, const void *d_weights, void *stream, int *accepted);

/* ---- Pairing-product checks on the GPU: many independent checks per launch, a verdict byte per check (csrc/pairing.hpp).
 * Every verifier above ends in ONE pairing check on the host; a verdict per item -- which openings of a rejected batch are bad,
 * which of many independent proofs fail -- is thousands of independent checks, one lane each here.  Check c is accepted iff
 * prod_j e(P[c][j], Q_j) == 1 over k FIXED G2 points Q_j (G_2, [s]_2, ...): their Miller walks are done once, on the host, at
 * creation (68 line steps per point, 13056 bytes), so the device does no G2 arithmetic.  Two kernels: the Miller product of a
 * check (its k Miller functions share their squarings), then the final exponentiation E(f) = f^(3 (p^12 - 1) / r) by the x-chain.
 * THE VALUE IS THE CUBE OF zkp_pairing's (gcd(3, r) = 1: E == 1 iff the canonical pairing product is 1, so every verdict is the
 * canonical one; zkp_pairing keeps the plain exponent and its pinned value).  One lane per check: a single device check is slower
 * than the host's (profiles/pairing_dev.md) and the verifiers above keep their host check -- this is for many checks at once.
 * zkp_pairing_checker_create: k in 1 .. 8 (else ZKP_E_ARG), each point validated as [s]_2 is everywhere (canonical, on the twist,
 * in G2: ZKP_E_ARG naming the slot) unless g2_is_inf (nullable, k flags) marks it as the identity; max_checks in 1 .. 2^24.  The
 * checker lives on the slot current at creation and owns the prepared lines and 576 bytes per check; a workspace that does not
 * fit is ZKP_E_NOMEM with the sizes in zkp_last_error() and nothing left allocated.
 * zkp_pairing_check_batch_dev: d_p_xy holds n_checks x k x 12 limbs (check-major), d_p_is_inf (nullable) n_checks x k flags.  A
 * pair whose P is the identity, or whose Q was created as the identity, contributes nothing (a check with no live pair is
 * accepted).  validate != 0 runs the kernels of zkp_g1_validate over all n_checks x k points first and synchronises: a bad point
 * is ZKP_E_ARG and zkp_last_error() names the lowest flat index, its check and pair, and the status word "canonical", "curve" or
 * "subgroup".  validate == 0: garbage in, garbage verdict, never a fault (no index and no trip count depends on the data).
 * d_ok (n_checks bytes, 1 / 0) and d_out_fq12 (n_checks x 72 limbs: E in zkp_pairing's memory order, canonical residues) are
 * each nullable, not both.  Does not synchronise unless validate != 0; allocates nothing.  n_checks == 0 does nothing;
 * n_checks > max_checks is ZKP_E_SIZE.  While profiling is on a call records "pairing_miller" and "pairing_final_exp".
 * zkp_pairing_check_batch: the same from host arrays through the slot's staging buffer; blocks. */
typedef struct zkp_pairing_checker zkp_pairing_checker;
int zkp_pairing_checker_create(const uint64_t *g2_xy /* k x 24 */, const uint8_t *g2_is_inf, size_t k, size_t max_checks,
                               zkp_pairing_checker **out);
void zkp_pairing_checker_destroy(zkp_pairing_checker *c);
int zkp_pairing_check_batch_dev(const zkp_pairing_checker *c, const void *d_p_xy, const uint8_t *d_p_is_inf, size_t n_checks,
                                int validate, uint8_t *d_ok, void *d_out_fq12, void *stream);
int zkp_pairing_check_batch(const zkp_pairing_checker *c, const uint64_t *p_xy, const uint8_t *p_is_inf, size_t n_checks, int validate,
                            uint8_t *ok, uint64_t *out_fq12);
/* A verdict PER OPENING on the point verifier: the arguments of zkp_kzg_verify_points without weights.  ok[i] = 1 iff opening i alone
 * verifies,  e(C_m(i) + [z_i]W_i - [y_i]G, G_2) * e(-W_i, [s]_2) == 1;  *n_bad (nullable) receives the number of zeros.  One lane per
 * opening forms the left point (two variable-base multiplications by the lane routine of zkp_g1_scale_dev, complete additions, one
 * inversion per lane) and the verifier's own pairing checker over (G_2, [s]_2) judges every pair; that checker and a workspace of
 * about 1 KiB per opening are made on the FIRST call, so creating a verifier costs what it did, and the workspace grows with the
 * largest call (ZKP_E_NOMEM with the sizes when it does not fit).  No value visits the host before the verdict bytes.  The points
 * are validated as zkp_kzg_verify_points validates them (a bad point: ZKP_E_ARG naming the array, the lowest index and the status
 * word) and the refusals are the same; more than 2^24 openings in one call is ZKP_E_SIZE.  n_openings == 0 touches nothing
 * (*n_bad = 0).  Both forms BLOCK (the count comes back); in the _dev form everything but commit_index (host) is memory of the
 * verifier's device and d_ok receives n_openings bytes.  While profiling is on a call records "kzg_each_points", "pairing_miller"
 * and "pairing_final_exp". */
int zkp_kzg_verify_points_each(const zkp_kzg_point_verifier *v, const uint64_t *commits_xy, const uint8_t *commits_is_inf,
                               size_t n_commits, size_t n_openings, const uint32_t *commit_index, const uint64_t *z, const uint64_t *y,
                               const uint64_t *proofs_xy, const uint8_t *proofs_is_inf, uint8_t *ok, size_t *n_bad);
int zkp_kzg_verify_points_each_dev(const zkp_kzg_point_verifier *v, const void *d_commits_xy, const uint8_t *d_commits_is_inf,
                                   size_t n_commits, size_t n_openings, const uint32_t *commit_index, const void *d_z, const void *d_y,
                                   const void *d_proofs_xy, const uint8_t *d_proofs_is_inf, uint8_t *d_ok, size_t *n_bad, void *stream);
/* How many host pairing checks have ended in the x-chain final exponentiation (out[0]) and in the plain power (out[1]) since the
 * library was loaded: what ZKP_PAIRING_FINAL_EXP chose, for the test suite. */
int zkp_selftest_final_exp_counts(uint64_t out[2]);
/* Self-test hooks for the device tower under the checks (csrc/pairing_tower.hpp over the saturated Fq), one lane per case, raw ABI
 * limbs in and out: d_a, d_b and d_out hold n x 72 limbs (an Fq12 in zkp_pairing's memory order, canonical residues); d_out must not
 * be an operand.  op: 0 a * b, 1 a^2, 2 the sparse product a * line with the line read from b as (A, B, C) = (b.c0.c0, b.c0.c1,
 * b.c1.c1.c0), 3 1 / a (0 -> 0), 4 / 5 / 6 the Frobenius maps a^p, a^(p^2), a^(p^3), 7 Granger-Scott cyclotomic squaring (the square
 * only inside the cyclotomic subgroup), 8 E(a).  d_b is read by 0 and 2 only.  At most 2^24 cases.
 * zkp_selftest_miller_dev: the value of the Miller kernel BEFORE the final exponentiation, n_checks x 72 limbs: bit for bit the
 * product over j of the model's miller_loop(P[c][j], Q_j).  Arguments as zkp_pairing_check_batch_dev. */
int zkp_selftest_fq12_dev(int op, const void *d_a, const void *d_b, size_t n, void *d_out, void *stream);
int zkp_selftest_miller_dev(const zkp_pairing_checker *c, const void *d_p_xy, const uint8_t *d_p_is_inf, size_t n_checks,
                            void *d_out_fq12, void *stream);
/* Self-test hook for the two device inversions of Fr (csrc/fr_inv.hpp, csrc/plonk.hpp): inverts n elements in device memory, one lane
 * each, 8 x u32 words in and out (the memory form, Montgomery radix 2^256).  method 0: Bernstein-Yang division steps, any value
 * below 2r in; method 1: the Fermat power.  Canonical a^-1 R out; 0 (and r, method 0) map to 0.  At most 2^24 elements. */
int zkp_selftest_fr_inverse_dev(const void *d_in, size_t n, int method, void *d_out, void *stream);

/* ---- single scalar multiplication: KzgScheme::commit_para, kzg/src/scheme.rs:78-82 (`g1_0.mul(para)`),
 *      6x per proof at plonk/src/prover.rs:183-188.  Serial by nature: computed on the host. ---- */
int zkp_g1_mul(const uint64_t base_xy[12], uint8_t base_is_inf, const uint64_t scalar[4], uint64_t out_xy[12],
               uint8_t *out_is_inf);
/* P_i = k_i * G for n scalars (fixed-base, on the GPU): Srs::new_from_secret, kzg/src/srs.rs:48-63, with
 * k_i = s^i, and the benchmark's base-point generator.  Output n x 12 limbs to device memory; d_out_is_inf
 * (nullable, n bytes) receives 1 where k_i == 0 (coordinates are then written as zeros). */
int zkp_g1_fixed_base_mul_dev(const void *d_scalars, size_t n, void *d_out_xy, uint8_t *d_out_is_inf, void *stream);
/* Self-test hook for the device field inversion used by the two entries above and by zkp_g1_bases_precompute (`into_affine` of
 * kzg/src/scheme.rs:92-93 on the GPU: Bernstein-Yang division steps, csrc/fq28_inv.hpp): inverts n raw base-field elements in device
 * memory, one lane each.  form 0: 12 x u32 limbs per element, Montgomery radix 2^384 (the arkworks form), any value below 2p in,
 * canonical a^-1 R out; form 1: the library's internal 14 x 28-bit limbs (+ 2 pad words = 64 B per element), Montgomery radix 2^392,
 * any value below 2p in, a^-1 R below 2p out.  0 maps to 0.  Not part of the hot path. */
int zkp_selftest_fq_inverse_dev(const void *d_in, size_t n, int form, void *d_out, void *stream);
/* Self-test hooks for the device field and curve primitives everything above is built from (csrc/selftest.hpp): one lane per case, raw
 * limbs in and out, no conversion; the tests compare the output words with an exact limb model at the edges of each primitive's operand
 * contract (tests/test_gpu_field_selftest.py).  Not part of the hot path; the operation numbers are the enums of csrc/selftest.hpp.
 * Field families: d_in holds n records of 4 operand slots x 16 words (256 B per case), d_out receives n records of 2 result slots x 16
 * words (128 B per case, unused words zero); an operand fills the first words of its slot.  d_out must not be d_in.
 *   zkp_selftest_fq28_dev  14 x 28-bit limbs, radix 2^392: the six product forms (0 fq28_mul_inline, 1 fq28_mul_chain, 2 fq28_mul_chain2
 *                          = two products, 3 sqr, 4 fq28_sqr_chain, 5 fq28_mul2, 6 fq28_mul2_chain), 7 normalise, 8 sub4, 9 sub8, 10 sub16,
 *                          11 sub8w, 12 neg4, 13 tight_is_zero_mod_p (word 0), 14 fq28_from_sat (12 words in), 15 fq28_mul_chain2_inplace
 *                          = the two products of 2, each written over its first operand
 *   zkp_selftest_fr29_dev  9 x 29-bit limbs, radix 2^261: 0 operator*, 1 fr29_mul2 = two products, 2 fr29_to_canonical (8 words out),
 *                          3 the memory-form Fr operator* (8 words in and out), 4 sub_tight, 5 sub_wide8, 6 normalise, 7 fr29_pack_tight,
 *                          8 fr29_from_sat_shl5, 9 fr29_twiddle_from_mont, 10 fr29_from_sat
 *   zkp_selftest_fp_dev    saturated Montgomery form, field 0 = Fq (12 words), 1 = Fr (8 words): 0 +, 1 -, 2 neg, 3 dbl, 4 operator*
 *                          (Fq: the out-of-line product), 5 mont_mul
 *   zkp_selftest_gl_dev    Goldilocks, 2 words: 0 +, 1 -, 2 neg, 3 *, 4 gl_reduce128(lo = slot 0, hi = slot 1)
 * G1 (zkp_selftest_g1_dev): points are raw limbs, 4 coordinates (X, Y, ZZ, ZZZ; an affine point: x, y) of 16 words.  Operations 0..6
 * (0 / 1 g1_28_madd plain / asm chains, 2 / 3 g1_28_mmadd likewise, 4 g1_28_add, 5 g1_28_double, 6 g1_28_double_affine) take point i at
 * byte 256 i of each array, and d_out may be d_a; operations 7..12 (7 / 8 g1_28_add_stream plain / chains, 9 / 10
 * g1_28_add_stream_inplace, 11 g1_28_add_quad, 12 the same with dst = srcA) take the plane-major layout of the bucket arrays, 16-byte
 * chunk q of point i at byte 16 (q stride + i), stride >= n; the in-place forms read their first operand from d_out (d_a is not used)
 * and the quad forms run four lanes per case.  d_flag receives one word per case: the return value of mmadd, result.is_inf() for the
 * other operations 0..6, zero otherwise. */
int zkp_selftest_fq28_dev(int op, const void *d_in, size_t n, void *d_out, void *stream);
int zkp_selftest_fr29_dev(int op, const void *d_in, size_t n, void *d_out, void *stream);
int zkp_selftest_fp_dev(int field, int op, const void *d_in, size_t n, void *d_out, void *stream);
int zkp_selftest_gl_dev(int op, const void *d_in, size_t n, void *d_out, void *stream);
int zkp_selftest_g1_dev(int op, const void *d_a, const void *d_b, size_t n, size_t stride, void *d_out, void *d_flag, void *stream);
/* The scalar split of the endomorphism-split MSM (glv_split of csrc/glv.hpp, the function the digit recoding calls), one lane per case:
 * d_scalars holds n Fr in memory form (Montgomery, 8 words), d_out receives 8 words per case, k1 = k mod lambda then k2 = k div lambda,
 * canonical, low word first. */
int zkp_selftest_glv_split_dev(const void *d_scalars, size_t n, void *d_out, void *stream);
/* Self-test hooks for the polynomial layer under the PLONK prover, zkp_kzg_open and Nova's openings (csrc/plonk.hpp: the three-launch
 * scan, fr_scale_pow_kernel, the division by (X - z), fr_poly_eval_kernel, fr_lincomb_kernel, fr_trim_len_kernel).  Host code only: each
 * hook calls the host helper the prover calls (csrc/plonk_host.inc), which launches the kernels the prover launches, on the caller's
 * buffers and stream; scratch comes from the slot's staging buffer.  Vectors are Fr in memory form (Montgomery, 4 x u64) in device memory,
 * at most 2^22 elements each (ZKP_E_SIZE beyond); scalars (z, base, s) are host Fr in the same form.  The arrays d_in, d_out, n, ... are
 * host arrays with one entry per job.  A null pointer that would be read or written, a count or a chunk out of range and an output that
 * overlaps an input it may not overlap are refused with ZKP_E_ARG before anything is enqueued.  `chunk` = 0 takes the elements per thread
 * the production rule picks for the longest vector of the call; any other value forces it (the prover never does).  Not part of the hot
 * path (tests/test_gpu_poly_primitives.py).
 *   zkp_selftest_poly_scan_dev        count = 1 or 2 jobs of one operator (op 0: +, 1: *): flags[j] bit 0 = from the top index down
 *                                     (suffix scan), bit 1 = exclusive: d_out[j][i] = op of d_in[j][k] over k <= i (< i when exclusive; >= i,
 *                                     > i for a suffix scan), the empty operation being 0 or 1.  chunk 1..16.  d_out[j] may be d_in[j];
 *                                     no other overlap.  (run_scan_batch)
 *   zkp_selftest_poly_scale_pow_dev   d_out[i] = d_in[i] * base^(i + e0).  chunk 1..8.  d_out may be d_in.  (scale_pow_params and the grid
 *                                     of the division)
 *   zkp_selftest_poly_div_linear_dev  count = 1 or 2 requests: d_out[j] receives the len[j] - 1 coefficients of (c_j(X) - c_j(z_j)) / (X - z_j),
 *                                     q_k = sum_{i > k} c_i z^(i - k - 1); z = count x 4 words.  len <= 1 writes nothing.  chunk 1..8, for the
 *                                     scaling and the scan alike.  A quotient may not overlap a dividend.  (div_linear_batch_dev)
 *   zkp_selftest_poly_eval_dev        count <= 8 requests: out (host, count x 4 words) receives c_j(z_j); len 0 gives 0.  Returns after the
 *                                     stream has finished this work.  (eval_many_dev)
 *   zkp_selftest_poly_lincomb_dev     d_out[i] = sum_k s_k d_p[k][i] over the terms with i < len[k], i < n_out; terms <= 12, s = terms x 4
 *                                     words.  d_out may be one of the d_p[k].  (lincomb_dev)
 *   zkp_selftest_poly_trim_len_dev    *out_len = the highest index of a non-zero element of d_c[0..n) plus one, 0 if there is none.  Returns
 *                                     after the stream has finished this work.  (the launch of trim_len_dev) */
int zkp_selftest_poly_scan_dev(int op, size_t count, const void *const *d_in, void *const *d_out, const size_t *n, const unsigned *flags,
                               unsigned chunk, void *stream);
int zkp_selftest_poly_scale_pow_dev(const void *d_in, size_t n, const uint64_t base[4], uint64_t e0, unsigned chunk, void *d_out,
                                    void *stream);
int zkp_selftest_poly_div_linear_dev(size_t count, const void *const *d_c, const size_t *len, const uint64_t *z, void *const *d_out,
                                     unsigned chunk, void *stream);
int zkp_selftest_poly_eval_dev(size_t count, const void *const *d_c, const size_t *len, const uint64_t *z, uint64_t *out, void *stream);
int zkp_selftest_poly_lincomb_dev(size_t terms, const void *const *d_p, const size_t *len, const uint64_t *s, size_t n_out, void *d_out,
                                  void *stream);
int zkp_selftest_poly_trim_len_dev(const void *d_c, size_t n, size_t *out_len, void *stream);
/* Self-test hook for the MSM's digit recoding and counting sort (csrc/msm.hpp: msm_digits*, msm_parthist, msm_partprefix, msm_partstart,
 * msm_partscatter<TILE>, msm_binsort, msm_rank, msm_order).  Plans the MSM of `count` resident scalar vectors of n scalars over `bases`
 * exactly as zkp_msm_g1_batch_dev does, sizes the same workspaces, fills the sort outputs of scalar range `range_index` with 0xFF bytes,
 * runs that range's digits + sort through the launch function the MSM itself uses, and stops: no accumulate, no reduction.  *geom receives
 * the geometry the kernels were given and, in out_words, the 32-bit words of every output below.  out == NULL: only *geom is filled and
 * nothing is launched (the caller sizes its buffers with it).  Otherwise every out->d_out[k] is a device buffer of out->words[k] >=
 * geom->out_words[k] words that receives, with W = nwin and every array window-major (window w first):
 *   ZKP_SORT_DIGITS    W x n         the digits, (|d| << 1) | (d < 0), 0 = skip; laid out [msm or scalar half][slice][scalar of the range]
 *   ZKP_SORT_ENTRIES   W x n x 2     first pass: (index | sign << 31, (bucket - 1) & (2^lo_bits - 1)), partition hi = (bucket - 1) >> lo_bits
 *                                    at [pstart[hi], pstart[hi + 1]); words past pstart[nhi] untouched (0xFF)
 *   ZKP_SORT_PSTART    W x (nhi+1)   exclusive prefix of the partition sizes
 *   ZKP_SORT_GHIST     W x 256       ghist[255 - min(size, 255)] = buckets of that size class
 *   ZKP_SORT_START     W x (nb+2)    start[0] = 0, start[b] = first sorted position of bucket b = 1..nb, start[nb + 1] = non-zero digits
 *   ZKP_SORT_SORTED    W x n         index | sign << 31 in bucket order; words past start[nb + 1] untouched
 *   ZKP_SORT_PERM      W x nb        the buckets by non-increasing min(size, 255)
 *   ZKP_SORT_OVER      W x 2         {candidates n_over = buckets with min(size, 255) > min(run_limit, 254), pieces}
 *   ZKP_SORT_OVER_B    W x over_cap  over_b[r] = perm[r], r < n_over; the rest untouched
 *   ZKP_SORT_OVER_OFF  W x (over_cap+1)  first piece of candidate r (a candidate of size <= run_limit has none), [n_over] = pieces
 *   ZKP_SORT_DESC      W x desc_cap x 4  piece j = {bucket, piece index p, start[b] + p piece, min(that + piece, start[b + 1])}
 * Refused: null bases / geom / scalar pointers (ZKP_E_ARG), more scalars than bases (ZKP_E_SIZE), a range index past the plan and an
 * output that is null or too small (ZKP_E_ARG).  Returns without waiting for the stream.  Not part of the hot path
 * (tests/test_gpu_msm_sort.py, tests/model/msm_sort_model.py). */
enum { ZKP_SORT_DIGITS = 0, ZKP_SORT_ENTRIES, ZKP_SORT_PSTART, ZKP_SORT_GHIST, ZKP_SORT_START, ZKP_SORT_SORTED, ZKP_SORT_PERM,
       ZKP_SORT_OVER, ZKP_SORT_OVER_B, ZKP_SORT_OVER_OFF, ZKP_SORT_DESC, ZKP_SORT_OUTPUTS };
typedef struct {
    uint32_t c, nwin, nb, nslice;        /* widest slice in bits, sort windows W, buckets per window 2^(c-1), slices per scalar */
    uint32_t shared, glv, nchunk, lo_bits, nhi, run_limit, piece, over_cap, desc_cap, ps_tile;
    uint32_t nranges, range_index;       /* scalar ranges of the plan, and the one that ran */
    uint64_t n, ns, chunk;               /* entries per sort window, scalars of this range, entries per chunk of the first pass */
    uint64_t range_off, range_len;       /* first scalar and scalars of this range */
    uint64_t out_words[ZKP_SORT_OUTPUTS];
    uint16_t off[36];                    /* bit offset of every slice, off[nslice] >= the bits covered */
} zkp_msm_sort_geometry;
typedef struct {
    void *d_out[ZKP_SORT_OUTPUTS];
    size_t words[ZKP_SORT_OUTPUTS];      /* capacity of each buffer in 32-bit words */
} zkp_msm_sort_outputs;
int zkp_selftest_msm_sort_dev(const zkp_bases *bases, const void *const *d_scalars, size_t count, size_t n, size_t range_index, void *stream,
                              zkp_msm_sort_geometry *geom, const zkp_msm_sort_outputs *out);
/* The same hook over the plan and the digits kernel of the bounded entries (zkp_msm_g1_batch_bits_dev with this `bits`): *geom shows the
 * slices the bound leaves (nslice, n, nwin, glv), the digits are those of the truncated offset table.  bits outside 1..256 is ZKP_E_ARG,
 * bits >= 255 is the hook above.  With out != NULL and bits < 255 it synchronises `stream` before it returns; a scalar past the bound
 * is not reported here. */
int zkp_selftest_msm_sort_bits_dev(const zkp_bases *bases, const void *const *d_scalars, size_t count, size_t n, size_t range_index,
                                   unsigned bits, void *stream, zkp_msm_sort_geometry *geom, const zkp_msm_sort_outputs *out);
/* Self-test hook for the MSM's bucket reduction (csrc/msm.hpp: msm_combine, msm_fold_parts, msm_fold_parts_lane, msm_pyramid,
 * msm_pyramid_quad, msm_pyramid_tail, msm_collect).  No bases, no scalars, no sort: the caller names the window width c (2..24), the
 * bucket sets nwin and split_log (0..2) and supplies the bucket contents; the hook runs, on the workspaces of device slot `slot` (< 0: the
 * thread's), what an MSM runs behind its accumulate, through the launch functions and plans the MSM itself uses (plan_fold, plan_reduce, the
 * combine grid of acc_launch): the combine if in->d_over is given, the fold steps, the reduction.  It zeroes the barrier counters of the
 * last-levels launch, which the sort does in an MSM.  Before the caller's data goes in, the second pyramid buffer, both odd buffers, the pinned
 * result and whatever the bucket workspace holds past nwin sets are filled with 0xFF bytes, so that a result that read an entry no launch wrote
 * is no stored point.  Layouts, with nb = 2^(c-1), cap = nwin x nb, a point = 64 words (X, Y, ZZ, ZZZ of 16 words each, csrc/g1_28.hpp):
 *   plane-major  16 planes of cap uint4; bucket b = 1..nb of set w is entry w nb + pyr_pos(b - 1, nb), pyr_pos(i, n) = (i >> 1) + (i & 1)(n >> 1)
 *   entry-major  64 consecutive words per point
 *   d_buckets    plane-major, cap entries                       d_parts    2^split_log - 1 such arrays back to back (NULL for split_log 0)
 *   d_over       nwin x 2: {candidates, pieces} per set         d_over_b   nwin x over_cap: the bucket id of candidate r
 *   d_over_off   nwin x (over_cap + 1): first piece of candidate r, [candidates] = pieces; a candidate with no piece is left alone
 *   d_pieces     entry-major, nwin x desc_cap                   d_carry    entry-major, cap entries at the buckets' positions (resume only)
 * resume != 0: the combine adds the carry entry to a combined bucket.  more != 0: it writes the combined buckets to the hand-over array (entry-
 * major, cap entries) instead of the buckets; the hook then stops, copies that array to d_out_carry and leaves out_results / out_flags alone.
 * d_out_buckets (nullable): the bucket array behind combine and fold, before the first pyramid launch.  out_results (host): nwin x c points
 * entry-major, [w][0] = the sum of the set's buckets, [w][1 + j] = U_j = the sum of the buckets whose 0-based index has bit j set;
 * out_flags (host): nwin words, a set's barrier counter as the last-levels launch left it -- tail_blocks arrivals for each of its c - 1 - nlevel
 * levels, bit 31 set when a workgroup gave up waiting -- and 0 from msm_collect.  *geom receives the shape of every launch and the words of every
 * buffer.  out_results == NULL: only *geom is filled and nothing is launched.  Returns after the results have arrived (more: after the stream
 * has finished); ZKP_E_DEVICE when the last-levels launch timed out, as the MSM reports it.  With a combine block the hook first waits for
 * `stream` and reads d_over and d_over_b back: more candidates than over_cap or a bucket id outside 1..nb is refused, not launched.
 * Refused (ZKP_E_ARG): null in / geom, c outside 2..24, nwin outside 1..65535 or cap >= 2^31, split_log > 2, a null or too-small buffer, d_over
 * with over_cap 0 or desc_cap 0 or nwin times either >= 2^24, resume / more without d_over, a ZKP_PYR_TAIL_* knob out of range (before
 * anything is enqueued).  Not part of the hot path
 * (tests/test_gpu_msm_reduce.py, tests/model/msm_reduce_model.py). */
typedef struct { uint32_t level, half, quad, grid_x; } zkp_msm_reduce_level;  /* grid (grid_x, level + 1, nwin); quad: four lanes per add */
typedef struct { uint32_t pairs, lane, grid_x; } zkp_msm_fold_step;           /* grid (grid_x, pairs); lane: one lane per add, else four */
typedef struct {
    uint32_t c, nwin, nb, split_log;
    uint32_t tail_max_waves;             /* waves of the last-levels launch this device keeps resident */
    uint32_t nlevel, tail_blocks, tail_threads;  /* levels 0..nlevel-1 as own launches, then (tail_blocks, nwin) x tail_threads; 0: msm_collect */
    uint32_t combine_x, over_cap, desc_cap, reserved;  /* combine grid (combine_x, nwin); 0 without a combine block */
    uint64_t cap;
    zkp_msm_reduce_level level[24];
    zkp_msm_fold_step fold[2];
    uint64_t bucket_words, parts_words, over_words, over_b_words, over_off_words, pieces_words, carry_words, result_words, flag_words;
} zkp_msm_reduce_geometry;
typedef struct {
    uint32_t c, nwin, split_log;
    uint32_t over_cap, desc_cap, resume, more, reserved;
    const void *d_buckets, *d_parts, *d_over, *d_over_b, *d_over_off, *d_pieces, *d_carry;
    size_t buckets_words, parts_words, over_words, over_b_words, over_off_words, pieces_words, carry_words;  /* 32-bit words of each */
    void *d_out_buckets, *d_out_carry;
    size_t out_buckets_words, out_carry_words;
    uint32_t *out_results, *out_flags;
    size_t out_results_words, out_flags_words;
} zkp_msm_reduce_io;
int zkp_selftest_msm_reduce_dev(int slot, const zkp_msm_reduce_io *in, void *stream, zkp_msm_reduce_geometry *geom);
/* [s^i]G for i < n into host memory (kzg/src/srs.rs:48-63: n = circuit_size + 3). */
int zkp_srs_g1(const uint64_t secret[4], size_t n, uint64_t *out_xy);

/* ---- NTT over Fr: ark-poly Radix2EvaluationDomain semantics as used by the reference --
 *      `Evaluations::interpolate` (plonk/src/prover.rs:374-375,463; plonk/src/circuit.rs:175,230-232) = inverse;
 *      the FFTs inside `&DensePolynomial * &DensePolynomial` (prover.rs:396-426,437) = forward + inverse.
 *      In place, natural order in and out, size 2^log_n (log_n <= 32 and fits memory).
 *      inverse != 0 scales by n^-1.  coset != NULL: forward scales coefficient j by coset^j first (coset_fft);
 *      inverse scales output j by coset^-j (coset_ifft). ---- */
int zkp_ntt_fr(uint64_t *data, unsigned log_n, int inverse, const uint64_t *coset /* nullable Fr */);
/* `batch` independent transforms of size 2^log_n stored back to back in device memory. */
int zkp_ntt_fr_dev(void *d_data, unsigned log_n, size_t batch, int inverse, const uint64_t *coset, void *stream);

/* Twiddle step of a four-step (multi-GPU) transform of total size 2^log_n: the rows x cols row-major block is multiplied
 * element-wise by omega_n^((row0 + r) * c) (omega_n^-1 when inverse != 0).  Used by zkp_hip/dist.py between the column and
 * row transforms, around the RCCL all-to-all transposes. */
int zkp_ntt_fr_twiddle_dev(void *d_data, size_t rows, size_t cols, size_t row0, unsigned log_n, int inverse, void *stream);

/* The two local halves of the four-step transform in the layouts the all-to-all exchanges produce, so that no transpose or
 * twiddle pass over the data is needed (zkp_hip/dist.py; BASELINE.json configs[4]):
 * zkp_ntt_fr_axis0_dev -- transforms of length 2^log_len (<= 2^16) along axis 0 of a row-major [2^log_len][cols] matrix (cols a
 *   power of two >= 4, the contiguous direction), natural order in and out, out-of-place or in place; when tw_log_n != 0
 *   output (k, b) is also multiplied by omega_{2^tw_log_n}^((tw_col0 + b) k) (omega^-1 and the 1/2^log_len factor when
 *   inverse).  The column transforms: the first all-to-all delivers [all rows n1][my columns].
 * zkp_ntt_fr_layout_dev -- `batch` transforms of size 2^log_n, natural order, out-of-place, reading a gathered input and/or
 *   writing a scattered output: with a layout, logical element e of transform b lives at element
 *       b * batch_stride + (e mod 2^lo_bits) + ((e >> lo_bits) mod 2^mid_bits) * mid_stride + (e >> (lo_bits + mid_bits)) * hi_stride
 *   (NULL = contiguous transforms, b * 2^log_n + e); when tw_log_n != 0 output k of transform b is multiplied by
 *   omega_{2^tw_log_n}^((tw_row0 + b) k).  The row transforms: the second all-to-all delivers [source rank][my rows][that
 *   rank's columns], possibly in several column chunks (mid field). */
typedef struct {
    unsigned lo_bits, mid_bits;
    size_t mid_stride, hi_stride, batch_stride; /* in elements */
} zkp_ntt_layout;
int zkp_ntt_fr_axis0_dev(const void *d_in, void *d_out, unsigned log_len, size_t cols, int inverse, unsigned tw_log_n,
                         size_t tw_col0, void *stream);
int zkp_ntt_fr_layout_dev(const void *d_in, void *d_out, unsigned log_n, size_t batch, int inverse,
                          const zkp_ntt_layout *in_layout, const zkp_ntt_layout *out_layout, unsigned tw_log_n, size_t tw_row0,
                          void *stream);

/* ---- The same transform spread over the device slots of ONE process (BASELINE configs[4]; the multi-GPU face of the
 *      GeneralEvaluationDomain call sites above: plonk/src/prover.rs:70,374-375,396-443, plonk/src/circuit.rs:170-176).
 *      Four-step decomposition N = N1 x N2 over G = zkp_device_count() slots (G a power of two; slots created by zkp_init_devices, which
 *      may list one device several times -- how a 1-GPU box runs this code): column transforms (zkp_ntt_fr_axis0_dev's kernels), an
 *      all-to-all, row transforms (zkp_ntt_fr_layout_dev's kernels), with the exchange done INSIDE the library as peer-to-peer block
 *      copies between the slots' devices (hipMemcpyPeerAsync, every slot pulling its G blocks on its own copy stream: all xGMI links of a
 *      device busy at once; plain device-to-device copies between slots that share a device).  The columns are cut into `chunks`
 *      groups that go through pack / exchange / column transform as a pipeline (the copies of group q + 1 run under the transforms of
 *      group q).  No collective library, no other process: one resident host thread per slot drives its device.
 *
 *      Geometry (zkp_ntt_fr_sharded_geometry): N1 = 2^log_n1 with log_n1 = max(min(8, ceil(log_n / 2)), log2 G), N2 = N / N1, r1 = N1 / G,
 *      r2 = N2 / G (>= 4, otherwise ZKP_E_ARG: the transform is too small for this many slots), cw = r2 / chunks (>= 4).
 *      Slot g holds N / G elements at d_slabs[g] (memory of slot g's device), in one of three layouts:
 *        ZKP_NTT_NATURAL   elements [g N/G, (g+1) N/G) of the vector, i.e. rows [g r1, (g+1) r1) of the row-major N1 x N2 matrix
 *        ZKP_NTT_K1SLAB    slab g [j][k2] = X[(g r1 + j) + N1 k2]: the transposed order a four-step transform leaves; pointwise
 *                          products between a forward and an inverse transform do not care, and an MSM does not either
 *        ZKP_NTT_COLUMNS   slab g [q][n1][c] = x[n1 N2 + g r2 + q cw + c], q < chunks, c < cw: the COLUMNS [g r2, (g+1) r2) of every row
 *                          (chunk-major; `chunks` is part of this layout)
 *      Supported (layout_in -> layout_out), each for inverse == 0 and != 0 (in place: the result overwrites d_slabs[g]):
 *        NATURAL -> K1SLAB   two exchanges        K1SLAB -> NATURAL   two exchanges (the mirror image)
 *        COLUMNS -> K1SLAB   ONE exchange         K1SLAB -> COLUMNS   ONE exchange
 *        NATURAL -> NATURAL  three exchanges (the order ark-poly's fft / ifft return)
 *      Reading "input in K1SLAB order" as index i = i1 + N1 i2 stored at [i1][i2], every pair is the full transform of that vector.
 *      chunks: 0 = automatic (4, fewer when r2 < 16); otherwise a power of two with r2 / chunks >= 4 (anything else is ZKP_E_ARG,
 *      never adjusted silently).
 *      streams: NULL -- the library launches on each slot's own stream after waiting for all work enqueued on that slot's device
 *      (hipDeviceSynchronize) and returns when every device has finished; or G hipStream_t (streams[g] on slot g's device): the work
 *      of slot g is enqueued on streams[g], ordered after what that stream already holds, and the call returns without waiting (the
 *      copy streams are joined back into streams[g] by events before the call returns).
 *      Workspace per slot: two slabs of exchange buffers + the transform's scratch slab.
 *      zkp_ntt_fr_sharded is the host-pointer form (natural order in and out, optional coset, like zkp_ntt_fr): every slot uploads and
 *      downloads its own slab over its own PCIe link.  zkp_ntt_fr itself takes this route when the library runs on more than one slot
 *      and log_n >= ZKP_NTT_SHARD_MIN_LOG (environment, default 24), so the Rust seam needs no change to use a whole node. ---- */
#define ZKP_NTT_NATURAL 0
#define ZKP_NTT_K1SLAB 1
#define ZKP_NTT_COLUMNS 2
typedef struct {
    unsigned slots, log_n1, log_n2, chunks;
    size_t r1, r2, cw, slab; /* rows / columns per slot, columns per chunk, elements per slot */
} zkp_ntt_shard_geometry;
int zkp_ntt_fr_sharded_geometry(unsigned log_n, unsigned slots /* 0 = zkp_device_count() */, unsigned chunks,
                                zkp_ntt_shard_geometry *out);
int zkp_ntt_fr_sharded_dev(void *const *d_slabs, unsigned log_n, int inverse, int layout_in, int layout_out, unsigned chunks,
                           void *const *streams);
int zkp_ntt_fr_sharded(uint64_t *data, unsigned log_n, int inverse, const uint64_t *coset /* nullable Fr */);

/* ---- NTT over Goldilocks: the evaluation loop of FriLayer::from_poly, fri/src/fri_layer.rs:40-46 ---- */
int zkp_ntt_goldilocks(uint64_t *data, unsigned log_n, int inverse, const uint64_t *coset /* nullable, 1 limb */);
int zkp_ntt_goldilocks_dev(void *d_data, unsigned log_n, size_t batch, int inverse, const uint64_t *coset, void *stream);
/* evals[i] = poly(coset * omega_D^i), i < D = 2^log_D, natural order (fri_layer.rs:40-46); d <= D coefficients. */
int zkp_fri_layer_eval(const uint64_t *coeffs, size_t d, uint64_t coset, unsigned log_D, uint64_t *out);
/* fold_polynomial, fri/src/prover.rs:34-42: out[j] = c[2j] + r*c[2j+1]; out has ceil(d/2) entries. */
int zkp_fri_fold(const uint64_t *coeffs, size_t d, uint64_t r, uint64_t *out);

/* ---- FRI commitment path around the NTT.  Field elements are Goldilocks memory-form limbs. ----
 * MerkleTree::new, fri/src/merkle_tree.rs:42-63, with hash / hash_slice of fri/src/hasher.rs:14-36 (SHA-256 over the
 * decimal strings, digest taken mod p as a little-endian integer).  `nodes` receives every level, concatenated: the n leaf
 * hashes, then ceil(n/2) parents, ... up to the root (zkp_fri_merkle_node_count(n) elements; the root is the last one). */
size_t zkp_fri_merkle_node_count(size_t n);
int zkp_fri_merkle_tree(const uint64_t *leaves, size_t n, uint64_t *nodes_out);
int zkp_fri_merkle_tree_dev(const void *d_leaves, size_t n, void *d_nodes, void *stream);
/* Transcript replay, fri/src/fiat_shamir/transcript.rs:30-139 as used by fri/src/verifier.rs:13-29: r_out[l] = the folding
 * challenge drawn after digesting root l (memory form); q_out[i] = the i-th query challenge as usize (before % domain),
 * drawn after digesting const_val.  Host only. */
int zkp_fri_challenges(const uint64_t *roots, size_t layers, uint64_t const_val, size_t num_queries, uint64_t *r_out,
                       uint64_t *q_out);
/* generate_proof, fri/src/prover.rs:141-168 (folding phase on the GPU: coset NTT + Merkle tree + fold per layer; query
 * decommitments gathered on the GPU).  *out_proof is a malloc'ed flat proof of *out_words words, layout:
 *   [0] domain_size [1] layers = log2(domain_size) [2] number_of_queries [3] coset (= 7)
 *   layers_root[layers], const_val, then per query, per layer l: index, evaluation, sym_evaluation,
 *   auth path (log2(domain_size >> l) sibling hashes from the leaf level up), sym auth path (same length).
 * Release with zkp_free.  A zero polynomial is ZKP_E_ARG (the reference's assert at prover.rs:72 panics). */
int zkp_fri_prove(const uint64_t *coeffs, size_t d, size_t blowup_factor, size_t num_queries, uint64_t **out_proof,
                  size_t *out_words);
/* verify, fri/src/verifier.rs:10-127, on the flat proof (host only).  ZKP_OK = accepted; ZKP_E_ARG otherwise, with the
 * reference's error string ("wrong index!", "verify Merkle path failed!", "folding wrong!") in zkp_last_error(). */
int zkp_fri_verify(const uint64_t *proof, size_t words);
void zkp_free(void *p);

/* ---- FRI over the BLS12-381 scalar field Fr (fri/src is generic over F: PrimeField; kzg::types::ScalarField) ----
 * Field elements are Fr memory form: uint64_t[4] Montgomery residues, as zkp_ntt_fr.  Same objects as the Goldilocks
 * entries above: Display is the canonical integer in decimal (up to 77 digits, zero prints as ""; ZKP_FRI_ZERO_AS_0=1
 * switches to "0" here too), a digest is reduced mod r as a 256-bit little-endian integer, F::GENERATOR = 7.
 * Node counts come from zkp_fri_merkle_node_count (elements, 4 words each).  zkp_fri_prove_fr runs the layers of at most 512
 * points in one workgroup (ZKP_FRI_FR_TAIL_LOG=0..10 moves that threshold for measurements; 0 = none); its phases are recorded
 * as "fri_merkle", "ntt_fr_pass", "fri_fold", "fri_transcript", "fri_tail" and "fri_gather". */
/* evals[i] = poly(coset * omega_D^i), i < D = 2^log_D (fri_layer.rs:40-46); coeffs d x 4 words, d <= D; out D x 4 words. */
int zkp_fri_layer_eval_fr(const uint64_t *coeffs, size_t d, const uint64_t coset[4], unsigned log_D, uint64_t *out);
/* fold_polynomial, fri/src/prover.rs:34-42: out[j] = c[2j] + r*c[2j+1]; out has ceil(d/2) elements. */
int zkp_fri_fold_fr(const uint64_t *coeffs, size_t d, const uint64_t r[4], uint64_t *out);
int zkp_fri_merkle_tree_fr(const uint64_t *leaves, size_t n, uint64_t *nodes_out);
int zkp_fri_merkle_tree_fr_dev(const void *d_leaves, size_t n, void *d_nodes, void *stream);
/* Transcript replay over Fr: r_out = layers x 4 words (memory form), q_out[i] = the i-th query challenge as usize (the low
 * limb of its canonical value, before % domain).  Host only. */
int zkp_fri_challenges_fr(const uint64_t *roots, size_t layers, const uint64_t const_val[4], size_t num_queries, uint64_t *r_out,
                          uint64_t *q_out);
/* generate_proof over Fr.  *out_proof is a malloc'ed flat proof of *out_words words, layout:
 *   [0] domain_size [1] layers = log2(domain_size) [2] number_of_queries
 *   then 4-word fields: coset (memory form of 7), layers_root[layers], const_val
 *   then per query, per layer l: index (1 word), evaluation (4), sym_evaluation (4),
 *   auth path (log2(domain_size >> l) sibling hashes from the leaf level up, 4 words each), sym auth path (same length).
 * Release with zkp_free.  A zero polynomial (after trimming trailing zeros) or blowup_factor == 0 is ZKP_E_ARG; a domain
 * above 2^32 (the two-adicity of Fr) is ZKP_E_SIZE. */
int zkp_fri_prove_fr(const uint64_t *coeffs, size_t d, size_t blowup_factor, size_t num_queries, uint64_t **out_proof,
                     size_t *out_words);
/* verify over Fr on the flat proof (host only); ZKP_OK = accepted, ZKP_E_ARG otherwise with the reference's error string. */
int zkp_fri_verify_fr(const uint64_t *proof, size_t words);

/* ---- ChallengeGenerator<Sha256>, plonk/src/challenge.rs:22-77 (host): feed commitments (serialize_uncompressed, 96
 *      bytes), then draw Fr challenges (memory form, n x 4 limbs) through StdRng::seed_from_u64 + Fr::rand.  Drawing twice
 *      without feeding is ZKP_E_ARG (the reference panics "I'm hungry! Feed me something first"). ---- */
typedef struct zkp_plonk_transcript zkp_plonk_transcript;
int zkp_plonk_transcript_create(zkp_plonk_transcript **out);
void zkp_plonk_transcript_destroy(zkp_plonk_transcript *t);
int zkp_plonk_transcript_feed(zkp_plonk_transcript *t, const uint64_t xy[12], uint8_t is_inf);
int zkp_plonk_transcript_challenges(zkp_plonk_transcript *t, size_t n, uint64_t *out);

/* ---- polynomial product with ark-poly `Mul` semantics (plonk/src/prover.rs:396-426): FFT-based on the radix-2
 *      domain of size next_pow2(la+lb-1); out has la+lb-1 entries; either operand empty gives an empty product ---- */
int zkp_poly_mul_fr(const uint64_t *a, size_t la, const uint64_t *b, size_t lb, uint64_t *out);

/* ---- PLONK prover rounds: plonk/src/prover.rs::generate_proof (61-293), one entry per round.  Blinders (the
 *      reference draws them from StdRng::from_entropy(), prover.rs:68-77,104-106) and Fiat-Shamir challenges (the
 *      reference's SHA-256 ChallengeGenerator, plonk/src/challenge.rs) are INPUTS: the caller keeps its transcript and
 *      feeds the returned commitments to it between rounds.  Polynomials stay in HBM between rounds.
 *      create: the CompiledCircuit (plonk/src/compiled_circuit.rs, constraint.rs) as 12 coefficient vectors of at most
 *      n = 2^log_n entries, in the order q_m q_l q_r q_o q_c pi f_a f_b f_c s_sigma_1 s_sigma_2 s_sigma_3, plus k1, k2
 *      (circuit.rs:238-245); the SRS must hold n + 3 points (kzg/src/srs.rs:51). ---- */
typedef struct zkp_plonk_prover zkp_plonk_prover;
int zkp_plonk_prover_create(const zkp_bases *srs, unsigned log_n, const uint64_t *const polys[12], const size_t lens[12],
                            const uint64_t k1[4], const uint64_t k2[4], zkp_plonk_prover **out);
void zkp_plonk_prover_destroy(zkp_plonk_prover *p);
/* Round 1 (prover.rs:68-92): b1..b6 -> commitments to a(X), b(X), c(X) (3 x 12 limbs, 3 infinity bytes). */
int zkp_plonk_round1(zkp_plonk_prover *p, const uint64_t *blinders, uint64_t *out_xy, uint8_t *out_is_inf);
/* Round 2 (prover.rs:98-123, compute_acc 302-377): beta, gamma, b7..b9 -> commitment to z(X). */
int zkp_plonk_round2(zkp_plonk_prover *p, const uint64_t beta[4], const uint64_t gamma[4], const uint64_t *blinders,
                     uint64_t out_xy[12], uint8_t *out_is_inf);
/* Round 3 (prover.rs:136-150, compute_quotient_polynomial 381-444, SlicePoly): alpha -> t_lo, t_mid, t_hi commitments and
 * the slice degree.  An unsatisfied circuit returns ZKP_E_ARG (the reference panics with "No remainder"). */
int zkp_plonk_round3(zkp_plonk_prover *p, const uint64_t alpha[4], uint64_t *out_xy, uint8_t *out_is_inf, size_t *out_degree);
/* Round 4 (prover.rs:156-178): zeta -> bar_a bar_b bar_c bar_s_sigma_1 bar_s_sigma_2 bar_z_w (6 x 4 limbs). */
int zkp_plonk_round4(zkp_plonk_prover *p, const uint64_t zeta[4], uint64_t *out_bars);
/* Round 5 (prover.rs:183-268, compute_linearisation_polynomial 469-568): v -> commitments to W_zeta, W_zeta_omega. */
int zkp_plonk_round5(zkp_plonk_prover *p, const uint64_t v[4], uint64_t *out_xy, uint8_t *out_is_inf);
/* generate_proof in ONE call, plonk/src/prover.rs:61-293: rounds 1-5 above driven by the reference's transcript
 * (ChallengeGenerator<Sha256>, plonk/src/challenge.rs; the six evaluations are fed as commit_para(bar), scheme.rs:78-82).
 * blinders = b1..b9 (the reference draws them from StdRng::from_entropy, prover.rs:66-75,103-105).  Field order of the
 * proof = struct Proof, prover.rs:23-41. */
typedef struct {
    uint64_t commit_xy[9][12]; /* a, b, c, z, t_lo, t_mid, t_hi, w_ev_x, w_ev_wx */
    uint8_t commit_is_inf[9];
    uint64_t bars[6][4];       /* bar_a, bar_b, bar_c, bar_s_sigma_1, bar_s_sigma_2, bar_z_w */
    uint64_t u[4];
    uint64_t degree;
} zkp_plonk_proof;
int zkp_plonk_prove(zkp_plonk_prover *p, const uint64_t *blinders, zkp_plonk_proof *out);

/* ---- Verifiers with real pairings (host code, never a throughput path: ~20 ms per pairing).
 *      G2 points in arkworks memory form: x.c0 x.c1 y.c0 y.c1, 4 x 6 Montgomery limbs; Fq12 = 12 x 6 limbs in tower order.
 *      The pairing value is the reduced optimal ate pairing with the plain exponent (p^12 - 1) / r; the reference only ever
 *      compares two values (kzg/src/scheme.rs:157-159,244; plonk/src/verifier.rs:151).
 *      The ABI is the deserialisation boundary (the reference only ever holds typed, validated arkworks points): every finite G1
 *      and G2 input of the entries below must have canonical limbs (< p), lie on its curve and in the prime-order subgroup
 *      ([r]P = O; both cofactors are large), otherwise the call fails with ZKP_E_ARG before any pairing runs. ---- */
int zkp_g2_generator(uint64_t out_xy[24]);
int zkp_g2_mul(const uint64_t q_xy[24], uint8_t q_is_inf, const uint64_t scalar[4], uint64_t out_xy[24], uint8_t *out_is_inf);
int zkp_pairing(const uint64_t p_xy[12], uint8_t p_is_inf, const uint64_t q_xy[24], uint8_t q_is_inf, uint64_t out_fq12[72]);
/* KzgScheme::verify, kzg/src/scheme.rs:143-160; g2s = [s]_2 (Srs::g2s, kzg/src/srs.rs:66).  *accepted = 1 / 0. */
int zkp_kzg_verify(const uint64_t g2s_xy[24], const uint64_t commit_xy[12], uint8_t commit_is_inf, const uint64_t w_xy[12],
                   uint8_t w_is_inf, const uint64_t y[4], const uint64_t z[4], int *accepted);
/* KzgScheme::batch_verify, kzg/src/scheme.rs:215-245; r_primes (n x 4 limbs) stand for Fr::from(rng.gen::<u128>()). */
int zkp_kzg_batch_verify(const uint64_t g2s_xy[24], size_t n, const uint64_t *commits_xy, const uint8_t *commits_is_inf,
                         const uint64_t *points, const uint64_t *openings_xy, const uint8_t *openings_is_inf,
                         const uint64_t *evals, const uint64_t *r_primes, int *accepted);
/* KzgScheme::aggregate_commitments, kzg/src/scheme.rs:187-202 (test: kzg/src/commitment.rs:78-89): sum_i challenge^i * C_i over n
 * commitments (n x 12 limbs; commits_is_inf nullable); host code, the points are validated like the verifiers' inputs. */
int zkp_kzg_aggregate_commitments(const uint64_t *commits_xy, const uint8_t *commits_is_inf, size_t n, const uint64_t challenge[4],
                                  uint64_t out_xy[12], uint8_t *out_is_inf);
/* verify, plonk/src/verifier.rs:19-157, against the circuit and SRS held by `p`: *accepted = 1 accepted, 0 "Pairing failed,
 * rejected", -1 "Challenge verification failed".  The eight circuit commitments and pi(zeta) are computed on the GPU. */
int zkp_plonk_verify(zkp_plonk_prover *p, const uint64_t g2s_xy[24], const zkp_plonk_proof *proof, int *accepted);

/* Parity accessor: copy a working polynomial to the host.  which: 0 ax 1 bx 2 cx 3 z 4 r 5 W_zeta 6 W_zeta_omega
 * 7 tx_compact 8 t (before round 5). */
int zkp_plonk_get_poly(zkp_plonk_prover *p, int which, uint64_t *out, size_t cap_elems, size_t *len);

/* ---- Circuit::compile (plonk/src/circuit.rs:166-245) on the device: the gate list to a resident prover, and a new witness
 *      for the same circuit.  The gates of circuit.rs as the caller holds them, struct of arrays, g = `gates` real gates (no
 *      dummies: pad_circuit adds those, and they are always trailing). ---- */
typedef struct {
    size_t gates;          /* g >= 2 */
    const uint32_t *pos;   /* g x 6: a_col a_row b_col b_row c_col c_row = Position::Pos(col, row), gate.rs */
    const uint64_t *sel;   /* g x 6 x 4 limbs: q_m q_l q_r q_o q_c pi AS STORED in Gate (pi already negated, gate.rs:53) */
    const uint64_t *vals;  /* g x 3 x 4 limbs: the a, b, c values of Circuit::vals */
} zkp_plonk_gates;
/* n = 2^((g - 1).ilog2() + 1) (pad_circuit, circuit.rs:148-157): g < 2 and log_n > 24 are ZKP_E_ARG, an SRS below n + 3 points
 * ZKP_E_SIZE, a sharded SRS ZKP_E_ARG.  The nine assignment columns hold the gate's selector or value in row i < g and zero
 * beyond (get_assignment skips dummies, interpolate zero-pads); sigma_j[i] = K_col w^row for the wire (col, row) of gate i
 * with K = (1, k1, k2), k1 = 2, k2 = 3 (find_cosets), and K_j w^i in the dummy rows (cal_permutation).  A col above 2 or a
 * row >= n is ZKP_E_ARG (the reference panics with "Invalid position" or indexes out of bounds), decided before any prover
 * exists.  The twelve inverse transforms run on the device; the prover is the one zkp_plonk_prover_create makes from the
 * same twelve coefficient vectors with k1 = 2, k2 = 3. */
int zkp_plonk_prover_create_from_gates(const zkp_bases *srs, const zkp_plonk_gates *gates, zkp_plonk_prover **out);
/* Another witness for a prover made by zkp_plonk_prover_create_from_gates (any other prover: ZKP_E_ARG): vals = g x 3 x 4
 * limbs, pi = g x 4 limbs as stored (nullable: the public inputs stay), gates = the g of creation (else ZKP_E_ARG).
 * Selectors, wiring and everything computed from them stay; the next proof starts at round 1.  A witness that does not
 * satisfy its gates is reported by round 3 / zkp_plonk_prove ("No remainder expected"), and a later good one proves again.
 * _dev: device pointers (16-byte aligned), read on `stream`; the call returns when the device work is done. */
int zkp_plonk_prover_set_witness(zkp_plonk_prover *p, const uint64_t *vals, const uint64_t *pi, size_t gates);
int zkp_plonk_prover_set_witness_dev(zkp_plonk_prover *p, const void *d_vals, const void *d_pi, size_t gates, void *stream);
/* Parity accessor: the n coefficients (zero-padded) of circuit polynomial `which`, 0..11 in the order of
 * zkp_plonk_prover_create.  `out` receives min(cap_elems, n) coefficients; *len = n. */
int zkp_plonk_get_circuit_poly(zkp_plonk_prover *p, int which, uint64_t *out, size_t cap_elems, size_t *len);
int zkp_plonk_prover_info(const zkp_plonk_prover *p, unsigned *log_n, uint64_t k1[4], uint64_t k2[4]);

/* ---- Nova folding (NIFS) over a sparse R1CS: nova/src/nifs/mod.rs, nifs_prover.rs, nifs_verifier.rs, r1cs/mod.rs.
 *      R1CS (r1cs/mod.rs:9-16): A, B, C with `rows` rows over z = (W || x || u), |W| = num_vars, |x| = num_io, so columns
 *      0..num_vars+num_io.  The reference holds dense ragged rows (utils.rs:14-22: an entry beyond a row's length is zero); here each
 *      matrix is host CSR: row_ptr (rows + 1 entries, row_ptr[0] = 0, non-decreasing), cols (row_ptr[rows] column indices) and vals
 *      (row_ptr[rows] Fr, Montgomery).  Duplicate (row, column) entries add up and explicit zeros are kept, as in the dense sum.
 *      ZKP_E_ARG for a null pointer, rows == 0, num_vars == 0, a column >= num_vars + num_io + 1, a row_ptr that does not start at 0
 *      or decreases, or an SRS sharded over several slots (the handle is single-slot, like the PLONK prover: it lives on the SRS's
 *      device).  z is never materialised: column c reads W[c] (c < num_vars), x[c - num_vars], or u (the last column), so a
 *      resident W is used in place.  E and T have `rows` entries, W has num_vars.  Rows are split at create time: rows with at most
 *      64 entries in A, B and C together run one lane per row, longer ones one wave per row. ---- */
typedef struct zkp_nova_r1cs zkp_nova_r1cs;
typedef struct {
    const uint64_t *row_ptr; /* rows + 1 */
    const uint32_t *cols;    /* row_ptr[rows] */
    const uint64_t *vals;    /* row_ptr[rows] x 4 limbs */
} zkp_csr;
int zkp_nova_r1cs_create(const zkp_bases *srs, size_t rows, size_t num_vars, size_t num_io, const zkp_csr *a, const zkp_csr *b,
                         const zkp_csr *c, zkp_nova_r1cs **out);
void zkp_nova_r1cs_destroy(zkp_nova_r1cs *r);
/* FInstance (r1cs/mod.rs:19-26): x points to num_io x 4 limbs owned by the caller (an output instance writes them). */
typedef struct {
    uint64_t com_e_xy[12];
    uint8_t com_e_is_inf;
    uint64_t u[4];
    uint64_t com_w_xy[12];
    uint8_t com_w_is_inf;
    uint64_t *x;
} zkp_nova_instance;
/* NIFSProof (nifs/mod.rs:19-25) with each KzgOpening (kzg/src/opening.rs:12) as point + evaluation. */
typedef struct {
    uint64_t r[4];
    uint64_t opening_point[4];
    uint64_t open_e_xy[12];
    uint8_t open_e_is_inf;
    uint64_t eval_e[4];
    uint64_t open_w_xy[12];
    uint8_t open_w_is_inf;
    uint64_t eval_w[4];
} zkp_nova_proof;
/* NIFS::compute_t, nifs/mod.rs:34-59: d_t = A z1 o B z2 + A z2 o B z1 - u1 C z2 - u2 C z1 in one pass over the matrices (the six
 * products are never written).  d_w1 / d_w2: num_vars Fr on the device; x1 / x2: num_io Fr on the host; d_t: rows Fr. */
int zkp_nova_cross_term_dev(zkp_nova_r1cs *r, const void *d_w1, const uint64_t *x1, const uint64_t u1[4], const void *d_w2,
                            const uint64_t *x2, const uint64_t u2[4], void *d_t, void *stream);
/* NIFS::fold_witness, nifs/mod.rs:64-82: E = E1 + r T + r^2 E2, W = W1 + r W2, one pass.  d_e_out / d_w_out may be d_e1 / d_w1
 * (the running instance of an IVC chain folded in place); they must not overlap the other inputs. */
int zkp_nova_fold_witness_dev(zkp_nova_r1cs *r, const uint64_t rr[4], const void *d_e1, const void *d_w1, const void *d_e2,
                              const void *d_w2, const void *d_t, void *d_e_out, void *d_w_out, void *stream);
/* The equation of is_r1cs_satisfied, r1cs/mod.rs:94-127: *bad_rows = the number of rows i with (A z)_i (B z)_i != u (C z)_i + E_i
 * (0 = satisfied).  The commitment half of that check is zkp_kzg_commit on W and E.  Synchronises `stream`. */
int zkp_nova_relaxed_residual_dev(zkp_nova_r1cs *r, const void *d_w, const uint64_t *x, const uint64_t u[4], const void *d_e,
                                  void *stream, uint64_t *bad_rows);

/* ---- Transcript<Sha256>, nova/src/transcript.rs:69-114 (host).  feed = the PLONK ChallengeGenerator feed (96 bytes of
 *      serialize_uncompressed(G1)); feed_scalar hashes prev || serialize_uncompressed(Fr): the canonical integer as 32 little-endian
 *      bytes (ark-serialize 0.4 for a 255-bit field, restated and PARITY-UNPINNED: no reference fixture fixes those bytes);
 *      challenges draws n Fr (memory form) through StdRng::seed_from_u64 + Fr::rand.  Drawing twice without feeding, or before
 *      any feed, is ZKP_E_ARG (the reference panics, transcript.rs:91-93). ---- */
typedef struct zkp_nova_transcript zkp_nova_transcript;
int zkp_nova_transcript_create(zkp_nova_transcript **out);
void zkp_nova_transcript_destroy(zkp_nova_transcript *t);
int zkp_nova_transcript_feed(zkp_nova_transcript *t, const uint64_t xy[12], uint8_t is_inf);
int zkp_nova_transcript_feed_scalar(zkp_nova_transcript *t, const uint64_t s[4]);
int zkp_nova_transcript_challenges(zkp_nova_transcript *t, size_t n, uint64_t *out);

/* ---- NIFS::prover, nifs_prover.rs:11-47: T on the device (zkp_nova_cross_term_dev), com_T = commit_vector(T) with the resident MSM
 *      (trailing zeros trimmed; ZKP_E_SIZE when the SRS is empty or shorter, like zkp_kzg_commit), feed u1, u2, com_T and draw r,
 *      fold the witness on the device into d_e_out / d_w_out (aliasing as zkp_nova_fold_witness_dev), and fold the instance on the
 *      host (fold_instance, nifs/mod.rs:88-106): com_E = com_E1 + r com_T + r^2 com_E2, com_W = com_W1 + r com_W2, u = u1 + r u2,
 *      x = x1 + r x2.  *out may be *fi1 (and out->x may be fi1->x).  Synchronises `stream` (the MSM result is read back). ---- */
int zkp_nova_nifs_prover_dev(zkp_nova_r1cs *r, const void *d_e1, const void *d_w1, const void *d_e2, const void *d_w2,
                             const zkp_nova_instance *fi1, const zkp_nova_instance *fi2, zkp_nova_transcript *t, void *d_e_out,
                             void *d_w_out, void *stream, zkp_nova_instance *out, uint64_t com_t_xy[12], uint8_t *com_t_is_inf,
                             uint64_t r_out[4]);
/* Host-pointer form: uploads E1, W1, E2, W2, calls the form above and reads E, W back (e_out / w_out may be e1 / w1). */
int zkp_nova_nifs_prover(zkp_nova_r1cs *r, const uint64_t *e1, const uint64_t *w1, const uint64_t *e2, const uint64_t *w2,
                         const zkp_nova_instance *fi1, const zkp_nova_instance *fi2, zkp_nova_transcript *t, uint64_t *e_out,
                         uint64_t *w_out, zkp_nova_instance *out, uint64_t com_t_xy[12], uint8_t *com_t_is_inf, uint64_t r_out[4]);
/* NIFS::prove, nifs_prover.rs:49-70: feed com_E, com_W of fi, draw the opening point, and open E and W there ON THE DEVICE
 * (evaluation and quotient by X - z with the PLONK scan and evaluation kernels, then the MSM): the same values zkp_kzg_open returns
 * for those vectors.  An E that is all zeros opens like zkp_kzg_open opens it: evaluation 0 and the identity (the reference
 * panics there, kzg/src/scheme.rs:136-137).  Synchronises `stream`. */
int zkp_nova_nifs_prove_dev(zkp_nova_r1cs *r, const uint64_t rr[4], const void *d_e, const void *d_w, const zkp_nova_instance *fi,
                            zkp_nova_transcript *t, void *stream, zkp_nova_proof *out);
int zkp_nova_nifs_prove(zkp_nova_r1cs *r, const uint64_t rr[4], const uint64_t *e, const uint64_t *w, const zkp_nova_instance *fi,
                        zkp_nova_transcript *t, zkp_nova_proof *out);
/* NIFS::verify, nifs_verifier.rs:22-91 (host): re-derives r from u1, u2, com_T, then the opening point from fi3's com_E, com_W, then
 * runs zkp_kzg_verify for W and for E.  *accepted = 1 accepted, -1 "Error in computing random r", -2 "Error in computing random
 * opening point", 0 "Folding wrong at W", -3 "Folding wrong at E" (checked in that order, as the reference). */
int zkp_nova_nifs_verify(const uint64_t g2s_xy[24], const zkp_nova_proof *proof, const zkp_nova_instance *fi1,
                         const zkp_nova_instance *fi2, const zkp_nova_instance *fi3, const uint64_t com_t_xy[12], uint8_t com_t_is_inf,
                         zkp_nova_transcript *t, int *accepted);

#ifdef __cplusplus
}
#endif
#endif /* ZKP_HIP_H */
