//! zkp-hip-sys -- `extern "C"` declarations for libzkp_hip.so, one to one with include/zkp_hip.h.
//!
//! SOURCE-ONLY: this crate has not been compiled (no Rust toolchain in the repository's build environment); the
//! declarations below are generated from the header by tools/gen_rust_sys.py and checked against it by
//! tests/test_rust_sys_matches_header.py, and every symbol is checked against the built library by tests/test_abi_cpu.py.
//! Each function's contract, and the reference file:line it replaces, is documented in include/zkp_hip.h.
#![allow(non_camel_case_types)]
use core::ffi::{c_char, c_void};

pub const ZKP_OK: i32 = 0;
pub const ZKP_E_ARG: i32 = -1;
pub const ZKP_E_NOMEM: i32 = -2;
pub const ZKP_E_DEVICE: i32 = -3;
pub const ZKP_E_SIZE: i32 = -4;
/// layout of the evaluations of zkp_kzg_recover_cosets_batch*: value j of coset k at k + j r, or at k l + j (cells)
pub const ZKP_KZG_LAYOUT_NATURAL: i32 = 0;
pub const ZKP_KZG_LAYOUT_CELLS: i32 = 1;
pub const ZKP_KZG_ORDER_NATURAL: i32 = 0;
pub const ZKP_KZG_ORDER_BITREV: i32 = 1;

#[repr(C)] pub struct zkp_bases { _private: [u8; 0] }
#[repr(C)] pub struct zkp_plonk_prover { _private: [u8; 0] }
#[repr(C)] pub struct zkp_plonk_transcript { _private: [u8; 0] }
#[repr(C)] pub struct zkp_nova_r1cs { _private: [u8; 0] }
#[repr(C)] pub struct zkp_nova_transcript { _private: [u8; 0] }
#[repr(C)] pub struct zkp_kzg_opener { _private: [u8; 0] }
#[repr(C)] pub struct zkp_kzg_recoverer { _private: [u8; 0] }
#[repr(C)] pub struct zkp_kzg_cell_verifier { _private: [u8; 0] }
#[repr(C)] pub struct zkp_kzg_eval_opener { _private: [u8; 0] }
#[repr(C)] pub struct zkp_kzg_point_verifier { _private: [u8; 0] }
#[repr(C)] pub struct zkp_pairing_checker { _private: [u8; 0] }

/// how a bases handle is expanded (zkp_g1_bases_expansion); all zero when it is not
#[repr(C)]
pub struct zkp_bases_expansion {
    pub window_bits: u32,
    pub slices: u32,      // insertions per scalar: 2 x planes for endomorphism-split planes
    pub planes: u32,
    pub glv: u32,         // 1: zkp_g1_bases_precompute_glv
    pub widest_slice_bits: u32,
    pub bytes: usize,     // device bytes of the planes, summed over shards
}

/// report of zkp_g1_validate* / zkp_g1_bases_validate; status of a point: 0 valid, 1 non-canonical, 2 off the curve, 3 outside G1
#[repr(C)]
pub struct zkp_g1_validation {
    pub checked: u64,
    pub bad: u64,
    pub non_canonical: u64,
    pub off_curve: u64,
    pub outside_subgroup: u64,
    pub first_bad: u64,    // lowest bad index, or n when bad == 0
    pub first_status: i32, // its status, or 0
}

/// outputs of zkp_selftest_msm_sort_dev, in the order of the ZKP_SORT_* enum: digits, entries, pstart, ghist, start, sorted, perm, over,
/// over_b, over_off, desc
pub const ZKP_SORT_OUTPUTS: usize = 11;

/// the geometry the MSM's sort kernels were given (zkp_selftest_msm_sort_dev); out_words: 32-bit words of every output
#[repr(C)]
pub struct zkp_msm_sort_geometry {
    pub c: u32,
    pub nwin: u32,
    pub nb: u32,
    pub nslice: u32,
    pub shared: u32,
    pub glv: u32,
    pub nchunk: u32,
    pub lo_bits: u32,
    pub nhi: u32,
    pub run_limit: u32,
    pub piece: u32,
    pub over_cap: u32,
    pub desc_cap: u32,
    pub ps_tile: u32,
    pub nranges: u32,
    pub range_index: u32,
    pub n: u64,
    pub ns: u64,
    pub chunk: u64,
    pub range_off: u64,
    pub range_len: u64,
    pub out_words: [u64; ZKP_SORT_OUTPUTS],
    pub off: [u16; 36],
}

/// caller's device buffers for zkp_selftest_msm_sort_dev and their capacities in 32-bit words
#[repr(C)]
pub struct zkp_msm_sort_outputs {
    pub d_out: [*mut c_void; ZKP_SORT_OUTPUTS],
    pub words: [usize; ZKP_SORT_OUTPUTS],
}

/// one pyramid launch of the bucket reduction: grid (grid_x, level + 1, nwin); quad: four lanes per add
#[repr(C)]
#[derive(Clone, Copy)]
pub struct zkp_msm_reduce_level {
    pub level: u32,
    pub half: u32,
    pub quad: u32,
    pub grid_x: u32,
}

/// one fold step: grid (grid_x, pairs); lane: one lane per add, else four
#[repr(C)]
#[derive(Clone, Copy)]
pub struct zkp_msm_fold_step {
    pub pairs: u32,
    pub lane: u32,
    pub grid_x: u32,
}

/// the launches and buffer sizes (32-bit words) of zkp_selftest_msm_reduce_dev
#[repr(C)]
pub struct zkp_msm_reduce_geometry {
    pub c: u32,
    pub nwin: u32,
    pub nb: u32,
    pub split_log: u32,
    pub tail_max_waves: u32,
    pub nlevel: u32,
    pub tail_blocks: u32,
    pub tail_threads: u32,
    pub combine_x: u32,
    pub over_cap: u32,
    pub desc_cap: u32,
    pub reserved: u32,
    pub cap: u64,
    pub level: [zkp_msm_reduce_level; 24],
    pub fold: [zkp_msm_fold_step; 2],
    pub bucket_words: u64,
    pub parts_words: u64,
    pub over_words: u64,
    pub over_b_words: u64,
    pub over_off_words: u64,
    pub pieces_words: u64,
    pub carry_words: u64,
    pub result_words: u64,
    pub flag_words: u64,
}

/// the caller's buffers for zkp_selftest_msm_reduce_dev and their capacities in 32-bit words
#[repr(C)]
pub struct zkp_msm_reduce_io {
    pub c: u32,
    pub nwin: u32,
    pub split_log: u32,
    pub over_cap: u32,
    pub desc_cap: u32,
    pub resume: u32,
    pub more: u32,
    pub reserved: u32,
    pub d_buckets: *const c_void,
    pub d_parts: *const c_void,
    pub d_over: *const c_void,
    pub d_over_b: *const c_void,
    pub d_over_off: *const c_void,
    pub d_pieces: *const c_void,
    pub d_carry: *const c_void,
    pub buckets_words: usize,
    pub parts_words: usize,
    pub over_words: usize,
    pub over_b_words: usize,
    pub over_off_words: usize,
    pub pieces_words: usize,
    pub carry_words: usize,
    pub d_out_buckets: *mut c_void,
    pub d_out_carry: *mut c_void,
    pub out_buckets_words: usize,
    pub out_carry_words: usize,
    pub out_results: *mut u32,
    pub out_flags: *mut u32,
    pub out_results_words: usize,
    pub out_flags_words: usize,
}

/// ZKP_G1_DECODE_SUBGROUP: run the subgroup test of zkp_g1_validate while decoding
pub const ZKP_G1_DECODE_SUBGROUP: u32 = 1;

/// report of zkp_g1_decompress* / zkp_g1_bases_create_compressed; status of a point: as zkp_g1_validation, and 4 malformed encoding
#[repr(C)]
pub struct zkp_g1_decoding {
    pub checked: u64,
    pub bad: u64,
    pub malformed: u64,
    pub non_canonical: u64,
    pub off_curve: u64,
    pub outside_subgroup: u64,
    pub first_bad: u64,    // lowest bad index, or n when bad == 0
    pub first_status: i32, // its status, or 0
}

/// struct Proof of plonk/src/prover.rs:23-41 in ABI form
#[repr(C)]
pub struct zkp_plonk_proof {
    pub commit_xy: [[u64; 12]; 9], // a, b, c, z, t_lo, t_mid, t_hi, w_ev_x, w_ev_wx
    pub commit_is_inf: [u8; 9],
    pub bars: [[u64; 4]; 6],       // bar_a, bar_b, bar_c, bar_s_sigma_1, bar_s_sigma_2, bar_z_w
    pub u: [u64; 4],
    pub degree: u64,
}

/// the gates of plonk/src/circuit.rs as struct of arrays (zkp_plonk_prover_create_from_gates)
#[repr(C)]
pub struct zkp_plonk_gates {
    pub gates: usize,     // g >= 2 real gates
    pub pos: *const u32,  // g x 6: a_col a_row b_col b_row c_col c_row
    pub sel: *const u64,  // g x 6 x 4 limbs: q_m q_l q_r q_o q_c pi as stored in Gate
    pub vals: *const u64, // g x 3 x 4 limbs: a, b, c of Circuit::vals
}

/// gathered / scattered transform layout of zkp_ntt_fr_layout_dev (strides in elements)
#[repr(C)]
pub struct zkp_ntt_layout {
    pub lo_bits: u32,
    pub mid_bits: u32,
    pub mid_stride: usize,
    pub hi_stride: usize,
    pub batch_stride: usize,
}

/// split of the in-process multi-GPU transform (zkp_ntt_fr_sharded_geometry)
#[repr(C)]
pub struct zkp_ntt_shard_geometry {
    pub slots: u32,
    pub log_n1: u32,
    pub log_n2: u32,
    pub chunks: u32,
    pub r1: usize,
    pub r2: usize,
    pub cw: usize,
    pub slab: usize,
}
/// one R1CS matrix as host CSR (zkp_nova_r1cs_create)
#[repr(C)]
pub struct zkp_csr {
    pub row_ptr: *const u64,
    pub cols: *const u32,
    pub vals: *const u64,
}

/// FInstance of nova/src/r1cs/mod.rs:19-26 in ABI form; x = num_io x 4 limbs owned by the caller
#[repr(C)]
pub struct zkp_nova_instance {
    pub com_e_xy: [u64; 12],
    pub com_e_is_inf: u8,
    pub u: [u64; 4],
    pub com_w_xy: [u64; 12],
    pub com_w_is_inf: u8,
    pub x: *mut u64,
}

/// NIFSProof of nova/src/nifs/mod.rs:19-25 in ABI form
#[repr(C)]
pub struct zkp_nova_proof {
    pub r: [u64; 4],
    pub opening_point: [u64; 4],
    pub open_e_xy: [u64; 12],
    pub open_e_is_inf: u8,
    pub eval_e: [u64; 4],
    pub open_w_xy: [u64; 12],
    pub open_w_is_inf: u8,
    pub eval_w: [u64; 4],
}

pub const ZKP_NTT_NATURAL: i32 = 0;
pub const ZKP_NTT_K1SLAB: i32 = 1;
pub const ZKP_NTT_COLUMNS: i32 = 2;

extern "C" {
    pub fn zkp_init(device: i32) -> i32;
    pub fn zkp_init_devices(devices: *const i32, n_devices: i32) -> i32;
    pub fn zkp_device_count() -> i32;
    pub fn zkp_set_device(slot: i32) -> i32;
    pub fn zkp_shutdown();
    pub fn zkp_last_error() -> *const c_char;
    pub fn zkp_abi_version() -> i32;
    pub fn zkp_profile_enable(on: i32);
    pub fn zkp_profile_reset();
    pub fn zkp_profile_read(name: *const c_char, total_ms: *mut f64, count: *mut u64) -> i32;
    pub fn zkp_profile_clock_read(name: *const c_char, cycles: *mut u64, ref_ticks: *mut u64, waves: *mut u64) -> i32;
    pub fn zkp_probe_mad_rate(launches: u32, lane_mads_per_s: *mut f64, clock_mhz: *mut f64, ms_per_launch: *mut f64) -> i32;
    pub fn zkp_g1_bases_create(xy: *const u64, is_inf: *const u8, n: usize, out: *mut *mut zkp_bases) -> i32;
    pub fn zkp_g1_bases_create_dev(d_xy: *const c_void, d_is_inf: *const u8, n: usize, stream: *mut c_void, out: *mut *mut zkp_bases) -> i32;
    pub fn zkp_g1_bases_precompute(b: *mut zkp_bases, window_bits: u32) -> i32;
    pub fn zkp_g1_bases_precompute_glv(b: *mut zkp_bases, window_bits: u32) -> i32;
    pub fn zkp_g1_bases_len(b: *const zkp_bases) -> usize;
    pub fn zkp_g1_bases_info(b: *const zkp_bases, window_bits: *mut u32, slices: *mut u32) -> i32;
    pub fn zkp_g1_bases_expansion(b: *const zkp_bases, out: *mut zkp_bases_expansion) -> i32;
    pub fn zkp_g1_bases_destroy(b: *mut zkp_bases);
    pub fn zkp_g1_validate_dev(d_xy: *const c_void, d_is_inf: *const u8, n: usize, d_status: *mut u8, stream: *mut c_void, out: *mut zkp_g1_validation) -> i32;
    pub fn zkp_g1_validate(xy: *const u64, is_inf: *const u8, n: usize, status: *mut u8, out: *mut zkp_g1_validation) -> i32;
    pub fn zkp_g1_bases_validate(b: *const zkp_bases, status: *mut u8, out: *mut zkp_g1_validation) -> i32;
    pub fn zkp_srs_check(srs: *const zkp_bases, g2s_xy: *const u64, n: usize, r: *const u64, accepted: *mut i32) -> i32;
    pub fn zkp_g1_decompress_dev(d_bytes: *const c_void, n: usize, flags: u32, d_out_xy: *mut c_void, d_out_is_inf: *mut u8, d_status: *mut u8, stream: *mut c_void, out: *mut zkp_g1_decoding) -> i32;
    pub fn zkp_g1_decompress(bytes: *const u8, n: usize, flags: u32, out_xy: *mut u64, out_is_inf: *mut u8, status: *mut u8, out: *mut zkp_g1_decoding) -> i32;
    pub fn zkp_g1_compress_dev(d_xy: *const c_void, d_is_inf: *const u8, n: usize, d_out_bytes: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_g1_compress(xy: *const u64, is_inf: *const u8, n: usize, out_bytes: *mut u8) -> i32;
    pub fn zkp_g1_bases_create_compressed(bytes: *const u8, n: usize, flags: u32, report: *mut zkp_g1_decoding, out: *mut *mut zkp_bases) -> i32;
    pub fn zkp_fr_from_bytes_dev(d_bytes: *const c_void, n: usize, big_endian: i32, d_out: *mut c_void, stream: *mut c_void, bad: *mut u64, first_bad: *mut u64) -> i32;
    pub fn zkp_fr_to_bytes_dev(d_in: *const c_void, n: usize, big_endian: i32, d_out_bytes: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_msm_g1(bases: *const zkp_bases, scalars: *const u64, n: usize, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_msm_g1_dev(bases: *const zkp_bases, d_scalars: *const c_void, n: usize, stream: *mut c_void, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_msm_g1_batch_dev(bases: *const zkp_bases, d_scalars: *const *const c_void, count: usize, n: usize, stream: *mut c_void, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_msm_g1_bits(bases: *const zkp_bases, scalars: *const u64, n: usize, bits: u32, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_msm_g1_bits_dev(bases: *const zkp_bases, d_scalars: *const c_void, n: usize, bits: u32, stream: *mut c_void, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_msm_g1_batch_bits_dev(bases: *const zkp_bases, d_scalars: *const *const c_void, count: usize, n: usize, bits: u32, stream: *mut c_void, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_fr_bit_length_dev(d_scalars: *const c_void, n: usize, stream: *mut c_void, out_bits: *mut u32) -> i32;
    pub fn zkp_msm_g1_partial_dev(bases: *const zkp_bases, d_scalars: *const c_void, n: usize, stream: *mut c_void, out_xyzz: *mut u64) -> i32;
    pub fn zkp_msm_g1_partial(bases: *const zkp_bases, scalars: *const u64, n: usize, out_xyzz: *mut u64) -> i32;
    pub fn zkp_g1_bases_shard_count(b: *const zkp_bases) -> i32;
    pub fn zkp_g1_bases_shard(b: *const zkp_bases, i: usize, slot: *mut i32, device: *mut i32, offset: *mut usize, len: *mut usize) -> i32;
    pub fn zkp_msm_g1_sharded_dev(bases: *const zkp_bases, d_scalars: *const *const c_void, n: usize, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_msm_g1_sharded_dev_after(bases: *const zkp_bases, d_scalars: *const *const c_void, ready_events: *mut *mut c_void, n: usize, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_g1_xyzz_sum(partials: *const u64, count: usize, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_kzg_commit(srs: *const zkp_bases, coeffs: *const u64, len: usize, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_kzg_open(srs: *const zkp_bases, coeffs: *const u64, len: usize, z: *const u64, out_xy: *mut u64, out_is_inf: *mut u8, out_eval: *mut u64) -> i32;
    pub fn zkp_g1_scale_dev(d_xy: *mut c_void, d_is_inf: *mut u8, d_scalars: *const c_void, n: usize, stream: *mut c_void) -> i32;
    pub fn zkp_g1_ntt_dev(d_xy: *mut c_void, d_is_inf: *mut u8, log_n: u32, inverse: i32, stream: *mut c_void) -> i32;
    pub fn zkp_g1_ntt(xy: *mut u64, is_inf: *mut u8, log_n: u32, inverse: i32) -> i32;
    pub fn zkp_g1_bases_lagrange(srs: *const zkp_bases, log_n: u32, out: *mut *mut zkp_bases) -> i32;
    pub fn zkp_kzg_opener_create(srs: *const zkp_bases, log_n: u32, out: *mut *mut zkp_kzg_opener) -> i32;
    pub fn zkp_kzg_opener_destroy(o: *mut zkp_kzg_opener);
    pub fn zkp_kzg_open_all(o: *const zkp_kzg_opener, coeffs: *const u64, len: usize, out_xy: *mut u64, out_is_inf: *mut u8, out_evals: *mut u64) -> i32;
    pub fn zkp_kzg_open_all_dev(o: *const zkp_kzg_opener, d_coeffs: *const c_void, len: usize, d_out_xy: *mut c_void, d_out_is_inf: *mut u8, d_out_evals: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_kzg_opener_create_cosets(srs: *const zkp_bases, log_n: u32, log_l: u32, out: *mut *mut zkp_kzg_opener) -> i32;
    pub fn zkp_kzg_open_cosets(o: *const zkp_kzg_opener, coeffs: *const u64, len: usize, out_xy: *mut u64, out_is_inf: *mut u8, out_evals: *mut u64) -> i32;
    pub fn zkp_kzg_open_cosets_dev(o: *const zkp_kzg_opener, d_coeffs: *const c_void, len: usize, d_out_xy: *mut c_void, d_out_is_inf: *mut u8, d_out_evals: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_kzg_opener_create_cosets_batch(srs: *const zkp_bases, log_n: u32, log_l: u32, max_polys: usize, out: *mut *mut zkp_kzg_opener) -> i32;
    pub fn zkp_kzg_open_cosets_batch(o: *const zkp_kzg_opener, coeffs: *const u64, n_polys: usize, len: usize, stride: usize, out_xy: *mut u64, out_is_inf: *mut u8, out_evals: *mut u64) -> i32;
    pub fn zkp_kzg_open_cosets_batch_dev(o: *const zkp_kzg_opener, d_coeffs: *const c_void, n_polys: usize, len: usize, stride: usize, d_out_xy: *mut c_void, d_out_is_inf: *mut u8, d_out_evals: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_kzg_verify_coset(srs: *const zkp_bases, g2_sl_xy: *const u64, commit_xy: *const u64, commit_is_inf: u8, w_xy: *const u64, w_is_inf: u8, x: *const u64, log_l: u32, evals: *const u64, accepted: *mut i32) -> i32;
    pub fn zkp_kzg_recoverer_create(log_n: u32, log_l: u32, out: *mut *mut zkp_kzg_recoverer) -> i32;
    pub fn zkp_kzg_recoverer_destroy(rc: *mut zkp_kzg_recoverer);
    pub fn zkp_kzg_recover_cosets(rc: *const zkp_kzg_recoverer, evals: *const u64, present: *const u8, len: usize, out_coeffs: *mut u64, out_evals: *mut u64, consistent: *mut i32) -> i32;
    pub fn zkp_kzg_recover_cosets_dev(rc: *const zkp_kzg_recoverer, d_evals: *const c_void, present: *const u8, len: usize, d_out_coeffs: *mut c_void, d_out_evals: *mut c_void, d_inconsistent: *mut u32, stream: *mut c_void) -> i32;
    pub fn zkp_kzg_recoverer_create_batch(log_n: u32, log_l: u32, max_polys: usize, out: *mut *mut zkp_kzg_recoverer) -> i32;
    pub fn zkp_kzg_recover_cosets_batch(rc: *const zkp_kzg_recoverer, evals: *const u64, n_polys: usize, present: *const u8, len: usize, layout: i32, out_coeffs: *mut u64, out_evals: *mut u64, consistent: *mut u8) -> i32;
    pub fn zkp_kzg_recover_cosets_batch_dev(rc: *const zkp_kzg_recoverer, d_evals: *const c_void, n_polys: usize, present: *const u8, len: usize, stride: usize, layout: i32, d_out_coeffs: *mut c_void, d_out_evals: *mut c_void, d_inconsistent: *mut u32, stream: *mut c_void) -> i32;
    pub fn zkp_kzg_cell_verifier_create(srs: *const zkp_bases, g2_sl_xy: *const u64, log_n: u32, log_l: u32, max_cells: usize, max_commits: usize, out: *mut *mut zkp_kzg_cell_verifier) -> i32;
    pub fn zkp_kzg_cell_verifier_destroy(v: *mut zkp_kzg_cell_verifier);
    pub fn zkp_kzg_verify_cells(v: *const zkp_kzg_cell_verifier, commits_xy: *const u64, commits_is_inf: *const u8, n_commits: usize, n_cells: usize, commit_index: *const u32, coset_index: *const u32, evals: *const u64, proofs_xy: *const u64, proofs_is_inf: *const u8, weights: *const u64, accepted: *mut i32) -> i32;
    pub fn zkp_kzg_verify_cells_dev(v: *const zkp_kzg_cell_verifier, d_commits_xy: *const c_void, d_commits_is_inf: *const u8, n_commits: usize, n_cells: usize, commit_index: *const u32, coset_index: *const u32, d_evals: *const c_void, d_proofs_xy: *const c_void, d_proofs_is_inf: *const u8, d_weights: *const c_void, stream: *mut c_void, accepted: *mut i32) -> i32;
    pub fn zkp_kzg_cells_aggregate_dev(v: *const zkp_kzg_cell_verifier, n_commits: usize, n_cells: usize, commit_index: *const u32, coset_index: *const u32, d_evals: *const c_void, d_weights: *const c_void, d_out_interp: *mut c_void, d_out_commit_weights: *mut c_void, d_out_proof_scalars: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_kzg_eval_opener_create(lagrange: *const zkp_bases, log_n: u32, order: i32, max_polys: usize, out: *mut *mut zkp_kzg_eval_opener) -> i32;
    pub fn zkp_kzg_eval_opener_destroy(o: *mut zkp_kzg_eval_opener);
    pub fn zkp_kzg_commit_evals_batch(o: *const zkp_kzg_eval_opener, evals: *const u64, n_polys: usize, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_kzg_commit_evals_batch_dev(o: *const zkp_kzg_eval_opener, d_evals: *const c_void, n_polys: usize, stream: *mut c_void, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_kzg_open_evals_batch(o: *const zkp_kzg_eval_opener, evals: *const u64, n_polys: usize, z: *const u64, out_xy: *mut u64, out_is_inf: *mut u8, out_y: *mut u64) -> i32;
    pub fn zkp_kzg_open_evals_batch_dev(o: *const zkp_kzg_eval_opener, d_evals: *const c_void, n_polys: usize, d_z: *const c_void, stream: *mut c_void, out_xy: *mut u64, out_is_inf: *mut u8, out_y: *mut u64) -> i32;
    pub fn zkp_kzg_open_evals_field_dev(o: *const zkp_kzg_eval_opener, d_evals: *const c_void, n_polys: usize, d_z: *const c_void, d_out_y: *mut c_void, d_out_quotient: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_kzg_point_verifier_create(g2s_xy: *const u64, max_openings: usize, max_commits: usize, out: *mut *mut zkp_kzg_point_verifier) -> i32;
    pub fn zkp_kzg_point_verifier_destroy(v: *mut zkp_kzg_point_verifier);
    pub fn zkp_kzg_verify_points(v: *const zkp_kzg_point_verifier, commits_xy: *const u64, commits_is_inf: *const u8, n_commits: usize, n_openings: usize, commit_index: *const u32, z: *const u64, y: *const u64, proofs_xy: *const u64, proofs_is_inf: *const u8, weights: *const u64, accepted: *mut i32) -> i32;
    pub fn zkp_kzg_verify_points_dev(v: *const zkp_kzg_point_verifier, d_commits_xy: *const c_void, d_commits_is_inf: *const u8, n_commits: usize, n_openings: usize, commit_index: *const u32, d_z: *const c_void, d_y: *const c_void, d_proofs_xy: *const c_void, d_proofs_is_inf: *const u8, d_weights: *const c_void, stream: *mut c_void, accepted: *mut i32) -> i32;
    pub fn zkp_kzg_verify_points_find_bad(v: *const zkp_kzg_point_verifier, commits_xy: *const u64, commits_is_inf: *const u8, n_commits: usize, n_openings: usize, commit_index: *const u32, z: *const u64, y: *const u64, proofs_xy: *const u64, proofs_is_inf: *const u8, weights: *const u64, accepted: *mut i32, first_bad: *mut usize) -> i32;
    pub fn zkp_kzg_verify_points_find_bad_dev(v: *const zkp_kzg_point_verifier, d_commits_xy: *const c_void, d_commits_is_inf: *const u8, n_commits: usize, n_openings: usize, commit_index: *const u32, d_z: *const c_void, d_y: *const c_void, d_proofs_xy: *const c_void, d_proofs_is_inf: *const u8, d_weights: *const c_void, stream: *mut c_void, accepted: *mut i32, first_bad: *mut usize) -> i32;
    pub fn zkp_kzg_points_aggregate_dev(v: *const zkp_kzg_point_verifier, n_commits: usize, n_openings: usize, commit_index: *const u32, d_z: *const c_void, d_y: *const c_void, d_weights: *const c_void, d_out_commit_weights: *mut c_void, d_out_rz: *mut c_void, d_out_r: *mut c_void, d_out_neg_sum: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_kzg_verify_evals_batch_dev(v: *const zkp_kzg_point_verifier, o: *const zkp_kzg_eval_opener, d_evals: *const c_void, n_polys: usize, d_z: *const c_void, d_commits_xy: *const c_void, d_commits_is_inf: *const u8, d_proofs_xy: *const c_void, d_proofs_is_inf: *const u8, d_weights: *const c_void, stream: *mut c_void, accepted: *mut i32) -> i32;
    pub fn zkp_pairing_checker_create(g2_xy: *const u64, g2_is_inf: *const u8, k: usize, max_checks: usize, out: *mut *mut zkp_pairing_checker) -> i32;
    pub fn zkp_pairing_checker_destroy(c: *mut zkp_pairing_checker);
    pub fn zkp_pairing_check_batch_dev(c: *const zkp_pairing_checker, d_p_xy: *const c_void, d_p_is_inf: *const u8, n_checks: usize, validate: i32, d_ok: *mut u8, d_out_fq12: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_pairing_check_batch(c: *const zkp_pairing_checker, p_xy: *const u64, p_is_inf: *const u8, n_checks: usize, validate: i32, ok: *mut u8, out_fq12: *mut u64) -> i32;
    pub fn zkp_kzg_verify_points_each(v: *const zkp_kzg_point_verifier, commits_xy: *const u64, commits_is_inf: *const u8, n_commits: usize, n_openings: usize, commit_index: *const u32, z: *const u64, y: *const u64, proofs_xy: *const u64, proofs_is_inf: *const u8, ok: *mut u8, n_bad: *mut usize) -> i32;
    pub fn zkp_kzg_verify_points_each_dev(v: *const zkp_kzg_point_verifier, d_commits_xy: *const c_void, d_commits_is_inf: *const u8, n_commits: usize, n_openings: usize, commit_index: *const u32, d_z: *const c_void, d_y: *const c_void, d_proofs_xy: *const c_void, d_proofs_is_inf: *const u8, d_ok: *mut u8, n_bad: *mut usize, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_final_exp_counts(out: *mut u64) -> i32;
    pub fn zkp_selftest_fq12_dev(op: i32, d_a: *const c_void, d_b: *const c_void, n: usize, d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_miller_dev(c: *const zkp_pairing_checker, d_p_xy: *const c_void, d_p_is_inf: *const u8, n_checks: usize, d_out_fq12: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_fr_inverse_dev(d_in: *const c_void, n: usize, method: i32, d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_g1_mul(base_xy: *const u64, base_is_inf: u8, scalar: *const u64, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_g1_fixed_base_mul_dev(d_scalars: *const c_void, n: usize, d_out_xy: *mut c_void, d_out_is_inf: *mut u8, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_fq_inverse_dev(d_in: *const c_void, n: usize, form: i32, d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_fq28_dev(op: i32, d_in: *const c_void, n: usize, d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_fr29_dev(op: i32, d_in: *const c_void, n: usize, d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_fp_dev(field: i32, op: i32, d_in: *const c_void, n: usize, d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_gl_dev(op: i32, d_in: *const c_void, n: usize, d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_g1_dev(op: i32, d_a: *const c_void, d_b: *const c_void, n: usize, stride: usize, d_out: *mut c_void, d_flag: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_glv_split_dev(d_scalars: *const c_void, n: usize, d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_poly_scan_dev(op: i32, count: usize, d_in: *const *const c_void, d_out: *const *mut c_void, n: *const usize, flags: *const u32, chunk: u32, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_poly_scale_pow_dev(d_in: *const c_void, n: usize, base: *const u64, e0: u64, chunk: u32, d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_poly_div_linear_dev(count: usize, d_c: *const *const c_void, len: *const usize, z: *const u64, d_out: *const *mut c_void, chunk: u32, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_poly_eval_dev(count: usize, d_c: *const *const c_void, len: *const usize, z: *const u64, out: *mut u64, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_poly_lincomb_dev(terms: usize, d_p: *const *const c_void, len: *const usize, s: *const u64, n_out: usize, d_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_poly_trim_len_dev(d_c: *const c_void, n: usize, out_len: *mut usize, stream: *mut c_void) -> i32;
    pub fn zkp_selftest_msm_sort_dev(bases: *const zkp_bases, d_scalars: *const *const c_void, count: usize, n: usize, range_index: usize, stream: *mut c_void, geom: *mut zkp_msm_sort_geometry, out: *const zkp_msm_sort_outputs) -> i32;
    pub fn zkp_selftest_msm_reduce_dev(slot: i32, r#in: *const zkp_msm_reduce_io, stream: *mut c_void, geom: *mut zkp_msm_reduce_geometry) -> i32;
    pub fn zkp_selftest_msm_sort_bits_dev(bases: *const zkp_bases, d_scalars: *const *const c_void, count: usize, n: usize, range_index: usize, bits: u32, stream: *mut c_void, geom: *mut zkp_msm_sort_geometry, out: *const zkp_msm_sort_outputs) -> i32;
    pub fn zkp_srs_g1(secret: *const u64, n: usize, out_xy: *mut u64) -> i32;
    pub fn zkp_ntt_fr(data: *mut u64, log_n: u32, inverse: i32, coset: *const u64) -> i32;
    pub fn zkp_ntt_fr_dev(d_data: *mut c_void, log_n: u32, batch: usize, inverse: i32, coset: *const u64, stream: *mut c_void) -> i32;
    pub fn zkp_ntt_fr_twiddle_dev(d_data: *mut c_void, rows: usize, cols: usize, row0: usize, log_n: u32, inverse: i32, stream: *mut c_void) -> i32;
    pub fn zkp_ntt_fr_axis0_dev(d_in: *const c_void, d_out: *mut c_void, log_len: u32, cols: usize, inverse: i32, tw_log_n: u32, tw_col0: usize, stream: *mut c_void) -> i32;
    pub fn zkp_ntt_fr_layout_dev(d_in: *const c_void, d_out: *mut c_void, log_n: u32, batch: usize, inverse: i32, in_layout: *const zkp_ntt_layout, out_layout: *const zkp_ntt_layout, tw_log_n: u32, tw_row0: usize, stream: *mut c_void) -> i32;
    pub fn zkp_ntt_fr_sharded_geometry(log_n: u32, slots: u32, chunks: u32, out: *mut zkp_ntt_shard_geometry) -> i32;
    pub fn zkp_ntt_fr_sharded_dev(d_slabs: *mut *mut c_void, log_n: u32, inverse: i32, layout_in: i32, layout_out: i32, chunks: u32, streams: *mut *mut c_void) -> i32;
    pub fn zkp_ntt_fr_sharded(data: *mut u64, log_n: u32, inverse: i32, coset: *const u64) -> i32;
    pub fn zkp_ntt_goldilocks(data: *mut u64, log_n: u32, inverse: i32, coset: *const u64) -> i32;
    pub fn zkp_ntt_goldilocks_dev(d_data: *mut c_void, log_n: u32, batch: usize, inverse: i32, coset: *const u64, stream: *mut c_void) -> i32;
    pub fn zkp_fri_layer_eval(coeffs: *const u64, d: usize, coset: u64, log_D: u32, out: *mut u64) -> i32;
    pub fn zkp_fri_fold(coeffs: *const u64, d: usize, r: u64, out: *mut u64) -> i32;
    pub fn zkp_fri_merkle_node_count(n: usize) -> usize;
    pub fn zkp_fri_merkle_tree(leaves: *const u64, n: usize, nodes_out: *mut u64) -> i32;
    pub fn zkp_fri_merkle_tree_dev(d_leaves: *const c_void, n: usize, d_nodes: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_fri_challenges(roots: *const u64, layers: usize, const_val: u64, num_queries: usize, r_out: *mut u64, q_out: *mut u64) -> i32;
    pub fn zkp_fri_prove(coeffs: *const u64, d: usize, blowup_factor: usize, num_queries: usize, out_proof: *mut *mut u64, out_words: *mut usize) -> i32;
    pub fn zkp_fri_verify(proof: *const u64, words: usize) -> i32;
    pub fn zkp_free(p: *mut c_void);
    pub fn zkp_fri_layer_eval_fr(coeffs: *const u64, d: usize, coset: *const u64, log_D: u32, out: *mut u64) -> i32;
    pub fn zkp_fri_fold_fr(coeffs: *const u64, d: usize, r: *const u64, out: *mut u64) -> i32;
    pub fn zkp_fri_merkle_tree_fr(leaves: *const u64, n: usize, nodes_out: *mut u64) -> i32;
    pub fn zkp_fri_merkle_tree_fr_dev(d_leaves: *const c_void, n: usize, d_nodes: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_fri_challenges_fr(roots: *const u64, layers: usize, const_val: *const u64, num_queries: usize, r_out: *mut u64, q_out: *mut u64) -> i32;
    pub fn zkp_fri_prove_fr(coeffs: *const u64, d: usize, blowup_factor: usize, num_queries: usize, out_proof: *mut *mut u64, out_words: *mut usize) -> i32;
    pub fn zkp_fri_verify_fr(proof: *const u64, words: usize) -> i32;
    pub fn zkp_plonk_transcript_create(out: *mut *mut zkp_plonk_transcript) -> i32;
    pub fn zkp_plonk_transcript_destroy(t: *mut zkp_plonk_transcript);
    pub fn zkp_plonk_transcript_feed(t: *mut zkp_plonk_transcript, xy: *const u64, is_inf: u8) -> i32;
    pub fn zkp_plonk_transcript_challenges(t: *mut zkp_plonk_transcript, n: usize, out: *mut u64) -> i32;
    pub fn zkp_poly_mul_fr(a: *const u64, la: usize, b: *const u64, lb: usize, out: *mut u64) -> i32;
    pub fn zkp_plonk_prover_create(srs: *const zkp_bases, log_n: u32, polys: *const *const u64, lens: *const usize, k1: *const u64, k2: *const u64, out: *mut *mut zkp_plonk_prover) -> i32;
    pub fn zkp_plonk_prover_destroy(p: *mut zkp_plonk_prover);
    pub fn zkp_plonk_round1(p: *mut zkp_plonk_prover, blinders: *const u64, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_plonk_round2(p: *mut zkp_plonk_prover, beta: *const u64, gamma: *const u64, blinders: *const u64, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_plonk_round3(p: *mut zkp_plonk_prover, alpha: *const u64, out_xy: *mut u64, out_is_inf: *mut u8, out_degree: *mut usize) -> i32;
    pub fn zkp_plonk_round4(p: *mut zkp_plonk_prover, zeta: *const u64, out_bars: *mut u64) -> i32;
    pub fn zkp_plonk_round5(p: *mut zkp_plonk_prover, v: *const u64, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_plonk_prove(p: *mut zkp_plonk_prover, blinders: *const u64, out: *mut zkp_plonk_proof) -> i32;
    pub fn zkp_g2_generator(out_xy: *mut u64) -> i32;
    pub fn zkp_g2_mul(q_xy: *const u64, q_is_inf: u8, scalar: *const u64, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_pairing(p_xy: *const u64, p_is_inf: u8, q_xy: *const u64, q_is_inf: u8, out_fq12: *mut u64) -> i32;
    pub fn zkp_kzg_verify(g2s_xy: *const u64, commit_xy: *const u64, commit_is_inf: u8, w_xy: *const u64, w_is_inf: u8, y: *const u64, z: *const u64, accepted: *mut i32) -> i32;
    pub fn zkp_kzg_batch_verify(g2s_xy: *const u64, n: usize, commits_xy: *const u64, commits_is_inf: *const u8, points: *const u64, openings_xy: *const u64, openings_is_inf: *const u8, evals: *const u64, r_primes: *const u64, accepted: *mut i32) -> i32;
    pub fn zkp_kzg_aggregate_commitments(commits_xy: *const u64, commits_is_inf: *const u8, n: usize, challenge: *const u64, out_xy: *mut u64, out_is_inf: *mut u8) -> i32;
    pub fn zkp_plonk_verify(p: *mut zkp_plonk_prover, g2s_xy: *const u64, proof: *const zkp_plonk_proof, accepted: *mut i32) -> i32;
    pub fn zkp_plonk_get_poly(p: *mut zkp_plonk_prover, which: i32, out: *mut u64, cap_elems: usize, len: *mut usize) -> i32;
    pub fn zkp_plonk_prover_create_from_gates(srs: *const zkp_bases, gates: *const zkp_plonk_gates, out: *mut *mut zkp_plonk_prover) -> i32;
    pub fn zkp_plonk_prover_set_witness(p: *mut zkp_plonk_prover, vals: *const u64, pi: *const u64, gates: usize) -> i32;
    pub fn zkp_plonk_prover_set_witness_dev(p: *mut zkp_plonk_prover, d_vals: *const c_void, d_pi: *const c_void, gates: usize, stream: *mut c_void) -> i32;
    pub fn zkp_plonk_get_circuit_poly(p: *mut zkp_plonk_prover, which: i32, out: *mut u64, cap_elems: usize, len: *mut usize) -> i32;
    pub fn zkp_plonk_prover_info(p: *const zkp_plonk_prover, log_n: *mut u32, k1: *mut u64, k2: *mut u64) -> i32;
    pub fn zkp_nova_r1cs_create(srs: *const zkp_bases, rows: usize, num_vars: usize, num_io: usize, a: *const zkp_csr, b: *const zkp_csr, c: *const zkp_csr, out: *mut *mut zkp_nova_r1cs) -> i32;
    pub fn zkp_nova_r1cs_destroy(r: *mut zkp_nova_r1cs);
    pub fn zkp_nova_cross_term_dev(r: *mut zkp_nova_r1cs, d_w1: *const c_void, x1: *const u64, u1: *const u64, d_w2: *const c_void, x2: *const u64, u2: *const u64, d_t: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_nova_fold_witness_dev(r: *mut zkp_nova_r1cs, rr: *const u64, d_e1: *const c_void, d_w1: *const c_void, d_e2: *const c_void, d_w2: *const c_void, d_t: *const c_void, d_e_out: *mut c_void, d_w_out: *mut c_void, stream: *mut c_void) -> i32;
    pub fn zkp_nova_relaxed_residual_dev(r: *mut zkp_nova_r1cs, d_w: *const c_void, x: *const u64, u: *const u64, d_e: *const c_void, stream: *mut c_void, bad_rows: *mut u64) -> i32;
    pub fn zkp_nova_transcript_create(out: *mut *mut zkp_nova_transcript) -> i32;
    pub fn zkp_nova_transcript_destroy(t: *mut zkp_nova_transcript);
    pub fn zkp_nova_transcript_feed(t: *mut zkp_nova_transcript, xy: *const u64, is_inf: u8) -> i32;
    pub fn zkp_nova_transcript_feed_scalar(t: *mut zkp_nova_transcript, s: *const u64) -> i32;
    pub fn zkp_nova_transcript_challenges(t: *mut zkp_nova_transcript, n: usize, out: *mut u64) -> i32;
    pub fn zkp_nova_nifs_prover_dev(r: *mut zkp_nova_r1cs, d_e1: *const c_void, d_w1: *const c_void, d_e2: *const c_void, d_w2: *const c_void, fi1: *const zkp_nova_instance, fi2: *const zkp_nova_instance, t: *mut zkp_nova_transcript, d_e_out: *mut c_void, d_w_out: *mut c_void, stream: *mut c_void, out: *mut zkp_nova_instance, com_t_xy: *mut u64, com_t_is_inf: *mut u8, r_out: *mut u64) -> i32;
    pub fn zkp_nova_nifs_prover(r: *mut zkp_nova_r1cs, e1: *const u64, w1: *const u64, e2: *const u64, w2: *const u64, fi1: *const zkp_nova_instance, fi2: *const zkp_nova_instance, t: *mut zkp_nova_transcript, e_out: *mut u64, w_out: *mut u64, out: *mut zkp_nova_instance, com_t_xy: *mut u64, com_t_is_inf: *mut u8, r_out: *mut u64) -> i32;
    pub fn zkp_nova_nifs_prove_dev(r: *mut zkp_nova_r1cs, rr: *const u64, d_e: *const c_void, d_w: *const c_void, fi: *const zkp_nova_instance, t: *mut zkp_nova_transcript, stream: *mut c_void, out: *mut zkp_nova_proof) -> i32;
    pub fn zkp_nova_nifs_prove(r: *mut zkp_nova_r1cs, rr: *const u64, e: *const u64, w: *const u64, fi: *const zkp_nova_instance, t: *mut zkp_nova_transcript, out: *mut zkp_nova_proof) -> i32;
    pub fn zkp_nova_nifs_verify(g2s_xy: *const u64, proof: *const zkp_nova_proof, fi1: *const zkp_nova_instance, fi2: *const zkp_nova_instance, fi3: *const zkp_nova_instance, com_t_xy: *const u64, com_t_is_inf: u8, t: *mut zkp_nova_transcript, accepted: *mut i32) -> i32;
}

/// The thread-local message of the last failed call.
pub fn last_error() -> String {
    unsafe { std::ffi::CStr::from_ptr(zkp_last_error()).to_string_lossy().into_owned() }
}
