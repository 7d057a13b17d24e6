"""zkp_hip -- ctypes binding of libzkp_hip.so (include/zkp_hip.h), the MI355X backend for the MSM / NTT hot path.

This module is plumbing: it loads the in-tree HIP library and exposes its C ABI over numpy arrays (host entry
points) and torch CUDA tensors (``*_dev`` entry points).  There is NO Python or CPU implementation of any
operation here: if the library is missing or no gfx950 device is usable, calls raise ``ZkpError``.

Data conventions (arkworks in-memory forms, see include/zkp_hip.h): uint64 little-endian Montgomery limbs.
    Fr (n,4)   Goldilocks (n,)   G1 affine (n,12) + uint8 infinity flags
"""
import ctypes as C
import os
import sys

import numpy as np

_PKG = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_PKG)
LIB_PATH = os.path.join(_ROOT, "libzkp_hip.so")
if os.environ.get("ZKP_HIP_LIB"):  # development: try another build of the same library
    LIB_PATH = os.environ["ZKP_HIP_LIB"]

ZKP_OK, ZKP_E_ARG, ZKP_E_NOMEM, ZKP_E_DEVICE, ZKP_E_SIZE = 0, -1, -2, -3, -4


class ZkpError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"zkp_hip error {code}: {msg}")
        self.code = code


_lib = None

_VP, _SZ, _U8P = C.c_void_p, C.c_size_t, C.c_void_p
_SIGS = {
    "zkp_init": ([C.c_int], C.c_int),
    "zkp_init_devices": ([_VP, C.c_int], C.c_int),
    "zkp_device_count": ([], C.c_int),
    "zkp_set_device": ([C.c_int], C.c_int),
    "zkp_shutdown": ([], None),
    "zkp_last_error": ([], C.c_char_p),
    "zkp_abi_version": ([], C.c_int),
    "zkp_profile_enable": ([C.c_int], None),
    "zkp_profile_reset": ([], None),
    "zkp_profile_read": ([C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)], C.c_int),
    "zkp_profile_clock_read": ([C.c_char_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int),
    "zkp_probe_mad_rate": ([C.c_uint, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double)], C.c_int),
    "zkp_g1_bases_create": ([_VP, _U8P, _SZ, C.POINTER(_VP)], C.c_int),
    "zkp_g1_bases_create_dev": ([_VP, _U8P, _SZ, _VP, C.POINTER(_VP)], C.c_int),
    "zkp_g1_bases_precompute": ([_VP, C.c_uint], C.c_int),
    "zkp_g1_bases_len": ([_VP], _SZ),
    "zkp_g1_bases_precompute_glv": ([_VP, C.c_uint], C.c_int),
    "zkp_g1_bases_info": ([_VP, C.POINTER(C.c_uint), C.POINTER(C.c_uint)], C.c_int),
    "zkp_g1_bases_expansion": ([_VP, _VP], C.c_int),
    "zkp_g1_bases_destroy": ([_VP], None),
    "zkp_g1_validate_dev": ([_VP, _U8P, _SZ, _U8P, _VP, _VP], C.c_int),
    "zkp_g1_validate": ([_VP, _U8P, _SZ, _U8P, _VP], C.c_int),
    "zkp_g1_bases_validate": ([_VP, _U8P, _VP], C.c_int),
    "zkp_srs_check": ([_VP, _VP, _SZ, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_g1_decompress_dev": ([_VP, _SZ, C.c_uint, _VP, _U8P, _U8P, _VP, _VP], C.c_int),
    "zkp_g1_decompress": ([_VP, _SZ, C.c_uint, _VP, _U8P, _U8P, _VP], C.c_int),
    "zkp_g1_compress_dev": ([_VP, _U8P, _SZ, _VP, _VP], C.c_int),
    "zkp_g1_compress": ([_VP, _U8P, _SZ, _VP], C.c_int),
    "zkp_g1_bases_create_compressed": ([_VP, _SZ, C.c_uint, _VP, C.POINTER(_VP)], C.c_int),
    "zkp_fr_from_bytes_dev": ([_VP, _SZ, C.c_int, _VP, _VP, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)], C.c_int),
    "zkp_fr_to_bytes_dev": ([_VP, _SZ, C.c_int, _VP, _VP], C.c_int),
    "zkp_g1_scale_dev": ([_VP, _U8P, _VP, _SZ, _VP], C.c_int),
    "zkp_g1_ntt_dev": ([_VP, _U8P, C.c_uint, C.c_int, _VP], C.c_int),
    "zkp_g1_ntt": ([_VP, _U8P, C.c_uint, C.c_int], C.c_int),
    "zkp_g1_bases_lagrange": ([_VP, C.c_uint, C.POINTER(_VP)], C.c_int),
    "zkp_kzg_opener_create": ([_VP, C.c_uint, C.POINTER(_VP)], C.c_int),
    "zkp_kzg_opener_destroy": ([_VP], None),
    "zkp_kzg_open_all": ([_VP, _VP, _SZ, _VP, _U8P, _VP], C.c_int),
    "zkp_kzg_open_all_dev": ([_VP, _VP, _SZ, _VP, _U8P, _VP, _VP], C.c_int),
    "zkp_kzg_opener_create_cosets": ([_VP, C.c_uint, C.c_uint, C.POINTER(_VP)], C.c_int),
    "zkp_kzg_open_cosets": ([_VP, _VP, _SZ, _VP, _U8P, _VP], C.c_int),
    "zkp_kzg_open_cosets_dev": ([_VP, _VP, _SZ, _VP, _U8P, _VP, _VP], C.c_int),
    "zkp_kzg_opener_create_cosets_batch": ([_VP, C.c_uint, C.c_uint, _SZ, C.POINTER(_VP)], C.c_int),
    "zkp_kzg_open_cosets_batch": ([_VP, _VP, _SZ, _SZ, _SZ, _VP, _U8P, _VP], C.c_int),
    "zkp_kzg_open_cosets_batch_dev": ([_VP, _VP, _SZ, _SZ, _SZ, _VP, _U8P, _VP, _VP], C.c_int),
    "zkp_kzg_verify_coset": ([_VP, _VP, _VP, C.c_uint8, _VP, C.c_uint8, _VP, C.c_uint, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_kzg_recoverer_create": ([C.c_uint, C.c_uint, C.POINTER(_VP)], C.c_int),
    "zkp_kzg_recoverer_destroy": ([_VP], None),
    "zkp_kzg_recover_cosets": ([_VP, _VP, _VP, _SZ, _VP, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_kzg_recover_cosets_dev": ([_VP, _VP, _VP, _SZ, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_kzg_recoverer_create_batch": ([C.c_uint, C.c_uint, _SZ, C.POINTER(_VP)], C.c_int),
    "zkp_kzg_recover_cosets_batch": ([_VP, _VP, _SZ, _VP, _SZ, C.c_int, _VP, _VP, _VP], C.c_int),
    "zkp_kzg_recover_cosets_batch_dev": ([_VP, _VP, _SZ, _VP, _SZ, _SZ, C.c_int, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_kzg_cell_verifier_create": ([_VP, _VP, C.c_uint, C.c_uint, _SZ, _SZ, C.POINTER(_VP)], C.c_int),
    "zkp_kzg_cell_verifier_destroy": ([_VP], None),
    "zkp_kzg_verify_cells": ([_VP, _VP, _U8P, _SZ, _SZ, _VP, _VP, _VP, _VP, _U8P, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_kzg_verify_cells_dev": ([_VP, _VP, _U8P, _SZ, _SZ, _VP, _VP, _VP, _VP, _U8P, _VP, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_kzg_cells_aggregate_dev": ([_VP, _SZ, _SZ, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_msm_g1": ([_VP, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_msm_g1_dev": ([_VP, _VP, _SZ, _VP, _VP, _VP], C.c_int),
    "zkp_msm_g1_batch_dev": ([_VP, _VP, _SZ, _SZ, _VP, _VP, _VP], C.c_int),
    "zkp_msm_g1_bits": ([_VP, _VP, _SZ, C.c_uint, _VP, _VP], C.c_int),
    "zkp_msm_g1_bits_dev": ([_VP, _VP, _SZ, C.c_uint, _VP, _VP, _VP], C.c_int),
    "zkp_msm_g1_batch_bits_dev": ([_VP, _VP, _SZ, _SZ, C.c_uint, _VP, _VP, _VP], C.c_int),
    "zkp_fr_bit_length_dev": ([_VP, _SZ, _VP, C.POINTER(C.c_uint)], C.c_int),
    "zkp_msm_g1_partial_dev": ([_VP, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_msm_g1_partial": ([_VP, _VP, _SZ, _VP], C.c_int),
    "zkp_g1_bases_shard_count": ([_VP], C.c_int),
    "zkp_g1_bases_shard": ([_VP, _SZ, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(_SZ), C.POINTER(_SZ)], C.c_int),
    "zkp_msm_g1_sharded_dev": ([_VP, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_msm_g1_sharded_dev_after": ([_VP, _VP, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_g1_xyzz_sum": ([_VP, _SZ, _VP, _VP], C.c_int),
    "zkp_g1_mul": ([_VP, C.c_uint8, _VP, _VP, _VP], C.c_int),
    "zkp_g1_fixed_base_mul_dev": ([_VP, _SZ, _VP, _U8P, _VP], C.c_int),
    "zkp_selftest_fq_inverse_dev": ([_VP, _SZ, C.c_int, _VP, _VP], C.c_int),
    "zkp_selftest_fr_inverse_dev": ([_VP, _SZ, C.c_int, _VP, _VP], C.c_int),
    "zkp_kzg_eval_opener_create": ([_VP, C.c_uint, C.c_int, _SZ, C.POINTER(_VP)], C.c_int),
    "zkp_kzg_eval_opener_destroy": ([_VP], None),
    "zkp_kzg_commit_evals_batch": ([_VP, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_kzg_commit_evals_batch_dev": ([_VP, _VP, _SZ, _VP, _VP, _VP], C.c_int),
    "zkp_kzg_open_evals_batch": ([_VP, _VP, _SZ, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_kzg_open_evals_batch_dev": ([_VP, _VP, _SZ, _VP, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_kzg_open_evals_field_dev": ([_VP, _VP, _SZ, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_kzg_point_verifier_create": ([_VP, _SZ, _SZ, C.POINTER(_VP)], C.c_int),
    "zkp_kzg_point_verifier_destroy": ([_VP], None),
    "zkp_kzg_verify_points": ([_VP, _VP, _U8P, _SZ, _SZ, _VP, _VP, _VP, _VP, _U8P, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_kzg_verify_points_dev": ([_VP, _VP, _U8P, _SZ, _SZ, _VP, _VP, _VP, _VP, _U8P, _VP, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_kzg_verify_points_find_bad": ([_VP, _VP, _U8P, _SZ, _SZ, _VP, _VP, _VP, _VP, _U8P, _VP, C.POINTER(C.c_int), C.POINTER(_SZ)], C.c_int),
    "zkp_kzg_verify_points_find_bad_dev": ([_VP, _VP, _U8P, _SZ, _SZ, _VP, _VP, _VP, _VP, _U8P, _VP, _VP, C.POINTER(C.c_int), C.POINTER(_SZ)],
                                           C.c_int),
    "zkp_kzg_points_aggregate_dev": ([_VP, _SZ, _SZ, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_kzg_verify_evals_batch_dev": ([_VP, _VP, _VP, _SZ, _VP, _VP, _U8P, _VP, _U8P, _VP, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_pairing_checker_create": ([_VP, _U8P, _SZ, _SZ, C.POINTER(_VP)], C.c_int),
    "zkp_pairing_checker_destroy": ([_VP], None),
    "zkp_pairing_check_batch_dev": ([_VP, _VP, _U8P, _SZ, C.c_int, _U8P, _VP, _VP], C.c_int),
    "zkp_pairing_check_batch": ([_VP, _VP, _U8P, _SZ, C.c_int, _U8P, _VP], C.c_int),
    "zkp_kzg_verify_points_each": ([_VP, _VP, _U8P, _SZ, _SZ, _VP, _VP, _VP, _VP, _U8P, _U8P, C.POINTER(_SZ)], C.c_int),
    "zkp_kzg_verify_points_each_dev": ([_VP, _VP, _U8P, _SZ, _SZ, _VP, _VP, _VP, _VP, _U8P, _U8P, C.POINTER(_SZ), _VP], C.c_int),
    "zkp_selftest_final_exp_counts": ([_VP], C.c_int),
    "zkp_selftest_fq12_dev": ([C.c_int, _VP, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_selftest_miller_dev": ([_VP, _VP, _U8P, _SZ, _VP, _VP], C.c_int),
    "zkp_selftest_fq28_dev": ([C.c_int, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_selftest_fr29_dev": ([C.c_int, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_selftest_fp_dev": ([C.c_int, C.c_int, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_selftest_gl_dev": ([C.c_int, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_selftest_g1_dev": ([C.c_int, _VP, _VP, _SZ, _SZ, _VP, _VP, _VP], C.c_int),
    "zkp_selftest_glv_split_dev": ([_VP, _SZ, _VP, _VP], C.c_int),
    "zkp_selftest_poly_scan_dev": ([C.c_int, _SZ, _VP, _VP, _VP, _VP, C.c_uint, _VP], C.c_int),
    "zkp_selftest_poly_scale_pow_dev": ([_VP, _SZ, _VP, C.c_uint64, C.c_uint, _VP, _VP], C.c_int),
    "zkp_selftest_poly_div_linear_dev": ([_SZ, _VP, _VP, _VP, _VP, C.c_uint, _VP], C.c_int),
    "zkp_selftest_poly_eval_dev": ([_SZ, _VP, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_selftest_poly_lincomb_dev": ([_SZ, _VP, _VP, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_selftest_poly_trim_len_dev": ([_VP, _SZ, C.POINTER(_SZ), _VP], C.c_int),
    "zkp_selftest_msm_sort_dev": ([_VP, _VP, _SZ, _SZ, _SZ, _VP, _VP, _VP], C.c_int),
    "zkp_selftest_msm_sort_bits_dev": ([_VP, _VP, _SZ, _SZ, _SZ, C.c_uint, _VP, _VP, _VP], C.c_int),
    "zkp_selftest_msm_reduce_dev": ([C.c_int, _VP, _VP, _VP], C.c_int),
    "zkp_srs_g1": ([_VP, _SZ, _VP], C.c_int),
    "zkp_ntt_fr": ([_VP, C.c_uint, C.c_int, _VP], C.c_int),
    "zkp_ntt_fr_dev": ([_VP, C.c_uint, _SZ, C.c_int, _VP, _VP], C.c_int),
    "zkp_ntt_fr_twiddle_dev": ([_VP, _SZ, _SZ, _SZ, C.c_uint, C.c_int, _VP], C.c_int),
    "zkp_ntt_fr_axis0_dev": ([_VP, _VP, C.c_uint, _SZ, C.c_int, C.c_uint, _SZ, _VP], C.c_int),
    "zkp_ntt_fr_layout_dev": ([_VP, _VP, C.c_uint, _SZ, C.c_int, _VP, _VP, C.c_uint, _SZ, _VP], C.c_int),
    "zkp_ntt_fr_sharded_geometry": ([C.c_uint, C.c_uint, C.c_uint, _VP], C.c_int),
    "zkp_ntt_fr_sharded_dev": ([_VP, C.c_uint, C.c_int, C.c_int, C.c_int, C.c_uint, _VP], C.c_int),
    "zkp_ntt_fr_sharded": ([_VP, C.c_uint, C.c_int, _VP], C.c_int),
    "zkp_ntt_goldilocks": ([_VP, C.c_uint, C.c_int, _VP], C.c_int),
    "zkp_ntt_goldilocks_dev": ([_VP, C.c_uint, _SZ, C.c_int, _VP, _VP], C.c_int),
    "zkp_fri_layer_eval": ([_VP, _SZ, C.c_uint64, C.c_uint, _VP], C.c_int),
    "zkp_fri_fold": ([_VP, _SZ, C.c_uint64, _VP], C.c_int),
    "zkp_fri_merkle_node_count": ([_SZ], _SZ),
    "zkp_fri_merkle_tree": ([_VP, _SZ, _VP], C.c_int),
    "zkp_fri_merkle_tree_dev": ([_VP, _SZ, _VP, _VP], C.c_int),
    "zkp_fri_challenges": ([_VP, _SZ, C.c_uint64, _SZ, _VP, _VP], C.c_int),
    "zkp_fri_prove": ([_VP, _SZ, _SZ, _SZ, C.POINTER(_VP), C.POINTER(_SZ)], C.c_int),
    "zkp_fri_verify": ([_VP, _SZ], C.c_int),
    "zkp_fri_layer_eval_fr": ([_VP, _SZ, _VP, C.c_uint, _VP], C.c_int),
    "zkp_fri_fold_fr": ([_VP, _SZ, _VP, _VP], C.c_int),
    "zkp_fri_merkle_tree_fr": ([_VP, _SZ, _VP], C.c_int),
    "zkp_fri_merkle_tree_fr_dev": ([_VP, _SZ, _VP, _VP], C.c_int),
    "zkp_fri_challenges_fr": ([_VP, _SZ, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_fri_prove_fr": ([_VP, _SZ, _SZ, _SZ, C.POINTER(_VP), C.POINTER(_SZ)], C.c_int),
    "zkp_fri_verify_fr": ([_VP, _SZ], C.c_int),
    "zkp_free": ([_VP], None),
    "zkp_plonk_prove": ([_VP, _VP, _VP], C.c_int),
    "zkp_g2_generator": ([_VP], C.c_int),
    "zkp_g2_mul": ([_VP, C.c_uint8, _VP, _VP, _U8P], C.c_int),
    "zkp_pairing": ([_VP, C.c_uint8, _VP, C.c_uint8, _VP], C.c_int),
    "zkp_kzg_verify": ([_VP, _VP, C.c_uint8, _VP, C.c_uint8, _VP, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_kzg_batch_verify": ([_VP, _SZ, _VP, _U8P, _VP, _VP, _U8P, _VP, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_kzg_aggregate_commitments": ([_VP, _U8P, _SZ, _VP, _VP, _VP], C.c_int),
    "zkp_plonk_verify": ([_VP, _VP, _VP, C.POINTER(C.c_int)], C.c_int),
    "zkp_plonk_transcript_create": ([C.POINTER(_VP)], C.c_int),
    "zkp_plonk_transcript_destroy": ([_VP], None),
    "zkp_plonk_transcript_feed": ([_VP, _VP, C.c_uint8], C.c_int),
    "zkp_plonk_transcript_challenges": ([_VP, _SZ, _VP], C.c_int),
    "zkp_poly_mul_fr": ([_VP, _SZ, _VP, _SZ, _VP], C.c_int),
    "zkp_plonk_prover_create": ([_VP, C.c_uint, _VP, _VP, _VP, _VP, C.POINTER(_VP)], C.c_int),
    "zkp_plonk_prover_destroy": ([_VP], None),
    "zkp_plonk_round1": ([_VP, _VP, _VP, _VP], C.c_int),
    "zkp_plonk_round2": ([_VP, _VP, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_plonk_round3": ([_VP, _VP, _VP, _VP, C.POINTER(C.c_size_t)], C.c_int),
    "zkp_plonk_round4": ([_VP, _VP, _VP], C.c_int),
    "zkp_plonk_round5": ([_VP, _VP, _VP, _VP], C.c_int),
    "zkp_plonk_get_poly": ([_VP, C.c_int, _VP, _SZ, C.POINTER(C.c_size_t)], C.c_int),
    "zkp_plonk_prover_create_from_gates": ([_VP, _VP, C.POINTER(_VP)], C.c_int),
    "zkp_plonk_prover_set_witness": ([_VP, _VP, _VP, _SZ], C.c_int),
    "zkp_plonk_prover_set_witness_dev": ([_VP, _VP, _VP, _SZ, _VP], C.c_int),
    "zkp_plonk_get_circuit_poly": ([_VP, C.c_int, _VP, _SZ, C.POINTER(C.c_size_t)], C.c_int),
    "zkp_plonk_prover_info": ([_VP, C.POINTER(C.c_uint), _VP, _VP], C.c_int),
    "zkp_kzg_commit": ([_VP, _VP, _SZ, _VP, _VP], C.c_int),
    "zkp_kzg_open": ([_VP, _VP, _SZ, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_nova_r1cs_create": ([_VP, _SZ, _SZ, _SZ, _VP, _VP, _VP, C.POINTER(_VP)], C.c_int),
    "zkp_nova_r1cs_destroy": ([_VP], None),
    "zkp_nova_cross_term_dev": ([_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_nova_fold_witness_dev": ([_VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP], C.c_int),
    "zkp_nova_relaxed_residual_dev": ([_VP, _VP, _VP, _VP, _VP, _VP, C.POINTER(C.c_uint64)], C.c_int),
    "zkp_nova_transcript_create": ([C.POINTER(_VP)], C.c_int),
    "zkp_nova_transcript_destroy": ([_VP], None),
    "zkp_nova_transcript_feed": ([_VP, _VP, C.c_uint8], C.c_int),
    "zkp_nova_transcript_feed_scalar": ([_VP, _VP], C.c_int),
    "zkp_nova_transcript_challenges": ([_VP, _SZ, _VP], C.c_int),
    "zkp_nova_nifs_prover_dev": ([_VP] * 15, C.c_int),
    "zkp_nova_nifs_prover": ([_VP] * 14, C.c_int),
    "zkp_nova_nifs_prove_dev": ([_VP] * 8, C.c_int),
    "zkp_nova_nifs_prove": ([_VP] * 7, C.c_int),
    "zkp_nova_nifs_verify": ([_VP, _VP, _VP, _VP, _VP, _VP, C.c_uint8, _VP, C.POINTER(C.c_int)], C.c_int),
}


def exported_symbols():
    """Names every include/zkp_hip.h declaration must be exported under (checked by the CPU test-suite)."""
    return sorted(_SIGS)


def lib():
    """Load libzkp_hip.so (no GPU needed to load it).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ZkpError(ZKP_E_DEVICE, f"{LIB_PATH} not found: run `python zkp-implementation_amd/build.py` "
                           "(hipcc --offload-arch=gfx950); there is no CPU fallback")
        # One HIP runtime per process: PyTorch's wheel bundles its own libamdhip64, and libzkp_hip.so resolves the same soname.  Whichever
        # is loaded first serves both -- unless this library came first and pulled in /opt/rocm's copy: the runtime torch loads afterwards
        # owns the devices and this one sees none ("no HIP device visible" from zkp_init in a process that had loaded the library
        # before importing torch, e.g. build() followed by smoke()).  So torch, where it exists, goes first; plain C callers never load it.
        if "torch" not in sys.modules:
            try:
                import torch  # noqa: F401
            except ImportError:
                pass
        l = C.CDLL(LIB_PATH)
        for name, (args, res) in _SIGS.items():
            fn = getattr(l, name)
            fn.argtypes = args
            fn.restype = res
        _lib = l
    return _lib


def _chk(code):
    if code != ZKP_OK:
        raise ZkpError(code, lib().zkp_last_error().decode())


def init(device=-1):
    _chk(lib().zkp_init(device))


def init_devices(devices=None, n=0):
    """One slot per listed HIP device (a device may repeat); devices=None: devices 0..n-1, n == 0: all visible."""
    if devices is None:
        _chk(lib().zkp_init_devices(None, int(n)))
    else:
        arr = (C.c_int * len(devices))(*[int(d) for d in devices])
        _chk(lib().zkp_init_devices(C.cast(arr, C.c_void_p), len(devices)))


def device_count():
    return int(lib().zkp_device_count())


def set_device(slot):
    """Slot of this thread's handle-less entries; -1 = default (slot 0; zkp_g1_bases_create shards over all slots)."""
    _chk(lib().zkp_set_device(int(slot)))


def shutdown():
    lib().zkp_shutdown()


def profile_enable(on=True):
    """True / 1: every phase; 2: the dominant kernel only (msm_accumulate: events and clock stamps -- each recorded phase boundary is a
    ~5 us bubble on the stream); False / 0: off."""
    lib().zkp_profile_enable(2 if on == 2 and on is not True else int(bool(on)))


def profile_reset():
    lib().zkp_profile_reset()


def profile_read(name):
    """-> (total milliseconds, number of records) of one phase since the last reset (see include/zkp_hip.h)."""
    ms, cnt = C.c_double(0), C.c_uint64(0)
    _chk(lib().zkp_profile_read(name.encode(), C.byref(ms), C.byref(cnt)))
    return ms.value, int(cnt.value)


def profile_clock_read(name):
    """-> (shader cycles, 100 MHz reference ticks, stamped workgroups) of an instrumented kernel family since the last reset;
    cycles / ticks * 100 = the shader clock in MHz it held under its own load (include/zkp_hip.h)."""
    cyc, ref, waves = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    _chk(lib().zkp_profile_clock_read(name.encode(), C.byref(cyc), C.byref(ref), C.byref(waves)))
    return int(cyc.value), int(ref.value), int(waves.value)


def probe_mad_rate(launches=20):
    """-> (v_mad_u64_u32 lane-ops per second, shader clock in MHz during the probe, ms per launch) measured now on this device."""
    rate, mhz, ms = C.c_double(0), C.c_double(0), C.c_double(0)
    _chk(lib().zkp_probe_mad_rate(launches, C.byref(rate), C.byref(mhz), C.byref(ms)))
    return rate.value, mhz.value, ms.value


def _np(a, dtype, shape=None):
    a = np.ascontiguousarray(a, dtype=dtype)
    return a.reshape(shape) if shape is not None else a


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


def _stream_ptr(stream):
    if stream is None:
        try:
            import torch
            if torch.cuda.is_available():
                return C.c_void_p(torch.cuda.current_stream().cuda_stream)
        except ImportError:
            pass
        return None
    return C.c_void_p(int(stream))


def _dev_ptr(t, min_bytes):
    """torch CUDA tensor -> device pointer (contiguous, big enough)."""
    if not t.is_cuda or not t.is_contiguous():
        raise ZkpError(ZKP_E_ARG, "expected a contiguous CUDA tensor")
    if t.numel() * t.element_size() < min_bytes:
        raise ZkpError(ZKP_E_ARG, "tensor smaller than the operation needs")
    return C.c_void_p(t.data_ptr())


class _Handle:
    """An opaque handle of the library in ``_h``, released once through the entry ``_destroy`` names; csrc/kzg_handle.inc is the other
    side.  close() after close(), on a null handle or on an instance whose creation failed before ``_h`` was set does nothing."""

    _destroy = None  # the zkp_*_destroy of the subclass

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            getattr(lib(), self._destroy)(h)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------- bases / MSM
class _BasesExpansion(C.Structure):  # zkp_bases_expansion in include/zkp_hip.h
    _fields_ = [("window_bits", C.c_uint), ("slices", C.c_uint), ("planes", C.c_uint), ("glv", C.c_uint), ("widest_slice_bits", C.c_uint),
                ("bytes", C.c_size_t)]


class _G1Validation(C.Structure):  # zkp_g1_validation in include/zkp_hip.h
    _fields_ = [("checked", C.c_uint64), ("bad", C.c_uint64), ("non_canonical", C.c_uint64), ("off_curve", C.c_uint64),
                ("outside_subgroup", C.c_uint64), ("first_bad", C.c_uint64), ("first_status", C.c_int)]


G1_VALID, G1_NON_CANONICAL, G1_OFF_CURVE, G1_OUTSIDE_SUBGROUP = 0, 1, 2, 3  # status byte of a point


def _validation_dict(v):
    return {name: int(getattr(v, name)) for name, _ in _G1Validation._fields_}


def g1_validate(xy, is_inf=None, want_status=False):
    """zkp_g1_validate: n x 12 limbs of host memory checked on the GPU (canonical, on the curve, in G1) -> the report as a dict of
    checked, bad, non_canonical, off_curve, outside_subgroup, first_bad, first_status; with want_status (report, (n,) uint8 statuses)."""
    xy = _np(xy, np.uint64, (-1, 12))
    inf = _np(is_inf, np.uint8) if is_inf is not None else None
    status = np.zeros(xy.shape[0], dtype=np.uint8) if want_status else None
    v = _G1Validation()
    _chk(lib().zkp_g1_validate(_ptr(xy), _ptr(inf), xy.shape[0], _ptr(status), C.byref(v)))
    return (_validation_dict(v), status) if want_status else _validation_dict(v)


def g1_validate_dev(xy_tensor, n, is_inf_tensor=None, status_tensor=None, stream=None):
    """zkp_g1_validate_dev: the same over n x 12 limbs resident on the device; status_tensor: n bytes on the device, or None."""
    inf = _dev_ptr(is_inf_tensor, n) if is_inf_tensor is not None else None
    st = _dev_ptr(status_tensor, n) if status_tensor is not None else None
    v = _G1Validation()
    _chk(lib().zkp_g1_validate_dev(_dev_ptr(xy_tensor, 96 * n), inf, n, st, _stream_ptr(stream), C.byref(v)))
    return _validation_dict(v)


class _G1Decoding(C.Structure):  # zkp_g1_decoding in include/zkp_hip.h
    _fields_ = [("checked", C.c_uint64), ("bad", C.c_uint64), ("malformed", C.c_uint64), ("non_canonical", C.c_uint64),
                ("off_curve", C.c_uint64), ("outside_subgroup", C.c_uint64), ("first_bad", C.c_uint64), ("first_status", C.c_int)]


G1_MALFORMED = 4                # status byte of a compressed point that is no encoding at all (the others as above)
G1_DECODE_SUBGROUP = 1          # ZKP_G1_DECODE_SUBGROUP
_G1_STATUS_WORD = {G1_NON_CANONICAL: "canonical", G1_OFF_CURVE: "curve", G1_OUTSIDE_SUBGROUP: "subgroup", G1_MALFORMED: "encoding"}


def _decoding_dict(v):
    return {name: int(getattr(v, name)) for name, _ in _G1Decoding._fields_}


def _bytes48(data):
    return _np(np.frombuffer(data, dtype=np.uint8).copy() if isinstance(data, (bytes, bytearray, memoryview)) else data, np.uint8, (-1, 48))


def g1_decompress(data, check_subgroup=True, want_status=False):
    """zkp_g1_decompress: n x 48 bytes of compressed points (bytes or a uint8 array) decoded on the GPU -> ((n, 12) limbs, (n,) infinity
    flags, report dict of checked, bad, malformed, non_canonical, off_curve, outside_subgroup, first_bad, first_status), and the (n,) uint8
    statuses with want_status.  A point that does not decode is zeros with flag 0 and a non-zero status; nothing is raised for it."""
    b = _bytes48(data)
    n = b.shape[0]
    xy, inf = np.zeros((n, 12), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    status = np.zeros(n, dtype=np.uint8) if want_status else None
    v = _G1Decoding()
    _chk(lib().zkp_g1_decompress(_ptr(b), n, G1_DECODE_SUBGROUP if check_subgroup else 0, _ptr(xy), _ptr(inf), _ptr(status), C.byref(v)))
    return (xy, inf, _decoding_dict(v), status) if want_status else (xy, inf, _decoding_dict(v))


def g1_decompress_dev(bytes_tensor, n, out_xy_tensor, out_inf_tensor, check_subgroup=True, status_tensor=None, stream=None):
    """zkp_g1_decompress_dev: the same with the 48 n bytes, the 96 n bytes of limbs, the n flags and the n statuses (or None) resident on
    the device -> the report dict.  Blocks until the report is there."""
    st = _dev_ptr(status_tensor, n) if status_tensor is not None else None
    v = _G1Decoding()
    _chk(lib().zkp_g1_decompress_dev(_dev_ptr(bytes_tensor, 48 * n), n, G1_DECODE_SUBGROUP if check_subgroup else 0,
                                     _dev_ptr(out_xy_tensor, 96 * n), _dev_ptr(out_inf_tensor, n), st, _stream_ptr(stream), C.byref(v)))
    return _decoding_dict(v)


def g1_compress(xy, is_inf=None):
    """zkp_g1_compress: (n, 12) limbs and optional infinity flags -> (n, 48) uint8.  No validation."""
    xy = _np(xy, np.uint64, (-1, 12))
    inf = _np(is_inf, np.uint8, (xy.shape[0],)) if is_inf is not None else None
    out = np.zeros((xy.shape[0], 48), dtype=np.uint8)
    _chk(lib().zkp_g1_compress(_ptr(xy), _ptr(inf), xy.shape[0], _ptr(out)))
    return out


def g1_compress_dev(xy_tensor, n, out_bytes_tensor, is_inf_tensor=None, stream=None):
    """zkp_g1_compress_dev: the same on the device; nothing is synchronised."""
    inf = _dev_ptr(is_inf_tensor, n) if is_inf_tensor is not None else None
    _chk(lib().zkp_g1_compress_dev(_dev_ptr(xy_tensor, 96 * n), inf, n, _dev_ptr(out_bytes_tensor, 48 * n), _stream_ptr(stream)))


def fr_from_bytes_dev(bytes_tensor, n, out_tensor, big_endian=True, stream=None):
    """zkp_fr_from_bytes_dev: n x 32 bytes of canonical scalars on the device -> n x 4 limbs of the Fr memory form on the device;
    -> (number of values >= r, lowest such index or n).  Their slots are zeroed."""
    bad, first = C.c_uint64(0), C.c_uint64(0)
    _chk(lib().zkp_fr_from_bytes_dev(_dev_ptr(bytes_tensor, 32 * n), n, int(bool(big_endian)), _dev_ptr(out_tensor, 32 * n), _stream_ptr(stream),
                                     C.byref(bad), C.byref(first)))
    return int(bad.value), int(first.value)


def fr_to_bytes_dev(in_tensor, n, out_bytes_tensor, big_endian=True, stream=None):
    """zkp_fr_to_bytes_dev: the way back; nothing is synchronised."""
    _chk(lib().zkp_fr_to_bytes_dev(_dev_ptr(in_tensor, 32 * n), n, int(bool(big_endian)), _dev_ptr(out_bytes_tensor, 32 * n), _stream_ptr(stream)))


def srs_check(bases, g2s, n, r):
    """zkp_srs_check: are the first n points of the handle [s^i]G for the s behind g2s = [s]_2?  r: (n - 1, 4) random Fr limbs.
    -> 1 accepted, 0 rejected.  Assumes valid points: G1Bases.validate() first."""
    g2s = _np(g2s, np.uint64, (24,))
    r = _np(r, np.uint64, (-1, 4)) if n > 1 else None
    if r is not None and r.shape[0] < n - 1:
        raise ZkpError(ZKP_E_ARG, "srs_check needs n - 1 random scalars")
    ok = C.c_int(0)
    _chk(lib().zkp_srs_check(bases._h, _ptr(g2s), n, _ptr(r), C.byref(ok)))
    return int(ok.value)


class G1Bases(_Handle):
    """Base points resident in HBM (the SRS of kzg/src/srs.rs:14-21, uploaded once)."""
    _destroy = "zkp_g1_bases_destroy"

    def __init__(self, handle):
        self._h = handle

    @classmethod
    def from_host(cls, xy, is_inf=None):
        xy = _np(xy, np.uint64, (-1, 12))
        inf = _np(is_inf, np.uint8) if is_inf is not None else None
        h = C.c_void_p()
        _chk(lib().zkp_g1_bases_create(_ptr(xy), _ptr(inf), xy.shape[0], C.byref(h)))
        return cls(h)

    @classmethod
    def from_device(cls, xy_tensor, n, is_inf_tensor=None, stream=None):
        h = C.c_void_p()
        inf = C.c_void_p(is_inf_tensor.data_ptr()) if is_inf_tensor is not None else None
        _chk(lib().zkp_g1_bases_create_dev(_dev_ptr(xy_tensor, 96 * n), inf, n, _stream_ptr(stream), C.byref(h)))
        return cls(h)

    @classmethod
    def from_compressed(cls, data, check_subgroup=True):
        """zkp_g1_bases_create_compressed: n x 48 bytes of compressed points, decoded on the GPU straight into the handle (one slot, never
        sharded).  A point that does not decode raises ZkpError(ZKP_E_ARG) naming its index; ``.report`` of the error is the report dict."""
        b = _bytes48(data)
        h, v = C.c_void_p(), _G1Decoding()
        code = lib().zkp_g1_bases_create_compressed(_ptr(b), b.shape[0], G1_DECODE_SUBGROUP if check_subgroup else 0, C.byref(v), C.byref(h))
        if code != ZKP_OK:
            err = ZkpError(code, lib().zkp_last_error().decode())
            err.report = _decoding_dict(v)
            raise err
        return cls(h)

    def precompute(self, window_bits=20, glv=False):
        """Expand to the multiples 2^(window_bits s) P (shared-bucket MSM, see include/zkp_hip.h).  glv: the endomorphism-split
        expansion (zkp_g1_bases_precompute_glv), about half as many planes for the same results."""
        _chk((lib().zkp_g1_bases_precompute_glv if glv else lib().zkp_g1_bases_precompute)(self._h, window_bits))
        return self

    def expansion(self):
        """zkp_g1_bases_expansion -> dict(window_bits, slices, planes, glv, widest_slice_bits, bytes); all zero when not expanded."""
        e = _BasesExpansion()
        _chk(lib().zkp_g1_bases_expansion(self._h, C.byref(e)))
        return {name: int(getattr(e, name)) for name, _ in _BasesExpansion._fields_}

    def validate(self, want_status=False):
        """zkp_g1_bases_validate: every point of the handle on the curve and in G1 (statuses 0, 2, 3) -> report dict, or
        (report, (len,) uint8 statuses).  Call it before precompute(glv=True) on points that were not checked elsewhere."""
        status = np.zeros(len(self), dtype=np.uint8) if want_status else None
        v = _G1Validation()
        _chk(lib().zkp_g1_bases_validate(self._h, _ptr(status), C.byref(v)))
        return (_validation_dict(v), status) if want_status else _validation_dict(v)

    def lagrange(self, log_n):
        """zkp_g1_bases_lagrange: the inverse point transform of the first 2^log_n points as a new handle -- [L_i(s)]G for an SRS
        [s^i]G, so that kzg_commit(lagrange, evals) commits to the interpolant of evals on the domain."""
        h = C.c_void_p()
        _chk(lib().zkp_g1_bases_lagrange(self._h, log_n, C.byref(h)))
        return G1Bases(h)

    def shards(self):
        """[(slot, hip_device, offset, length)] of the chunks of this handle (one entry for a single-slot handle)."""
        out = []
        for i in range(lib().zkp_g1_bases_shard_count(self._h)):
            slot, dev, off, ln = C.c_int(0), C.c_int(0), C.c_size_t(0), C.c_size_t(0)
            _chk(lib().zkp_g1_bases_shard(self._h, i, C.byref(slot), C.byref(dev), C.byref(off), C.byref(ln)))
            out.append((int(slot.value), int(dev.value), int(off.value), int(ln.value)))
        return out

    def info(self):
        """-> (window_bits asked for, slices = insertions per scalar); (0, 0) when not expanded."""
        w, sl = C.c_uint(0), C.c_uint(0)
        _chk(lib().zkp_g1_bases_info(self._h, C.byref(w), C.byref(sl)))
        return int(w.value), int(sl.value)

    def __len__(self):
        return int(lib().zkp_g1_bases_len(self._h))


def msm_g1(bases, scalars, bits=None):
    """sum_i scalars[i] * bases[i]  ->  ((12,) uint64 affine Montgomery coords, is_infinity).  Host scalars.
    bits: every canonical scalar is below 2**bits (zkp_msm_g1_bits: only the slices such scalars fill are run; a scalar past the
    bound is ZKP_E_ARG).  None: whole scalars."""
    scalars = _np(scalars, np.uint64, (-1, 4))
    out = np.zeros(12, dtype=np.uint64)
    inf = C.c_uint8(0)
    if bits is None:
        _chk(lib().zkp_msm_g1(bases._h, _ptr(scalars), scalars.shape[0], _ptr(out), C.byref(inf)))
    else:
        _chk(lib().zkp_msm_g1_bits(bases._h, _ptr(scalars), scalars.shape[0], bits, _ptr(out), C.byref(inf)))
    return out, int(inf.value)


def msm_g1_partial(bases, scalars):
    """Host scalars -> (24,) uint64 extended-Jacobian partial (summed over this process's devices for sharded bases)."""
    scalars = _np(scalars, np.uint64, (-1, 4))
    out = np.zeros(24, dtype=np.uint64)
    _chk(lib().zkp_msm_g1_partial(bases._h, _ptr(scalars), scalars.shape[0], _ptr(out)))
    return out


def msm_g1_sharded_dev(bases, scalar_tensors, n, events=None):
    """Sharded bases, one resident scalar tensor per chunk (on that chunk's device; None for a chunk beyond n) -> (affine, is_inf).

    Without `events` the library launches on each slot's own stream after a hipDeviceSynchronize() of that chunk's device, so tensors
    whose producing copy / kernel is still in flight on any torch stream are safe to pass.  With `events` (one recorded
    torch.cuda.Event, or None, per chunk) the chunk's launch waits for its event on the device instead and the host does not stall
    (include/zkp_hip.h, zkp_msm_g1_sharded_dev / zkp_msm_g1_sharded_dev_after)."""
    k = len(scalar_tensors)
    ptrs = (C.c_void_p * k)(*[(t.data_ptr() if t is not None else None) for t in scalar_tensors])
    out = np.zeros(12, dtype=np.uint64)
    inf = C.c_uint8(0)
    if events is None:
        _chk(lib().zkp_msm_g1_sharded_dev(bases._h, ptrs, n, _ptr(out), C.byref(inf)))
    else:
        if len(events) != k:
            raise ValueError("one event (or None) per chunk")
        evs = (C.c_void_p * k)(*[(e.cuda_event if e is not None else None) for e in events])
        _chk(lib().zkp_msm_g1_sharded_dev_after(bases._h, ptrs, evs, n, _ptr(out), C.byref(inf)))
    return out, int(inf.value)


def selftest_fq_inverse_dev(in_tensor, n, form, out_tensor, stream=None):
    """zkp_selftest_fq_inverse_dev: n raw base-field elements (form 0: 12 x u32, form 1: 16 x u32 per element) inverted on the device."""
    words = 12 if form == 0 else 16
    _chk(lib().zkp_selftest_fq_inverse_dev(_dev_ptr(in_tensor, 4 * words * n), n, form, _dev_ptr(out_tensor, 4 * words * n),
                                           _stream_ptr(stream)))


def selftest_fr_inverse_dev(in_tensor, n, method, out_tensor, stream=None):
    """zkp_selftest_fr_inverse_dev: n scalar-field elements (8 x u32 each, the memory form) inverted on the device, one lane each.
    method 0: division steps (csrc/fr_inv.hpp), 1: the Fermat power."""
    _chk(lib().zkp_selftest_fr_inverse_dev(_dev_ptr(in_tensor, 32 * n), n, method, _dev_ptr(out_tensor, 32 * n), _stream_ptr(stream)))


# operation numbers of the lane-level self-tests (the enums of csrc/selftest.hpp; tests/test_limb_model_cpu.py compares the two)
SELFTEST_OPS = {
    "fq28": {"mul_inline": 0, "mul_chain": 1, "mul_chain2": 2, "sqr": 3, "sqr_chain": 4, "mul2": 5, "mul2_chain": 6, "normalise": 7,
             "sub4": 8, "sub8": 9, "sub16": 10, "sub8w": 11, "neg4": 12, "is_zero": 13, "from_sat": 14, "mul_chain2_inplace": 15},
    "fr29": {"mul": 0, "mul2": 1, "to_canonical": 2, "fr_mul": 3, "sub_tight": 4, "sub_wide8": 5, "normalise": 6, "pack_tight": 7,
             "from_sat_shl5": 8, "twiddle": 9, "from_sat": 10},
    "fp": {"add": 0, "sub": 1, "neg": 2, "dbl": 3, "mul": 4, "mont_mul": 5},
    "gl": {"add": 0, "sub": 1, "neg": 2, "mul": 3, "reduce128": 4},
    "g1": {"madd": 0, "madd_chain": 1, "mmadd": 2, "mmadd_chain": 3, "add": 4, "double": 5, "double_affine": 6, "add_stream": 7,
           "add_stream_chain": 8, "add_inplace": 9, "add_inplace_chain": 10, "add_quad": 11, "add_quad_inplace": 12},
}


def selftest_field_dev(family, op, in_tensor, n, out_tensor, stream=None):
    """zkp_selftest_{fq28,fr29,fp,gl}_dev: n cases, 64 input words and 32 output words each (int32 tensors).  family: "fq28", "fr29", "gl",
    "fq" or "fr" (the saturated forms); op: a name of SELFTEST_OPS."""
    args = (_dev_ptr(in_tensor, 256 * n), n, _dev_ptr(out_tensor, 128 * n), _stream_ptr(stream))
    if family in ("fq", "fr"):
        _chk(lib().zkp_selftest_fp_dev(0 if family == "fq" else 1, SELFTEST_OPS["fp"][op], *args))
    else:
        _chk(getattr(lib(), f"zkp_selftest_{family}_dev")(SELFTEST_OPS[family][op], *args))


def selftest_glv_split_dev(scalars_tensor, n, out_tensor, stream=None):
    """zkp_selftest_glv_split_dev: n Fr in memory form (32 B each) -> 8 words per case (k mod lambda, k div lambda)."""
    _chk(lib().zkp_selftest_glv_split_dev(_dev_ptr(scalars_tensor, 32 * n), n, _dev_ptr(out_tensor, 32 * n), _stream_ptr(stream)))


def selftest_g1_dev(op, a_tensor, b_tensor, n, stride, out_tensor, flag_tensor, stream=None):
    """zkp_selftest_g1_dev: the point arrays hold 64 words per point (register forms: n points; plane-major forms: 16 chunks x stride);
    a_tensor may be None for the in-place forms."""
    pts = 256 * (stride if SELFTEST_OPS["g1"][op] >= 7 else n)
    _chk(lib().zkp_selftest_g1_dev(SELFTEST_OPS["g1"][op], _dev_ptr(a_tensor, pts) if a_tensor is not None else None, _dev_ptr(b_tensor, pts),
                                   n, stride, _dev_ptr(out_tensor, pts), _dev_ptr(flag_tensor, 4 * n), _stream_ptr(stream)))


# ---- self-test hooks of the polynomial layer (zkp_selftest_poly_*_dev): tensors hold Fr in memory form, 32 B per element; a tensor given
# as None is passed as a null pointer (the library refuses it)
def _fr_ptrs(tensors, lens):
    return (C.c_void_p * max(len(tensors), 1))(*[None if t is None else _dev_ptr(t, 32 * int(n)).value for t, n in zip(tensors, lens)])


def _sizes(lens):
    return (C.c_size_t * max(len(lens), 1))(*[int(n) for n in lens])


def selftest_poly_scan_dev(op, jobs, chunk=0, stream=None):
    """zkp_selftest_poly_scan_dev: op "add" or "mul"; jobs = one or two (in_tensor, out_tensor, n, rev, excl); chunk 0 = the production rule."""
    lens = [j[2] for j in jobs]
    flags = (C.c_uint * max(len(jobs), 1))(*[int(bool(j[3])) | int(bool(j[4])) << 1 for j in jobs])
    _chk(lib().zkp_selftest_poly_scan_dev({"add": 0, "mul": 1}[op], len(jobs), _fr_ptrs([j[0] for j in jobs], lens),
                                          _fr_ptrs([j[1] for j in jobs], lens), _sizes(lens), flags, chunk, _stream_ptr(stream)))


def selftest_poly_scale_pow_dev(in_tensor, n, base, e0, out_tensor, chunk=0, stream=None):
    """zkp_selftest_poly_scale_pow_dev: out[i] = in[i] * base^(i + e0); base = 4 Montgomery limbs."""
    _chk(lib().zkp_selftest_poly_scale_pow_dev(_fr_ptrs([in_tensor], [n])[0], n, _ptr(_np(base, np.uint64, (4,))), e0, chunk,
                                               _fr_ptrs([out_tensor], [n])[0], _stream_ptr(stream)))


def selftest_poly_div_linear_dev(reqs, chunk=0, stream=None):
    """zkp_selftest_poly_div_linear_dev: reqs = one or two (c_tensor, len, z, out_tensor); out receives the len - 1 coefficients of
    (c(X) - c(z)) / (X - z)."""
    lens = [r[1] for r in reqs]
    z = _np([r[2] for r in reqs], np.uint64, (-1, 4)) if reqs else np.zeros((1, 4), dtype=np.uint64)
    _chk(lib().zkp_selftest_poly_div_linear_dev(len(reqs), _fr_ptrs([r[0] for r in reqs], lens), _sizes(lens), _ptr(z),
                                                _fr_ptrs([r[3] for r in reqs], [max(n, 1) - 1 for n in lens]), chunk, _stream_ptr(stream)))


def selftest_poly_eval_dev(reqs, stream=None):
    """zkp_selftest_poly_eval_dev: reqs = up to eight (c_tensor, len, z) -> (len(reqs), 4) array of c(z)."""
    lens = [r[1] for r in reqs]
    z = _np([r[2] for r in reqs], np.uint64, (-1, 4)) if reqs else np.zeros((1, 4), dtype=np.uint64)
    out = np.zeros((max(len(reqs), 1), 4), dtype=np.uint64)
    _chk(lib().zkp_selftest_poly_eval_dev(len(reqs), _fr_ptrs([r[0] for r in reqs], lens), _sizes(lens), _ptr(z), _ptr(out), _stream_ptr(stream)))
    return out[:len(reqs)]


def selftest_poly_lincomb_dev(terms, n_out, out_tensor, stream=None):
    """zkp_selftest_poly_lincomb_dev: terms = up to twelve (p_tensor, len, s); out[i] = sum_k s_k p_k[i] over the terms with i < len_k."""
    lens = [t[1] for t in terms]
    s = _np([t[2] for t in terms], np.uint64, (-1, 4)) if terms else np.zeros((1, 4), dtype=np.uint64)
    _chk(lib().zkp_selftest_poly_lincomb_dev(len(terms), _fr_ptrs([t[0] for t in terms], lens), _sizes(lens), _ptr(s), n_out,
                                             _fr_ptrs([out_tensor], [n_out])[0], _stream_ptr(stream)))


def selftest_poly_trim_len_dev(c_tensor, n, stream=None):
    """zkp_selftest_poly_trim_len_dev: the highest index of a non-zero element of c[0..n), plus one; 0 for none."""
    out = C.c_size_t(0)
    _chk(lib().zkp_selftest_poly_trim_len_dev(_fr_ptrs([c_tensor], [n])[0], n, C.byref(out), _stream_ptr(stream)))
    return int(out.value)


# outputs of zkp_selftest_msm_sort_dev in the order of the ZKP_SORT_* enum of include/zkp_hip.h
MSM_SORT_OUTPUTS = ("digits", "entries", "pstart", "ghist", "start", "sorted", "perm", "over", "over_b", "over_off", "desc")


class _MsmSortGeometry(C.Structure):  # zkp_msm_sort_geometry in include/zkp_hip.h
    _fields_ = [(k, C.c_uint32) for k in ("c", "nwin", "nb", "nslice", "shared", "glv", "nchunk", "lo_bits", "nhi", "run_limit", "piece",
                                          "over_cap", "desc_cap", "ps_tile", "nranges", "range_index")] + \
               [(k, C.c_uint64) for k in ("n", "ns", "chunk", "range_off", "range_len")] + \
               [("out_words", C.c_uint64 * len(MSM_SORT_OUTPUTS)), ("off", C.c_uint16 * 36)]


class _MsmSortOutputs(C.Structure):  # zkp_msm_sort_outputs in include/zkp_hip.h
    _fields_ = [("d_out", C.c_void_p * len(MSM_SORT_OUTPUTS)), ("words", C.c_size_t * len(MSM_SORT_OUTPUTS))]


def selftest_msm_sort_dev(bases, scalar_tensors, n, range_index=0, out_tensors=None, stream=None, bits=None):
    """zkp_selftest_msm_sort_dev: plan the MSM of the scalar vectors (each n x 32 B, resident) over ``bases`` and run the digits + sort
    of one scalar range.  out_tensors None: -> the geometry dict only (its "out_words" names the int32 words of every output);
    otherwise a dict of int32 CUDA tensors keyed by MSM_SORT_OUTPUTS, which receive the outputs -> the geometry dict.
    bits: the plan and the digits kernel of the bounded entries (zkp_selftest_msm_sort_bits_dev)."""
    k = len(scalar_tensors)
    ptrs = (C.c_void_p * max(k, 1))(*[_dev_ptr(t, 32 * n).value for t in scalar_tensors])
    g, o = _MsmSortGeometry(), None
    if out_tensors is not None:
        o = _MsmSortOutputs()
        for i, name in enumerate(MSM_SORT_OUTPUTS):
            t = out_tensors[name]
            o.d_out[i] = _dev_ptr(t, 0).value if t is not None and t.numel() else None
            o.words[i] = t.numel() * t.element_size() // 4 if t is not None else 0
    h, po = bases._h if bases is not None else None, C.byref(o) if o is not None else None
    if bits is None:
        _chk(lib().zkp_selftest_msm_sort_dev(h, ptrs, k, n, range_index, _stream_ptr(stream), C.byref(g), po))
    else:
        _chk(lib().zkp_selftest_msm_sort_bits_dev(h, ptrs, k, n, range_index, bits, _stream_ptr(stream), C.byref(g), po))
    d = {name: int(getattr(g, name)) for name, _ in _MsmSortGeometry._fields_[:21]}
    d["out_words"] = {name: int(g.out_words[i]) for i, name in enumerate(MSM_SORT_OUTPUTS)}
    d["off"] = [int(x) for x in g.off[:d["nslice"] + 1]]
    return d


class _MsmReduceLevel(C.Structure):  # zkp_msm_reduce_level in include/zkp_hip.h
    _fields_ = [(k, C.c_uint32) for k in ("level", "half", "quad", "grid_x")]


class _MsmFoldStep(C.Structure):  # zkp_msm_fold_step
    _fields_ = [(k, C.c_uint32) for k in ("pairs", "lane", "grid_x")]


_MSM_REDUCE_WORDS = ("bucket_words", "parts_words", "over_words", "over_b_words", "over_off_words", "pieces_words", "carry_words",
                     "result_words", "flag_words")


class _MsmReduceGeometry(C.Structure):  # zkp_msm_reduce_geometry
    _fields_ = [(k, C.c_uint32) for k in ("c", "nwin", "nb", "split_log", "tail_max_waves", "nlevel", "tail_blocks", "tail_threads",
                                          "combine_x", "over_cap", "desc_cap", "reserved")] + \
               [("cap", C.c_uint64), ("level", _MsmReduceLevel * 24), ("fold", _MsmFoldStep * 2)] + [(k, C.c_uint64) for k in _MSM_REDUCE_WORDS]


_MSM_REDUCE_IN = ("buckets", "parts", "over", "over_b", "over_off", "pieces", "carry")


class _MsmReduceIo(C.Structure):  # zkp_msm_reduce_io
    _fields_ = [(k, C.c_uint32) for k in ("c", "nwin", "split_log", "over_cap", "desc_cap", "resume", "more", "reserved")] + \
               [("d_" + k, C.c_void_p) for k in _MSM_REDUCE_IN] + [(k + "_words", C.c_size_t) for k in _MSM_REDUCE_IN] + \
               [("d_out_buckets", C.c_void_p), ("d_out_carry", C.c_void_p), ("out_buckets_words", C.c_size_t), ("out_carry_words", C.c_size_t),
                ("out_results", C.c_void_p), ("out_flags", C.c_void_p), ("out_results_words", C.c_size_t), ("out_flags_words", C.c_size_t)]


def selftest_msm_reduce_dev(c, nwin, split_log=0, buckets=None, parts=None, combine=None, out_buckets=None, run=True, stream=None, slot=-1):
    """zkp_selftest_msm_reduce_dev: the MSM's combine, fold and bucket reduction on bucket contents of the caller's.
    buckets / parts / out_buckets: int32 CUDA tensors in the plane-major layout; combine: None or a dict with over_cap, desc_cap, the
    int32 CUDA tensors over, over_b, over_off, pieces, optionally carry (-> resume), more (flag) and out_carry (required with more).
    run=False: nothing is launched.  -> (geometry dict, results (nwin, c, 64) uint32 or None, flags (nwin,) uint32 or None); under
    more the results and flags are returned as they were handed in: all 0xFF."""
    io, g = _MsmReduceIo(), _MsmReduceGeometry()
    io.c, io.nwin, io.split_log = c, nwin, split_log

    def put(name, t, prefix="d_"):
        if t is not None:
            setattr(io, prefix + name, _dev_ptr(t, 0).value if t.numel() else None)
            setattr(io, name + "_words", t.numel() * t.element_size() // 4)

    put("buckets", buckets)
    put("parts", parts)
    put("out_buckets", out_buckets)
    if combine is not None:
        io.over_cap, io.desc_cap = combine["over_cap"], combine["desc_cap"]
        io.resume, io.more = int(combine.get("carry") is not None), int(bool(combine.get("more")))
        for k in ("over", "over_b", "over_off", "pieces", "carry"):
            put(k, combine.get(k))
        put("out_carry", combine.get("out_carry"))
    res = flags = None
    if run:
        res = np.full((max(nwin, 1), max(c, 1), 64), 0xFFFFFFFF, dtype=np.uint32)
        flags = np.full(max(nwin, 1), 0xFFFFFFFF, dtype=np.uint32)
        io.out_results, io.out_flags = res.ctypes.data, flags.ctypes.data
        io.out_results_words, io.out_flags_words = res.size, flags.size
    _chk(lib().zkp_selftest_msm_reduce_dev(slot, C.byref(io), _stream_ptr(stream), C.byref(g)))
    d = {k: int(getattr(g, k)) for k, _ in _MsmReduceGeometry._fields_ if k not in ("level", "fold", "reserved")}
    d["level"] = [{k: int(getattr(g.level[i], k)) for k, _ in _MsmReduceLevel._fields_} for i in range(d["nlevel"])]
    d["fold"] = [{k: int(getattr(g.fold[i], k)) for k, _ in _MsmFoldStep._fields_} for i in range(d["split_log"])]
    return d, res, flags


def msm_g1_dev(bases, scalars_tensor, n, stream=None, bits=None):
    """Resident scalars.  bits: as msm_g1 (zkp_msm_g1_bits_dev); fr_bit_length_dev finds the smallest bound a vector allows."""
    out = np.zeros(12, dtype=np.uint64)
    inf = C.c_uint8(0)
    if bits is None:
        _chk(lib().zkp_msm_g1_dev(bases._h, _dev_ptr(scalars_tensor, 32 * n), n, _stream_ptr(stream), _ptr(out),
                                  C.byref(inf)))
    else:
        _chk(lib().zkp_msm_g1_bits_dev(bases._h, _dev_ptr(scalars_tensor, 32 * n), n, bits, _stream_ptr(stream), _ptr(out),
                                       C.byref(inf)))
    return out, int(inf.value)


def msm_g1_batch_dev(bases, scalar_tensors, n, stream=None, bits=None):
    """Several MSMs over the same bases in one pass (equal length n): list of (affine (12,), is_inf).
    bits: one bound for every vector (zkp_msm_g1_batch_bits_dev)."""
    k = len(scalar_tensors)
    ptrs = (C.c_void_p * k)(*[_dev_ptr(t, 32 * n).value for t in scalar_tensors])
    xy, inf = np.zeros((k, 12), dtype=np.uint64), np.zeros(k, dtype=np.uint8)
    if bits is None:
        _chk(lib().zkp_msm_g1_batch_dev(bases._h, ptrs, k, n, _stream_ptr(stream), _ptr(xy), _ptr(inf)))
    else:
        _chk(lib().zkp_msm_g1_batch_bits_dev(bases._h, ptrs, k, n, bits, _stream_ptr(stream), _ptr(xy), _ptr(inf)))
    return [(xy[i].copy(), int(inf[i])) for i in range(k)]


def fr_bit_length_dev(tensor, n, stream=None):
    """zkp_fr_bit_length_dev: the largest bit length among the n resident scalars of ``tensor`` (0 for none or all zeros).  Blocks."""
    bits = C.c_uint(0)
    _chk(lib().zkp_fr_bit_length_dev(_dev_ptr(tensor, 32 * n) if n else None, n, _stream_ptr(stream), C.byref(bits)))
    return int(bits.value)


def msm_g1_partial_dev(bases, scalars_tensor, n, stream=None):
    """Unnormalised partial sum (X, Y, ZZ, ZZZ) as (24,) uint64 -- the multi-GPU exchange unit."""
    out = np.zeros(24, dtype=np.uint64)
    _chk(lib().zkp_msm_g1_partial_dev(bases._h, _dev_ptr(scalars_tensor, 32 * n), n, _stream_ptr(stream), _ptr(out)))
    return out


def g1_xyzz_sum(partials):
    partials = _np(partials, np.uint64, (-1, 24))
    out = np.zeros(12, dtype=np.uint64)
    inf = C.c_uint8(0)
    _chk(lib().zkp_g1_xyzz_sum(_ptr(partials), partials.shape[0], _ptr(out), C.byref(inf)))
    return out, int(inf.value)


def g1_mul(base_xy, base_inf, scalar):
    base_xy, scalar = _np(base_xy, np.uint64, (12,)), _np(scalar, np.uint64, (4,))
    out = np.zeros(12, dtype=np.uint64)
    inf = C.c_uint8(0)
    _chk(lib().zkp_g1_mul(_ptr(base_xy), int(base_inf), _ptr(scalar), _ptr(out), C.byref(inf)))
    return out, int(inf.value)


def g1_fixed_base_mul_dev(scalars_tensor, n, out_xy_tensor, out_inf_tensor=None, stream=None):
    inf = C.c_void_p(out_inf_tensor.data_ptr()) if out_inf_tensor is not None else None
    _chk(lib().zkp_g1_fixed_base_mul_dev(_dev_ptr(scalars_tensor, 32 * n), n, _dev_ptr(out_xy_tensor, 96 * n), inf,
                                         _stream_ptr(stream)))


def srs_g1(secret, n):
    """[s^i]G, i < n (kzg/src/srs.rs:48-63) -> (n,12) uint64."""
    secret = _np(secret, np.uint64, (4,))
    out = np.zeros((n, 12), dtype=np.uint64)
    _chk(lib().zkp_srs_g1(_ptr(secret), n, _ptr(out)))
    return out


# ----------------------------------------------------------------------------- NTT
def _log2(n):
    lg = int(n).bit_length() - 1
    if n <= 0 or (1 << lg) != n:
        raise ZkpError(ZKP_E_ARG, "size must be a power of two")
    return lg


def ntt_fr(data, inverse=False, coset=None):
    a = _np(data, np.uint64, (-1, 4)).copy()
    cs = _np(coset, np.uint64, (4,)) if coset is not None else None
    _chk(lib().zkp_ntt_fr(_ptr(a), _log2(a.shape[0]), int(bool(inverse)), _ptr(cs)))
    return a


def ntt_goldilocks(data, inverse=False, coset=None):
    a = _np(data, np.uint64).reshape(-1).copy()
    cs = _np(coset, np.uint64, (1,)) if coset is not None else None
    _chk(lib().zkp_ntt_goldilocks(_ptr(a), _log2(a.shape[0]), int(bool(inverse)), _ptr(cs)))
    return a


def ntt_fr_dev(tensor, log_n, batch=1, inverse=False, coset=None, stream=None):
    cs = _np(coset, np.uint64, (4,)) if coset is not None else None
    _chk(lib().zkp_ntt_fr_dev(_dev_ptr(tensor, (32 << log_n) * batch), log_n, batch, int(bool(inverse)), _ptr(cs),
                              _stream_ptr(stream)))


def ntt_fr_twiddle_dev(tensor, rows, cols, row0, log_n, inverse=False, stream=None):
    """tensor[r][c] *= omega_n^((row0 + r) * c) for a rows x cols row-major block (four-step transform, dist.py)."""
    _chk(lib().zkp_ntt_fr_twiddle_dev(_dev_ptr(tensor, 32 * rows * cols), rows, cols, row0, log_n, int(bool(inverse)),
                                      _stream_ptr(stream)))


class NttLayout(C.Structure):  # zkp_ntt_layout in include/zkp_hip.h (strides in elements)
    _fields_ = [("lo_bits", C.c_uint), ("mid_bits", C.c_uint), ("mid_stride", C.c_size_t), ("hi_stride", C.c_size_t),
                ("batch_stride", C.c_size_t)]


def ntt_fr_axis0_dev(t_in, t_out, log_len, cols, inverse=False, tw_log_n=0, tw_col0=0, stream=None):
    """Length-2^log_len transforms along axis 0 of a row-major [2^log_len][cols] matrix, optional four-step twiddle."""
    nbytes = 32 * (cols << log_len)
    _chk(lib().zkp_ntt_fr_axis0_dev(_dev_ptr(t_in, nbytes), _dev_ptr(t_out, nbytes), log_len, cols, int(inverse), tw_log_n,
                                    tw_col0, _stream_ptr(stream)))


def ntt_fr_layout_dev(t_in, t_out, log_n, batch, inverse=False, in_layout=None, out_layout=None, tw_log_n=0, tw_row0=0,
                      stream=None):
    """`batch` transforms with a gathered input / scattered output layout (NttLayout or None), optional four-step twiddle."""
    nbytes = 32 * (batch << log_n)
    li = C.byref(in_layout) if in_layout is not None else None
    lo = C.byref(out_layout) if out_layout is not None else None
    _chk(lib().zkp_ntt_fr_layout_dev(_dev_ptr(t_in, nbytes), _dev_ptr(t_out, nbytes), log_n, batch, int(inverse),
                                     C.cast(li, C.c_void_p) if li is not None else None,
                                     C.cast(lo, C.c_void_p) if lo is not None else None, tw_log_n, tw_row0, _stream_ptr(stream)))


NTT_NATURAL, NTT_K1SLAB, NTT_COLUMNS = 0, 1, 2


class NttShardGeometry(C.Structure):  # zkp_ntt_shard_geometry in include/zkp_hip.h
    _fields_ = [("slots", C.c_uint), ("log_n1", C.c_uint), ("log_n2", C.c_uint), ("chunks", C.c_uint), ("r1", C.c_size_t),
                ("r2", C.c_size_t), ("cw", C.c_size_t), ("slab", C.c_size_t)]


def ntt_fr_sharded_geometry(log_n, slots=0, chunks=0):
    """Split of the in-process multi-GPU transform: dict(slots, log_n1, log_n2, chunks, r1, r2, cw, slab)."""
    g = NttShardGeometry()
    _chk(lib().zkp_ntt_fr_sharded_geometry(log_n, slots, chunks, C.cast(C.byref(g), C.c_void_p)))
    return {k: int(getattr(g, k)) for k, _ in NttShardGeometry._fields_}


def ntt_fr_sharded_dev(slab_tensors, log_n, inverse=False, layout_in=NTT_NATURAL, layout_out=NTT_K1SLAB, chunks=0, streams=None):
    """zkp_ntt_fr_sharded_dev: one resident slab tensor per device slot (on that slot's device), transformed in place.
    streams: None (synchronous: returns when every device is done) or one torch stream / raw handle per slot (enqueue only)."""
    k = len(slab_tensors)
    nbytes = (32 << log_n) // k
    ptrs = (C.c_void_p * k)(*[_dev_ptr(t, nbytes).value for t in slab_tensors])
    sts = None
    if streams is not None:
        if len(streams) != k:
            raise ValueError("one stream per slot")
        sts = (C.c_void_p * k)(*[int(getattr(s, "cuda_stream", s)) for s in streams])
    _chk(lib().zkp_ntt_fr_sharded_dev(ptrs, log_n, int(bool(inverse)), layout_in, layout_out, chunks, sts))


def ntt_fr_sharded(data, inverse=False, coset=None, inplace=False):
    """zkp_ntt_fr_sharded: host vector, natural order in and out, over all device slots of the process."""
    a = _np(data, np.uint64, (-1, 4))
    if not inplace:
        a = a.copy()
    cs = _np(coset, np.uint64, (4,)) if coset is not None else None
    _chk(lib().zkp_ntt_fr_sharded(_ptr(a), _log2(a.shape[0]), int(bool(inverse)), _ptr(cs)))
    return a


def ntt_goldilocks_dev(tensor, log_n, batch=1, inverse=False, coset=None, stream=None):
    cs = _np(coset, np.uint64, (1,)) if coset is not None else None
    _chk(lib().zkp_ntt_goldilocks_dev(_dev_ptr(tensor, (8 << log_n) * batch), log_n, batch, int(bool(inverse)),
                                      _ptr(cs), _stream_ptr(stream)))


def fri_layer_eval(coeffs, coset, log_d):
    """FriLayer::from_poly evaluations (fri/src/fri_layer.rs:40-46); coset is a Montgomery-form u64."""
    coeffs = _np(coeffs, np.uint64).reshape(-1)
    out = np.zeros(1 << log_d, dtype=np.uint64)
    _chk(lib().zkp_fri_layer_eval(_ptr(coeffs), coeffs.size, int(coset), log_d, _ptr(out)))
    return out


def fri_fold(coeffs, r):
    coeffs = _np(coeffs, np.uint64).reshape(-1)
    out = np.zeros((coeffs.size + 1) // 2, dtype=np.uint64)
    _chk(lib().zkp_fri_fold(_ptr(coeffs), coeffs.size, int(r), _ptr(out)))
    return out


def fri_merkle_node_count(n):
    return int(lib().zkp_fri_merkle_node_count(n))


def fri_merkle_tree(leaves):
    """MerkleTree::new (fri/src/merkle_tree.rs:42-63): every level, concatenated; the root is the last element."""
    leaves = _np(leaves, np.uint64).reshape(-1)
    out = np.zeros(fri_merkle_node_count(leaves.size), dtype=np.uint64)
    _chk(lib().zkp_fri_merkle_tree(_ptr(leaves), leaves.size, _ptr(out)))
    return out


def fri_merkle_tree_dev(leaves_tensor, n, nodes_tensor, stream=None):
    _chk(lib().zkp_fri_merkle_tree_dev(_dev_ptr(leaves_tensor, 8 * n), n, _dev_ptr(nodes_tensor, 8 * fri_merkle_node_count(n)),
                                       _stream_ptr(stream)))


def fri_challenges(roots, const_val, num_queries):
    roots = _np(roots, np.uint64).reshape(-1)
    r_out = np.zeros(roots.size, dtype=np.uint64)
    q_out = np.zeros(num_queries, dtype=np.uint64)
    _chk(lib().zkp_fri_challenges(_ptr(roots), roots.size, int(const_val), num_queries, _ptr(r_out), _ptr(q_out)))
    return r_out, q_out


def fri_prove(coeffs, blowup_factor, num_queries):
    """generate_proof (fri/src/prover.rs:141-168) -> flat proof (layout in include/zkp_hip.h)."""
    coeffs = _np(coeffs, np.uint64).reshape(-1)
    p, words = C.c_void_p(), C.c_size_t()
    _chk(lib().zkp_fri_prove(_ptr(coeffs), coeffs.size, blowup_factor, num_queries, C.byref(p), C.byref(words)))
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(words.value,)).copy()
    finally:
        lib().zkp_free(p)


def fri_verify(proof):
    """verify (fri/src/verifier.rs:10-127): True, or raises ZkpError carrying the reference's error string."""
    proof = _np(proof, np.uint64).reshape(-1)
    _chk(lib().zkp_fri_verify(_ptr(proof), proof.size))
    return True


# ----------------------------------------------------------------------------- FRI over Fr: (n, 4) uint64 memory-form arrays
def fri_layer_eval_fr(coeffs, coset, log_d):
    """FriLayer::from_poly evaluations over Fr; coset is a Montgomery-form (4,) uint64 array."""
    coeffs = _np(coeffs, np.uint64, (-1, 4))
    cs = _np(coset, np.uint64, (4,))
    out = np.zeros((1 << log_d, 4), dtype=np.uint64)
    _chk(lib().zkp_fri_layer_eval_fr(_ptr(coeffs), coeffs.shape[0], _ptr(cs), log_d, _ptr(out)))
    return out


def fri_fold_fr(coeffs, r):
    coeffs = _np(coeffs, np.uint64, (-1, 4))
    rr = _np(r, np.uint64, (4,))
    out = np.zeros(((coeffs.shape[0] + 1) // 2, 4), dtype=np.uint64)
    _chk(lib().zkp_fri_fold_fr(_ptr(coeffs), coeffs.shape[0], _ptr(rr), _ptr(out)))
    return out


def fri_merkle_tree_fr(leaves):
    """MerkleTree::new over Fr: every level, concatenated, as (zkp_fri_merkle_node_count(n), 4); the root is the last row."""
    leaves = _np(leaves, np.uint64, (-1, 4))
    out = np.zeros((fri_merkle_node_count(leaves.shape[0]), 4), dtype=np.uint64)
    _chk(lib().zkp_fri_merkle_tree_fr(_ptr(leaves), leaves.shape[0], _ptr(out)))
    return out


def fri_merkle_tree_fr_dev(leaves_tensor, n, nodes_tensor, stream=None):
    _chk(lib().zkp_fri_merkle_tree_fr_dev(_dev_ptr(leaves_tensor, 32 * n), n,
                                          _dev_ptr(nodes_tensor, 32 * fri_merkle_node_count(n)), _stream_ptr(stream)))


def fri_challenges_fr(roots, const_val, num_queries):
    roots = _np(roots, np.uint64, (-1, 4))
    cv = _np(const_val, np.uint64, (4,))
    r_out = np.zeros((roots.shape[0], 4), dtype=np.uint64)
    q_out = np.zeros(num_queries, dtype=np.uint64)
    _chk(lib().zkp_fri_challenges_fr(_ptr(roots), roots.shape[0], _ptr(cv), num_queries, _ptr(r_out), _ptr(q_out)))
    return r_out, q_out


def fri_prove_fr(coeffs, blowup_factor, num_queries):
    """generate_proof over Fr -> flat uint64 proof (layout in include/zkp_hip.h)."""
    coeffs = _np(coeffs, np.uint64, (-1, 4))
    p, words = C.c_void_p(), C.c_size_t()
    _chk(lib().zkp_fri_prove_fr(_ptr(coeffs), coeffs.shape[0], blowup_factor, num_queries, C.byref(p), C.byref(words)))
    try:
        return np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), shape=(words.value,)).copy()
    finally:
        lib().zkp_free(p)


def fri_verify_fr(proof):
    """verify over Fr: True, or raises ZkpError carrying the reference's error string."""
    proof = _np(proof, np.uint64).reshape(-1)
    _chk(lib().zkp_fri_verify_fr(_ptr(proof), proof.size))
    return True


# ----------------------------------------------------------------------------- pairings / verifiers (host code)
def g2_generator():
    out = np.zeros(24, dtype=np.uint64)
    _chk(lib().zkp_g2_generator(_ptr(out)))
    return out


def g2_mul(q_xy, scalar, q_is_inf=0):
    q = _np(q_xy, np.uint64).reshape(24)
    s = _np(scalar, np.uint64).reshape(4)
    out = np.zeros(24, dtype=np.uint64)
    inf = C.c_uint8(0)
    _chk(lib().zkp_g2_mul(_ptr(q), int(q_is_inf), _ptr(s), _ptr(out), C.byref(inf)))
    return out, int(inf.value)


def pairing(p_xy, q_xy, p_is_inf=0, q_is_inf=0):
    """Reduced optimal ate pairing as 12 x 6 Montgomery limbs (tower order)."""
    p = _np(p_xy, np.uint64).reshape(12)
    q = _np(q_xy, np.uint64).reshape(24)
    out = np.zeros((12, 6), dtype=np.uint64)
    _chk(lib().zkp_pairing(_ptr(p), int(p_is_inf), _ptr(q), int(q_is_inf), _ptr(out)))
    return out


def kzg_verify(g2s_xy, commitment, opening, y, z):
    """KzgScheme::verify (kzg/src/scheme.rs:143-160); commitment / opening = (xy, is_inf)."""
    acc = C.c_int(0)
    g2s = _np(g2s_xy, np.uint64).reshape(24)
    c, w = _np(commitment[0], np.uint64).reshape(12), _np(opening[0], np.uint64).reshape(12)
    yy, zz = _np(y, np.uint64).reshape(4), _np(z, np.uint64).reshape(4)
    _chk(lib().zkp_kzg_verify(_ptr(g2s), _ptr(c), int(commitment[1]), _ptr(w), int(opening[1]), _ptr(yy), _ptr(zz), C.byref(acc)))
    return bool(acc.value)


def kzg_verify_coset(srs, g2_sl_xy, commitment, opening, x, evals):
    """zkp_kzg_verify_coset: one coset proof of KzgOpener.open_cosets.  evals: the (l, 4) values f(x w_l^j), l a power of two;
    g2_sl_xy = [s^l]_2; commitment / opening = (xy, is_inf); srs: G1Bases with at least l points."""
    acc = C.c_int(0)
    g2 = _np(g2_sl_xy, np.uint64).reshape(24)
    c, w = _np(commitment[0], np.uint64).reshape(12), _np(opening[0], np.uint64).reshape(12)
    xx, ev = _np(x, np.uint64).reshape(4), _np(evals, np.uint64, (-1, 4))
    _chk(lib().zkp_kzg_verify_coset(srs._h, _ptr(g2), _ptr(c), int(commitment[1]), _ptr(w), int(opening[1]), _ptr(xx), _log2(ev.shape[0]),
                                    _ptr(ev), C.byref(acc)))
    return bool(acc.value)


def kzg_batch_verify(g2s_xy, commitments, points, openings, evals, r_primes):
    """KzgScheme::batch_verify (kzg/src/scheme.rs:215-245); commitments / openings: (n, 12) finite points."""
    g2s = _np(g2s_xy, np.uint64).reshape(24)
    cm, op = _np(commitments, np.uint64, (-1, 12)), _np(openings, np.uint64, (-1, 12))
    pts, ev, rp = _np(points, np.uint64, (-1, 4)), _np(evals, np.uint64, (-1, 4)), _np(r_primes, np.uint64, (-1, 4))
    acc = C.c_int(0)
    _chk(lib().zkp_kzg_batch_verify(_ptr(g2s), cm.shape[0], _ptr(cm), None, _ptr(pts), _ptr(op), None, _ptr(ev), _ptr(rp), C.byref(acc)))
    return bool(acc.value)


def kzg_aggregate_commitments(commitments, challenge, is_inf=None):
    """KzgScheme::aggregate_commitments (kzg/src/scheme.rs:187-202): sum_i challenge^i * C_i -> (affine, is_inf)."""
    cm = _np(commitments, np.uint64, (-1, 12))
    ch = _np(challenge, np.uint64).reshape(4)
    inf = _np(is_inf, np.uint8) if is_inf is not None else None
    out = np.zeros(12, dtype=np.uint64)
    oinf = C.c_uint8(0)
    _chk(lib().zkp_kzg_aggregate_commitments(_ptr(cm), _ptr(inf) if inf is not None else None, cm.shape[0], _ptr(ch), _ptr(out), C.byref(oinf)))
    return out, int(oinf.value)


class PlonkTranscript(_Handle):
    """ChallengeGenerator<Sha256> (plonk/src/challenge.rs:22-77)."""
    _destroy = "zkp_plonk_transcript_destroy"

    def __init__(self):
        self._h = C.c_void_p()
        _chk(lib().zkp_plonk_transcript_create(C.byref(self._h)))

    def feed(self, xy, is_inf=0):
        xy = _np(xy, np.uint64).reshape(12)
        _chk(lib().zkp_plonk_transcript_feed(self._h, _ptr(xy), int(is_inf)))

    def challenges(self, n):
        out = np.zeros((n, 4), dtype=np.uint64)
        _chk(lib().zkp_plonk_transcript_challenges(self._h, n, _ptr(out)))
        return out


def poly_mul_fr(a, b):
    a, b = _np(a, np.uint64, (-1, 4)), _np(b, np.uint64, (-1, 4))
    if a.shape[0] == 0 or b.shape[0] == 0:
        return np.zeros((0, 4), dtype=np.uint64)
    out = np.zeros((a.shape[0] + b.shape[0] - 1, 4), dtype=np.uint64)
    _chk(lib().zkp_poly_mul_fr(_ptr(a), a.shape[0], _ptr(b), b.shape[0], _ptr(out)))
    return out


# ----------------------------------------------------------------------------- KzgScheme mirror (kzg/src/scheme.rs)
def kzg_commit(srs, coeffs):
    coeffs = _np(coeffs, np.uint64, (-1, 4))
    out = np.zeros(12, dtype=np.uint64)
    inf = C.c_uint8(0)
    _chk(lib().zkp_kzg_commit(srs._h, _ptr(coeffs), coeffs.shape[0], _ptr(out), C.byref(inf)))
    return out, int(inf.value)


def kzg_open(srs, coeffs, z):
    coeffs, z = _np(coeffs, np.uint64, (-1, 4)), _np(z, np.uint64, (4,))
    out = np.zeros(12, dtype=np.uint64)
    ev = np.zeros(4, dtype=np.uint64)
    inf = C.c_uint8(0)
    _chk(lib().zkp_kzg_open(srs._h, _ptr(coeffs), coeffs.shape[0], _ptr(z), _ptr(out), C.byref(inf), _ptr(ev)))
    return (out, int(inf.value)), ev


# ----------------------------------------------------------------------------- transform over G1 points, all openings at once
def g1_scale_dev(xy_tensor, scalars_tensor, n, is_inf_tensor=None, stream=None):
    """zkp_g1_scale_dev: P_i <- [k_i] P_i in place over n x 12 limbs and n x 4 scalar limbs resident on the device."""
    inf = _dev_ptr(is_inf_tensor, n) if is_inf_tensor is not None else None
    _chk(lib().zkp_g1_scale_dev(_dev_ptr(xy_tensor, 96 * n), inf, _dev_ptr(scalars_tensor, 32 * n), n, _stream_ptr(stream)))


def g1_ntt_dev(xy_tensor, is_inf_tensor, log_n, inverse=False, stream=None):
    """zkp_g1_ntt_dev: Y_i = sum_j [w^(ij)] P_j in place over 2^log_n points (x 12 limbs, and as many flag bytes) on the device."""
    n = 1 << log_n
    _chk(lib().zkp_g1_ntt_dev(_dev_ptr(xy_tensor, 96 * n), _dev_ptr(is_inf_tensor, n), log_n, 1 if inverse else 0, _stream_ptr(stream)))


def g1_ntt(xy, is_inf=None, inverse=False):
    """zkp_g1_ntt on host memory: (n, 12) limbs and optional (n,) flags -> (the transformed points, their flags), n a power of two."""
    xy = _np(xy, np.uint64, (-1, 12)).copy()
    inf = _np(is_inf, np.uint8).copy() if is_inf is not None else np.zeros(xy.shape[0], dtype=np.uint8)
    _chk(lib().zkp_g1_ntt(_ptr(xy), _ptr(inf), _log2(xy.shape[0]), 1 if inverse else 0))
    return xy, inf


class KzgOpener(_Handle):
    """zkp_kzg_opener: all n = 2^log_n openings of a polynomial at the roots of unity in one call (Feist-Khovratovich); with
    log_l > 0 the n / 2^log_l multi-point proofs, one per coset of 2^log_l points (open_cosets); with max_polys > 1 those of up to
    max_polys polynomials in one call (open_cosets_batch), for which the opener owns the workspaces from creation on."""
    _destroy = "zkp_kzg_opener_destroy"

    def __init__(self, srs_bases, log_n, log_l=0, max_polys=1):
        self.log_n, self.n, self.log_l, self.max_polys = log_n, 1 << log_n, log_l, max_polys
        self.cosets = self.n >> log_l
        self._h = C.c_void_p()
        if max_polys != 1:
            _chk(lib().zkp_kzg_opener_create_cosets_batch(srs_bases._h, log_n, log_l, max_polys, C.byref(self._h)))
        elif log_l:
            _chk(lib().zkp_kzg_opener_create_cosets(srs_bases._h, log_n, log_l, C.byref(self._h)))
        else:  # (the same creation with log_l = 0; called by its own name so that the suite runs both entries)
            _chk(lib().zkp_kzg_opener_create(srs_bases._h, log_n, C.byref(self._h)))

    def open_all(self, coeffs, want_evals=True):
        """-> ((n, 12) proof points, (n,) flags), (n, 4) evaluations f(w^m) (None without want_evals); proof m is kzg_open at w^m."""
        coeffs = _np(coeffs, np.uint64, (-1, 4))
        xy = np.zeros((self.n, 12), dtype=np.uint64)
        inf = np.zeros(self.n, dtype=np.uint8)
        ev = np.zeros((self.n, 4), dtype=np.uint64) if want_evals else None
        _chk(lib().zkp_kzg_open_all(self._h, _ptr(coeffs), coeffs.shape[0], _ptr(xy), _ptr(inf), _ptr(ev)))
        return (xy, inf), ev

    def open_all_dev(self, coeffs_tensor, length, out_xy_tensor, out_inf_tensor, out_evals_tensor=None, stream=None):
        """The same with everything resident on the opener's device; nothing is synchronised."""
        ev = _dev_ptr(out_evals_tensor, 32 * self.n) if out_evals_tensor is not None else None
        _chk(lib().zkp_kzg_open_all_dev(self._h, _dev_ptr(coeffs_tensor, 32 * length), length, _dev_ptr(out_xy_tensor, 96 * self.n),
                                        _dev_ptr(out_inf_tensor, self.n), ev, _stream_ptr(stream)))

    def open_cosets(self, coeffs, evals=False):
        """-> ((r, 12) proof points, (r,) flags), (n, 4) evaluations on the whole domain (None without evals), r = n / 2^log_l: proof
        k is the commitment of the quotient of f by X^l - w^(k l); the values of coset k are evaluations[k::r]."""
        coeffs = _np(coeffs, np.uint64, (-1, 4))
        xy = np.zeros((self.cosets, 12), dtype=np.uint64)
        inf = np.zeros(self.cosets, dtype=np.uint8)
        ev = np.zeros((self.n, 4), dtype=np.uint64) if evals else None
        _chk(lib().zkp_kzg_open_cosets(self._h, _ptr(coeffs), coeffs.shape[0], _ptr(xy), _ptr(inf), _ptr(ev)))
        return (xy, inf), ev

    def open_cosets_dev(self, coeffs_tensor, length, out_xy_tensor, out_inf_tensor, out_evals_tensor=None, stream=None):
        """The same with everything resident on the opener's device; nothing is synchronised."""
        ev = _dev_ptr(out_evals_tensor, 32 * self.n) if out_evals_tensor is not None else None
        _chk(lib().zkp_kzg_open_cosets_dev(self._h, _dev_ptr(coeffs_tensor, 32 * length), length, _dev_ptr(out_xy_tensor, 96 * self.cosets),
                                           _dev_ptr(out_inf_tensor, self.cosets), ev, _stream_ptr(stream)))

    def open_cosets_batch(self, coeffs, evals=False):
        """open_cosets of P <= max_polys polynomials in one call: coeffs (P, len, 4) -> ((P, r, 12) proof points, (P, r) flags),
        (P, n, 4) evaluations (None without evals); row p is what open_cosets returns for coeffs[p]."""
        coeffs = _np(coeffs, np.uint64)
        if coeffs.ndim != 3 or coeffs.shape[2] != 4:
            raise ValueError("open_cosets_batch takes a (P, len, 4) array of coefficients")
        polys, length = coeffs.shape[0], coeffs.shape[1]
        xy = np.zeros((polys, self.cosets, 12), dtype=np.uint64)
        inf = np.zeros((polys, self.cosets), dtype=np.uint8)
        ev = np.zeros((polys, self.n, 4), dtype=np.uint64) if evals else None
        _chk(lib().zkp_kzg_open_cosets_batch(self._h, _ptr(coeffs), polys, length, length, _ptr(xy), _ptr(inf), _ptr(ev)))
        return (xy, inf), ev

    def open_cosets_batch_dev(self, coeffs_tensor, n_polys, length, stride, out_xy_tensor, out_inf_tensor, out_evals_tensor=None, stream=None):
        """The same with everything resident on the opener's device: polynomial p at `stride` scalars times p, `length` of them read;
        nothing is allocated, nothing synchronised."""
        ev = _dev_ptr(out_evals_tensor, 32 * self.n * n_polys) if out_evals_tensor is not None else None
        need = 32 * (stride * (n_polys - 1) + length) if n_polys else 0
        _chk(lib().zkp_kzg_open_cosets_batch_dev(self._h, _dev_ptr(coeffs_tensor, need), n_polys, length, stride,
                                                 _dev_ptr(out_xy_tensor, 96 * self.cosets * n_polys), _dev_ptr(out_inf_tensor, self.cosets * n_polys),
                                                 ev, _stream_ptr(stream)))


class KzgRecoverer(_Handle):
    """zkp_kzg_recoverer: the polynomial behind the cells of KzgOpener.open_cosets from any cosets that determine it; with
    max_polys > 1 those of up to max_polys polynomials that miss the same cosets in one call (recover_batch).  Made on the calling
    thread's slot; needs no SRS."""
    _destroy = "zkp_kzg_recoverer_destroy"

    def __init__(self, log_n, log_l, max_polys=1):
        self.log_n, self.n, self.log_l, self.max_polys = log_n, 1 << log_n, log_l, max_polys
        self.cosets = self.n >> log_l
        self._h = C.c_void_p()
        if max_polys != 1:
            _chk(lib().zkp_kzg_recoverer_create_batch(log_n, log_l, max_polys, C.byref(self._h)))
        else:  # (the same creation with max_polys = 1; called by its own name so that the suite runs both entries)
            _chk(lib().zkp_kzg_recoverer_create(log_n, log_l, C.byref(self._h)))

    def recover(self, evals, present, length, want_evals=False):
        """evals: (n, 4) values in natural order (coset k at k::r; what stands at a missing coset is not read); present: (r,) bytes,
        0 = missing -> ((length, 4) coefficients, (n, 4) evaluations on the whole domain or None, consistent)"""
        evals = _np(evals, np.uint64, (self.n, 4))
        present = _np(present, np.uint8, (self.cosets,))
        coeffs = np.zeros((int(length), 4), dtype=np.uint64)
        ev = np.zeros((self.n, 4), dtype=np.uint64) if want_evals else None
        ok = C.c_int(0)
        _chk(lib().zkp_kzg_recover_cosets(self._h, _ptr(evals), _ptr(present), int(length), _ptr(coeffs), _ptr(ev), C.byref(ok)))
        return coeffs, ev, bool(ok.value)

    def recover_dev(self, evals_tensor, present, length, out_coeffs_tensor, inconsistent_tensor, out_evals_tensor=None, stream=None):
        """The same with everything but `present` (host bytes) resident on the recoverer's device; inconsistent_tensor: at least 4
        bytes, its first 32-bit word becomes 0 or 1.  Nothing is synchronised."""
        present = _np(present, np.uint8, (self.cosets,))
        ev = _dev_ptr(out_evals_tensor, 32 * self.n) if out_evals_tensor is not None else None
        _chk(lib().zkp_kzg_recover_cosets_dev(self._h, _dev_ptr(evals_tensor, 32 * self.n), _ptr(present), int(length),
                                              _dev_ptr(out_coeffs_tensor, 32 * int(length)), ev, _dev_ptr(inconsistent_tensor, 4),
                                              _stream_ptr(stream)))

    def recover_batch(self, evals, present, length, want_evals=False, cells=False):
        """recover of P <= max_polys rows that miss the same cosets in one call: evals (P, n, 4) in natural order, or (P, r, l, 4)
        with cells=True (row p: r cells of l values, as KzgCellVerifier.verify takes them); present (r,) bytes for all rows ->
        ((P, length, 4) coefficients, the evaluations on the whole domain in the layout of `evals` or None, (P,) bool consistent);
        row p is what recover returns for evals[p]."""
        evals = _np(evals, np.uint64)
        shape = (self.cosets, self.n // self.cosets, 4) if cells else (self.n, 4)
        if evals.ndim != len(shape) + 1 or evals.shape[1:] != shape:
            raise ValueError("recover_batch takes a (P, n, 4) array of evaluations, or (P, r, l, 4) with cells=True")
        polys = evals.shape[0]
        present = _np(present, np.uint8, (self.cosets,))
        coeffs = np.zeros((polys, int(length), 4), dtype=np.uint64)
        ev = np.zeros((polys,) + shape, dtype=np.uint64) if want_evals else None
        ok = np.zeros(polys, dtype=np.uint8)
        _chk(lib().zkp_kzg_recover_cosets_batch(self._h, _ptr(evals), polys, _ptr(present), int(length), 1 if cells else 0, _ptr(coeffs),
                                                _ptr(ev), _ptr(ok)))
        return coeffs, ev, ok.astype(bool)

    def recover_batch_dev(self, evals_tensor, n_polys, present, length, stride, out_coeffs_tensor, inconsistent_tensor, out_evals_tensor=None,
                          cells=False, stream=None):
        """The same with everything but `present` (host bytes) resident on the recoverer's device: row p of the coefficients at
        `stride` scalars times p, `length` of them written; inconsistent_tensor: n_polys 32-bit words, each becomes 0 or 1.  `cells`
        may be a bool or a ZKP_KZG_LAYOUT_* number.  Nothing is allocated, nothing synchronised."""
        present = _np(present, np.uint8, (self.cosets,))
        ev = _dev_ptr(out_evals_tensor, 32 * self.n * n_polys) if out_evals_tensor is not None else None
        need = 32 * (int(stride) * (n_polys - 1) + int(length)) if n_polys else 0
        _chk(lib().zkp_kzg_recover_cosets_batch_dev(self._h, _dev_ptr(evals_tensor, 32 * self.n * n_polys), n_polys, _ptr(present), int(length),
                                                    int(stride), int(cells), _dev_ptr(out_coeffs_tensor, need), ev,
                                                    _dev_ptr(inconsistent_tensor, 4 * n_polys), _stream_ptr(stream)))


ZKP_KZG_ORDER_NATURAL, ZKP_KZG_ORDER_BITREV = 0, 1  # the orders of a row of evaluations (zkp_hip.kzg_evals.KzgEvalOpener)


def _points(p):
    """(xy, is_inf) or xy alone -> ((count, 12) limbs, (count,) flags or None)"""
    xy, inf = p if isinstance(p, tuple) else (p, None)
    xy = _np(xy, np.uint64, (-1, 12))
    return xy, (_np(inf, np.uint8, (xy.shape[0],)) if inf is not None else None)


class KzgCellVerifier(_Handle):
    """zkp_kzg_cell_verifier: any number of cells of KzgOpener.open_cosets, of any number of commitments, behind one pairing check.
    srs_bases is borrowed (kept alive here); g2_sl_xy = [s^l]_2.  The weights are the caller's randomness: see include/zkp_hip.h."""
    _destroy = "zkp_kzg_cell_verifier_destroy"

    def __init__(self, srs_bases, g2_sl_xy, log_n, log_l, max_cells, max_commits):
        self.log_n, self.n, self.log_l, self.l = log_n, 1 << log_n, log_l, 1 << log_l
        self.max_cells, self.max_commits = int(max_cells), int(max_commits)
        self._srs = srs_bases
        self._h = C.c_void_p()
        g2 = _np(g2_sl_xy, np.uint64).reshape(24)
        _chk(lib().zkp_kzg_cell_verifier_create(srs_bases._h, _ptr(g2), log_n, log_l, self.max_cells, self.max_commits, C.byref(self._h)))

    @staticmethod
    def _indices(commit_index, coset_index):
        ci, ki = _np(commit_index, np.uint32), _np(coset_index, np.uint32)
        if ci.shape != ki.shape or ci.ndim != 1:
            raise ZkpError(ZKP_E_ARG, "commit_index and coset_index are two vectors of one length")
        return ci, ki

    def verify(self, commitments, commit_index, coset_index, evals, proofs, weights):
        """commitments / proofs: (xy, is_inf) or xy alone; evals (n_cells, l, 4); weights (n_cells, 4) -> accepted"""
        ci, ki = self._indices(commit_index, coset_index)
        cells = ci.shape[0]
        (cxy, cinf), (pxy, pinf) = _points(commitments), _points(proofs)
        ev, wt = _np(evals, np.uint64, (cells, self.l, 4)), _np(weights, np.uint64, (cells, 4))
        if pxy.shape[0] != cells:
            raise ZkpError(ZKP_E_ARG, "one proof per cell")
        acc = C.c_int(0)
        _chk(lib().zkp_kzg_verify_cells(self._h, _ptr(cxy), _ptr(cinf), cxy.shape[0], cells, _ptr(ci), _ptr(ki), _ptr(ev), _ptr(pxy), _ptr(pinf),
                                        _ptr(wt), C.byref(acc)))
        return bool(acc.value)

    def verify_dev(self, commits_tensor, n_commits, commit_index, coset_index, evals_tensor, proofs_tensor, weights_tensor,
                   commits_inf_tensor=None, proofs_inf_tensor=None, stream=None):
        """The same with everything but the two index vectors (host) resident on the verifier's device; blocks like verify."""
        ci, ki = self._indices(commit_index, coset_index)
        cells = ci.shape[0]
        cinf = _dev_ptr(commits_inf_tensor, n_commits) if commits_inf_tensor is not None else None
        pinf = _dev_ptr(proofs_inf_tensor, cells) if proofs_inf_tensor is not None else None
        acc = C.c_int(0)
        _chk(lib().zkp_kzg_verify_cells_dev(self._h, _dev_ptr(commits_tensor, 96 * n_commits), cinf, n_commits, cells, _ptr(ci), _ptr(ki),
                                            _dev_ptr(evals_tensor, 32 * cells * self.l), _dev_ptr(proofs_tensor, 96 * cells), pinf,
                                            _dev_ptr(weights_tensor, 32 * cells), _stream_ptr(stream), C.byref(acc)))
        return bool(acc.value)

    def verify_bytes(self, commitments48, commit_index, coset_index, cell_bytes, proofs48, weights, big_endian=True):
        """The wire form: commitments48 (n_commits x 48) and proofs48 (n_cells x 48) compressed points, cell_bytes n_cells x l x 32 bytes
        of canonical scalars (big-endian unless told otherwise), weights (n_cells, 4) limbs as in verify -> accepted.  Everything is
        decoded on the device; the points without the subgroup test, which zkp_kzg_verify_cells_dev runs on every point anyway.  A point
        or scalar that does not decode raises ZkpError(ZKP_E_ARG) naming the array, the index and the status word.  Cells in the library's
        own order (EIP-7594's bit-reversed numbering is not built)."""
        import torch
        ci, ki = self._indices(commit_index, coset_index)
        cells = ci.shape[0]
        cb, pb = _bytes48(commitments48), _bytes48(proofs48)
        sb = _np(np.frombuffer(cell_bytes, dtype=np.uint8).copy() if isinstance(cell_bytes, (bytes, bytearray, memoryview)) else cell_bytes, np.uint8,
                 (cells * self.l, 32))
        if pb.shape[0] != cells:
            raise ZkpError(ZKP_E_ARG, "one proof per cell")
        if cells == 0:
            return True
        pts = []
        for name, b in (("commitments", cb), ("proofs", pb)):
            n = b.shape[0]
            xy = torch.empty(max(n, 1) * 12, dtype=torch.int64, device="cuda")
            inf = torch.empty(max(n, 1), dtype=torch.uint8, device="cuda")
            rep = g1_decompress_dev(torch.from_numpy(b).cuda(), n, xy, inf, check_subgroup=False) if n else {"bad": 0}
            if rep["bad"]:
                raise ZkpError(ZKP_E_ARG, f"{name}[{rep['first_bad']}] does not decode ({_G1_STATUS_WORD[rep['first_status']]})")
            pts.append((xy, inf, n))
        ev = torch.empty(cells * self.l * 4, dtype=torch.int64, device="cuda")
        bad, first = fr_from_bytes_dev(torch.from_numpy(sb).cuda(), cells * self.l, ev, big_endian=big_endian)
        if bad:
            raise ZkpError(ZKP_E_ARG, f"cell_bytes[{first}] does not decode (canonical): cell {first // self.l}, value {first % self.l}")
        wt = torch.from_numpy(_np(weights, np.uint64, (cells, 4)).view(np.int64)).cuda()
        (cxy, cinf, n_commits), (pxy, pinf, _) = pts
        return self.verify_dev(cxy, n_commits, ci, ki, ev, pxy, wt, commits_inf_tensor=cinf, proofs_inf_tensor=pinf)

    def aggregate_dev(self, n_commits, commit_index, coset_index, evals_tensor, weights_tensor, out_interp_tensor, out_commit_weights_tensor,
                      out_proof_scalars_tensor, stream=None):
        """zkp_kzg_cells_aggregate_dev: the field half alone -> the l coefficients of sum rho_i I_i, the n_commits sums of the weights,
        the n_cells scalars rho_i c_i, in the three tensors.  Nothing is synchronised."""
        ci, ki = self._indices(commit_index, coset_index)
        cells = ci.shape[0]
        _chk(lib().zkp_kzg_cells_aggregate_dev(self._h, n_commits, cells, _ptr(ci), _ptr(ki), _dev_ptr(evals_tensor, 32 * cells * self.l),
                                               _dev_ptr(weights_tensor, 32 * cells), _dev_ptr(out_interp_tensor, 32 * self.l),
                                               _dev_ptr(out_commit_weights_tensor, 32 * n_commits),
                                               _dev_ptr(out_proof_scalars_tensor, 32 * cells), _stream_ptr(stream)))


class Srs:
    """kzg/src/srs.rs: g1_points = [s^i]G for i < circuit_size + 3, generated on the GPU and kept resident."""

    def __init__(self, g1_points_xy):
        self.g1_points_xy = _np(g1_points_xy, np.uint64, (-1, 12))
        self.bases = G1Bases.from_host(self.g1_points_xy)

    @classmethod
    def new_from_secret(cls, secret, circuit_size):  # srs.rs:48
        return cls(srs_g1(secret, circuit_size + 3))

    def g1_points(self):  # srs.rs:78 (the reference clones; here a view)
        return self.g1_points_xy


class KzgScheme:
    """Python face of csrc/kzg_host.hpp (same surface as kzg/src/scheme.rs:22-142)."""

    def __init__(self, srs, expand_bases=True):  # scheme.rs:34
        self.srs = srs
        self._openers = {}  # log_n -> KzgOpener (open_all), released by close()
        self._coset_openers = {}  # (log_n, log_l) -> KzgOpener (open_cosets), released by close()
        self._recoverers = {}  # (log_n, log_l) -> KzgRecoverer (recover_cosets), released by close()
        self._cell_verifiers = {}  # (log_n, log_l) -> (g2_sl bytes, KzgCellVerifier) (verify_cells), released by close()
        self._lagrange = {}  # log_n -> G1Bases (the Lagrange basis of the first 2^log_n points), released by close()
        self._eval_openers = {}  # (log_n, bitrev) -> KzgEvalOpener (commit_evals_batch, open_evals_batch), released by close()
        if expand_bases:  # the SRS is fixed for the life of the scheme: pay the one-off expansion here
            srs.bases.precompute(0)

    def commit(self, coeffs):  # scheme.rs:49 / 63
        return kzg_commit(self.srs.bases, coeffs)

    commit_vector = commit

    def commit_para(self, para):  # scheme.rs:78
        return g1_mul(self.srs.g1_points_xy[0], 0, para)

    def open(self, coeffs, z):  # scheme.rs:108 / 132
        return kzg_open(self.srs.bases, coeffs, z)

    open_vector = open

    def open_all(self, coeffs, log_n):
        """Every opening of `coeffs` on the domain of 2^log_n roots of unity: KzgOpener.open_all (the opener is kept per log_n)."""
        if log_n not in self._openers:
            self._openers[log_n] = KzgOpener(self.srs.bases, log_n)
        return self._openers[log_n].open_all(coeffs)

    def open_cosets(self, coeffs, log_n, log_l, evals=False):
        """One proof per coset of 2^log_l points of the domain of 2^log_n roots of unity: KzgOpener.open_cosets (the opener is kept
        per shape)."""
        if (log_n, log_l) not in self._coset_openers:
            self._coset_openers[log_n, log_l] = KzgOpener(self.srs.bases, log_n, log_l)
        return self._coset_openers[log_n, log_l].open_cosets(coeffs, evals=evals)

    def open_cosets_batch(self, polys, log_n, log_l, evals=False):
        """open_cosets of every polynomial of `polys` ((P, len, 4)) in one call: KzgOpener.open_cosets_batch (the opener is kept per
        shape and replaced by a larger one when a batch outgrows it; open_cosets of that shape uses it too)."""
        polys = _np(polys, np.uint64)
        kept = self._coset_openers.get((log_n, log_l))
        if kept is None or kept.max_polys < polys.shape[0]:
            if kept is not None:
                kept.close()
            self._coset_openers[log_n, log_l] = KzgOpener(self.srs.bases, log_n, log_l, max(polys.shape[0], 1))
        return self._coset_openers[log_n, log_l].open_cosets_batch(polys, evals=evals)

    def recover_cosets(self, evals, present, length, log_n, log_l, proofs=False):
        """The polynomial of `length` coefficients behind the present cosets of `evals`: KzgRecoverer.recover with the evaluations (the
        recoverer is kept per shape) -> (coefficients, evaluations on the whole domain, consistent), and with proofs=True a fourth
        item, the (points, flags) of open_cosets on the recovered coefficients."""
        if (log_n, log_l) not in self._recoverers:
            self._recoverers[log_n, log_l] = KzgRecoverer(log_n, log_l)
        coeffs, ev, ok = self._recoverers[log_n, log_l].recover(evals, present, length, want_evals=True)
        if not proofs:
            return coeffs, ev, ok
        return coeffs, ev, ok, self.open_cosets(coeffs, log_n, log_l)[0]

    def recover_cosets_batch(self, evals, present, length, log_n, log_l, proofs=False, cells=False):
        """recover_cosets of every row of `evals` ((P, n, 4), or (P, r, l, 4) with cells=True), all missing the cosets of `present`,
        in one call: KzgRecoverer.recover_batch with the evaluations (the recoverer is kept per shape and replaced by a larger one
        when a batch outgrows it; recover_cosets of that shape uses it too) -> (coefficients, evaluations, (P,) consistent), and
        with proofs=True a fourth item, the (points, flags) of open_cosets_batch on the recovered rows."""
        evals = _np(evals, np.uint64)
        kept = self._recoverers.get((log_n, log_l))
        if kept is None or kept.max_polys < evals.shape[0]:
            if kept is not None:
                kept.close()
            self._recoverers[log_n, log_l] = KzgRecoverer(log_n, log_l, max(evals.shape[0], 1))
        coeffs, ev, ok = self._recoverers[log_n, log_l].recover_batch(evals, present, length, want_evals=True, cells=cells)
        if not proofs:
            return coeffs, ev, ok
        return coeffs, ev, ok, self.open_cosets_batch(coeffs, log_n, log_l)[0]

    def verify_cells(self, g2_sl_xy, commitments, commit_index, coset_index, evals, proofs, log_n, log_l, weights=None):
        """Cells of open_cosets, of any of `commitments`, in one pairing check: KzgCellVerifier.verify (the verifier is kept per
        shape and grows with the batch).  weights=None draws a 128-bit weight per cell from `secrets`, the counterpart of
        Fr::from(rng.gen::<u128>()) in kzg/src/scheme.rs:215-245; pass weights only to reproduce a run."""
        ci = _np(commit_index, np.uint32)
        cells, commits = ci.shape[0], _points(commitments)[0].shape[0]
        g2 = _np(g2_sl_xy, np.uint64).reshape(24)
        kept = self._cell_verifiers.get((log_n, log_l))
        if kept is None or kept[0] != g2.tobytes() or kept[1].max_cells < cells or kept[1].max_commits < commits:
            if kept is not None:
                kept[1].close()
            ver = KzgCellVerifier(self.srs.bases, g2, log_n, log_l, max(cells, 1), max(commits, 1))
            kept = self._cell_verifiers[log_n, log_l] = (g2.tobytes(), ver)
        if weights is None:
            import secrets
            weights = _fr_mont_rows([secrets.randbits(128) for _ in range(cells)])
        return kept[1].verify(commitments, ci, coset_index, evals, proofs, weights)

    def verify_points(self, g2s_xy, commitments, zs, ys, proofs, commit_index=None, weights=None):
        """Point openings (open, open_all, open_evals_batch) of any of `commitments` in one pairing check: KzgPointVerifier.verify
        (one verifier is kept and grows with the batch).  commit_index None: opening i belongs to commitment i, the shape of
        kzg_batch_verify.  weights=None draws a 128-bit weight per opening from `secrets`, the counterpart of
        Fr::from(rng.gen::<u128>()) in kzg/src/scheme.rs:215-245; pass weights only to reproduce a run."""
        count, commits = _points(proofs)[0].shape[0], _points(commitments)[0].shape[0]
        g2 = _np(g2s_xy, np.uint64).reshape(24)
        kept = getattr(self, "_point_verifier", None)
        if kept is None or kept[0] != g2.tobytes() or kept[1].max_openings < count or kept[1].max_commits < commits:
            room = (max(count, 1), max(commits, 1))
            if kept is not None:  # (grows in either capacity, shrinks in neither)
                room = (max(room[0], kept[1].max_openings), max(room[1], kept[1].max_commits))
                kept[1].close()
            from .kzg_points import KzgPointVerifier  # (that module imports this one)
            kept = self._point_verifier = (g2.tobytes(), KzgPointVerifier(g2, *room))
        if weights is None:
            import secrets
            weights = _fr_mont_rows([secrets.randbits(128) for _ in range(count)])
        return kept[1].verify(commitments, zs, ys, proofs, weights, commit_index=commit_index)

    def verify_points_each(self, g2s_xy, commitments, zs, ys, proofs, commit_index=None):
        """A verdict per opening (KzgPointVerifier.verify_each over the verifier verify_points keeps): -> (ok (n_openings,) uint8,
        n_bad).  ok[i] = 1 iff opening i alone verifies; no weights, every opening gets its own pairing check on the device."""
        count, commits = _points(proofs)[0].shape[0], _points(commitments)[0].shape[0]
        g2 = _np(g2s_xy, np.uint64).reshape(24)
        kept = getattr(self, "_point_verifier", None)
        if kept is None or kept[0] != g2.tobytes() or kept[1].max_openings < count or kept[1].max_commits < commits:
            room = (max(count, 1), max(commits, 1))
            if kept is not None:
                room = (max(room[0], kept[1].max_openings), max(room[1], kept[1].max_commits))
                kept[1].close()
            from .kzg_points import KzgPointVerifier
            kept = self._point_verifier = (g2.tobytes(), KzgPointVerifier(g2, *room))
        return kept[1].verify_each(commitments, zs, ys, proofs, commit_index=commit_index)

    def _eval_opener(self, log_n, bitrev, polys):
        """The opener kept per (log_n, bitrev), replaced by a larger one when a batch outgrows it; the Lagrange basis is kept per log_n"""
        from .kzg_evals import KzgEvalOpener  # (that module imports this one)
        if log_n not in self._lagrange:
            self._lagrange[log_n] = self.srs.bases.lagrange(log_n)
        kept = self._eval_openers.get((log_n, bool(bitrev)))
        if kept is None or kept.max_polys < polys:
            if kept is not None:
                kept.close()
            self._eval_openers[log_n, bool(bitrev)] = KzgEvalOpener(self._lagrange[log_n], log_n, max(polys, 1), bitrev=bitrev)
        return self._eval_openers[log_n, bool(bitrev)]

    def commit_evals_batch(self, evals, log_n, bitrev=False):
        """The commitments of the polynomials whose values on the domain of 2^log_n roots of unity are the rows of `evals`
        ((P, n, 4); bitrev: position i holds the value at w^bitrev(i)): KzgEvalOpener.commit_batch -> ((P, 12), (P,) flags)"""
        evals = _np(evals, np.uint64)
        return self._eval_opener(log_n, bitrev, evals.shape[0]).commit_batch(evals)

    def open_evals_batch(self, evals, zs, log_n, bitrev=False):
        """The openings of those polynomials, row p at zs[p] ((P, 4)), with no transform: KzgEvalOpener.open_batch ->
        (((P, 12) proofs, (P,) flags), (P, 4) values); row p is what open returns for the coefficients of row p's interpolant."""
        evals = _np(evals, np.uint64)
        return self._eval_opener(log_n, bitrev, evals.shape[0]).open_batch(evals, zs)

    def close(self):
        """Release the device memory of the openers open_all and open_cosets made (about 1.4 KB per point of a domain for open_all, about
        1.1 KB for open_cosets: 512 B of kept slices, 512 B of partial sums and 64 B of scalars, plus up to 64 MiB); the SRS stays."""
        for op in (list(self._openers.values()) + list(self._coset_openers.values()) + list(self._recoverers.values()) +
                   [ver for _, ver in self._cell_verifiers.values()]):
            op.close()
        for op in list(self._eval_openers.values()) + list(self._lagrange.values()):  # (the openers borrow the bases: they go first)
            op.close()
        kept, self._point_verifier = getattr(self, "_point_verifier", None), None  # (verify_points)
        if kept is not None:
            kept[1].close()
        self._eval_openers = {}
        self._lagrange = {}
        self._cell_verifiers = {}
        self._openers = {}
        self._coset_openers = {}
        self._recoverers = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ----------------------------------------------------------------------------- PLONK prover rounds (plonk/src/prover.rs)
CIRCUIT_POLYS = ("q_m", "q_l", "q_r", "q_o", "q_c", "pi", "f_a", "f_b", "f_c", "s_sigma_1", "s_sigma_2", "s_sigma_3")
POLY_IDS = {"ax": 0, "bx": 1, "cx": 2, "z": 3, "r": 4, "w_zeta": 5, "w_zeta_omega": 6, "tx_compact": 7, "t": 8}


class _PlonkProof(C.Structure):  # zkp_plonk_proof in include/zkp_hip.h
    _fields_ = [("commit_xy", (C.c_uint64 * 12) * 9), ("commit_is_inf", C.c_uint8 * 9), ("bars", (C.c_uint64 * 4) * 6),
                ("u", C.c_uint64 * 4), ("degree", C.c_uint64)]


class _PlonkGates(C.Structure):  # zkp_plonk_gates in include/zkp_hip.h
    _fields_ = [("gates", C.c_size_t), ("pos", C.c_void_p), ("sel", C.c_void_p), ("vals", C.c_void_p)]


_FR_MOD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def _fr_mont_rows(values):
    """ints -> (len, 4) uint64 Montgomery limbs (the memory form of the ABI); a circuit repeats few selector values, so each distinct
    value is converted once."""
    seen = {}
    out = np.empty((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        row = seen.get(v)
        if row is None:
            m = (v % _FR_MOD << 256) % _FR_MOD
            row = seen[v] = [(m >> (64 * k)) & 0xFFFFFFFFFFFFFFFF for k in range(4)]
        out[i] = row
    return out


class PlonkCircuit:
    """Circuit of plonk/src/circuit.rs: gates over (wire column, row, value) triples, with the selector rules of gate.rs:38-94
    (the stored pi is negated; a constant gate has q_l = 1 and q_c = -constant).  Holds plain integers; gate_table() packs them
    for zkp_plonk_prover_create_from_gates, compile() replaces Circuit::compile."""

    def __init__(self):
        self.pos = []   # per gate: a_col a_row b_col b_row c_col c_row
        self.sel = []   # per gate: q_m q_l q_r q_o q_c pi (as stored)
        self.vals = []  # per gate: a b c

    def __len__(self):
        return len(self.pos)

    def _add(self, a, b, c, q_m, q_l, q_r, q_o, q_c, pi):
        self.pos.append((a[0], a[1], b[0], b[1], c[0], c[1]))
        self.sel.append((q_m, q_l, q_r, q_o, q_c % _FR_MOD, (-pi) % _FR_MOD))
        self.vals.append((a[2] % _FR_MOD, b[2] % _FR_MOD, c[2] % _FR_MOD))

    def add_addition_gate(self, a, b, c, pi=0):        # gate.rs:38-55
        self._add(a, b, c, 0, 1, 1, _FR_MOD - 1, 0, pi)

    def add_multiplication_gate(self, a, b, c, pi=0):  # gate.rs:57-74
        self._add(a, b, c, 1, 0, 0, _FR_MOD - 1, 0, pi)

    def add_constant_gate(self, a, b, c, pi=0, constant=None):
        """gate.rs:76-94; Circuit::add_constant_gate takes the constant from a's value (circuit.rs:73-79), Gate::new_constant_gate
        any constant."""
        self._add(a, b, c, 0, 1, 0, 0, -(a[2] if constant is None else constant), pi)

    def gate_table(self):
        """-> pos (g, 6) uint32, sel (g, 6, 4) uint64, vals (g, 3, 4) uint64: the arrays of zkp_plonk_gates."""
        g = len(self.pos)
        pos = np.array(self.pos, dtype=np.uint32).reshape(g, 6)
        sel = _fr_mont_rows([v for row in self.sel for v in row]).reshape(g, 6, 4)
        vals = _fr_mont_rows([v for row in self.vals for v in row]).reshape(g, 3, 4)
        return pos, sel, vals

    def compile(self, srs_bases):
        """Circuit::compile (circuit.rs:166-245) on the device -> PlonkProver."""
        return PlonkProver.from_gates(srs_bases, *self.gate_table())


class PlonkProver(_Handle):
    """Round-by-round face of generate_proof (plonk/src/prover.rs:61-293); blinders and challenges are inputs."""
    _destroy = "zkp_plonk_prover_destroy"

    def __init__(self, srs_bases, log_n, circuit_polys, k1, k2):
        """circuit_polys: dict name -> (len,4) uint64 coefficient array (names in CIRCUIT_POLYS)."""
        arrs = [_np(circuit_polys[k], np.uint64, (-1, 4)) for k in CIRCUIT_POLYS]
        ptrs = (C.c_void_p * 12)(*[a.ctypes.data for a in arrs])
        lens = (C.c_size_t * 12)(*[a.shape[0] for a in arrs])
        k1, k2 = _np(k1, np.uint64, (4,)), _np(k2, np.uint64, (4,))
        self._bases = srs_bases  # keep alive
        self._h = C.c_void_p()
        self.n = 1 << log_n
        _chk(lib().zkp_plonk_prover_create(srs_bases._h, log_n, ptrs, lens, _ptr(k1), _ptr(k2), C.byref(self._h)))

    @classmethod
    def from_gates(cls, srs_bases, pos, sel, vals):
        """zkp_plonk_prover_create_from_gates: pos (g, 6) uint32, sel (g, 6, 4), vals (g, 3, 4) uint64 (PlonkCircuit.gate_table())."""
        pos = _np(pos, np.uint32, (-1, 6))
        g = pos.shape[0]
        sel, vals = _np(sel, np.uint64, (g, 6, 4)), _np(vals, np.uint64, (g, 3, 4))
        gt = _PlonkGates(g, pos.ctypes.data, sel.ctypes.data, vals.ctypes.data)
        self = cls.__new__(cls)
        self._bases = srs_bases  # keep alive
        self._h = C.c_void_p()
        _chk(lib().zkp_plonk_prover_create_from_gates(srs_bases._h, C.byref(gt), C.byref(self._h)))
        self.gates = g
        self.n = 1 << self.info()[0]
        return self

    def set_witness(self, vals, pi=None):
        """Another witness for the circuit of from_gates: vals (g, 3, 4) uint64, pi (g, 4) as stored (None: unchanged)."""
        vals = _np(vals, np.uint64, (-1, 3, 4))
        pi = _np(pi, np.uint64, (vals.shape[0], 4)) if pi is not None else None
        _chk(lib().zkp_plonk_prover_set_witness(self._h, _ptr(vals), _ptr(pi), vals.shape[0]))

    def set_witness_dev(self, vals, gates, pi=None, stream=None):
        """set_witness from torch CUDA tensors of 12 * gates (and 4 * gates) 64-bit words, read on `stream` (None: torch's current)."""
        _chk(lib().zkp_plonk_prover_set_witness_dev(self._h, _dev_ptr(vals, 96 * gates), _dev_ptr(pi, 32 * gates) if pi is not None else None,
                                                    gates, _stream_ptr(stream)))

    def circuit_poly(self, name):
        """The n coefficients (zero-padded) of one of CIRCUIT_POLYS as the prover holds it."""
        out = np.zeros((self.n, 4), dtype=np.uint64)
        ln = C.c_size_t(0)
        _chk(lib().zkp_plonk_get_circuit_poly(self._h, CIRCUIT_POLYS.index(name), _ptr(out), self.n, C.byref(ln)))
        return out

    def info(self):
        """-> (log_n, k1, k2)."""
        log_n, k1, k2 = C.c_uint(0), np.zeros(4, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        _chk(lib().zkp_plonk_prover_info(self._h, C.byref(log_n), _ptr(k1), _ptr(k2)))
        return int(log_n.value), k1, k2

    def prove(self, blinders):
        """generate_proof (plonk/src/prover.rs:61-293) with the reference's transcript; blinders = b1..b9 (9, 4)."""
        b = _np(blinders, np.uint64, (9, 4))
        out = _PlonkProof()
        _chk(lib().zkp_plonk_prove(self._h, _ptr(b), C.byref(out)))
        names = ("a", "b", "c", "z", "t_lo", "t_mid", "t_hi", "w_ev_x", "w_ev_wx")
        commits = {k: (np.array(out.commit_xy[i][:], dtype=np.uint64), int(out.commit_is_inf[i])) for i, k in enumerate(names)}
        bars = np.array([list(out.bars[i]) for i in range(6)], dtype=np.uint64)
        return {"commits": commits, "bars": bars, "u": np.array(out.u[:], dtype=np.uint64), "degree": int(out.degree)}

    def verify(self, g2s_xy, proof):
        """verify (plonk/src/verifier.rs:19-157) of a dict returned by prove(): 1 accepted, 0 pairing failed, -1 challenge mismatch."""
        out = _PlonkProof()
        names = ("a", "b", "c", "z", "t_lo", "t_mid", "t_hi", "w_ev_x", "w_ev_wx")
        for i, k in enumerate(names):
            xy, inf = proof["commits"][k]
            for q in range(12):
                out.commit_xy[i][q] = int(xy[q])
            out.commit_is_inf[i] = int(inf)
        for i in range(6):
            for q in range(4):
                out.bars[i][q] = int(proof["bars"][i][q])
        for q in range(4):
            out.u[q] = int(proof["u"][q])
        out.degree = int(proof["degree"])
        g2s = _np(g2s_xy, np.uint64).reshape(24)
        acc = C.c_int(0)
        _chk(lib().zkp_plonk_verify(self._h, _ptr(g2s), C.byref(out), C.byref(acc)))
        return int(acc.value)

    @staticmethod
    def _pts(xy, inf):
        return [(xy[i].copy(), int(inf[i])) for i in range(xy.shape[0])]

    def round1(self, blinders):  # b1..b6
        b = _np(blinders, np.uint64, (6, 4))
        xy, inf = np.zeros((3, 12), dtype=np.uint64), np.zeros(3, dtype=np.uint8)
        _chk(lib().zkp_plonk_round1(self._h, _ptr(b), _ptr(xy), _ptr(inf)))
        return self._pts(xy, inf)

    def round2(self, beta, gamma, blinders):  # b7..b9
        b = _np(blinders, np.uint64, (3, 4))
        beta, gamma = _np(beta, np.uint64, (4,)), _np(gamma, np.uint64, (4,))
        xy, inf = np.zeros((1, 12), dtype=np.uint64), np.zeros(1, dtype=np.uint8)
        _chk(lib().zkp_plonk_round2(self._h, _ptr(beta), _ptr(gamma), _ptr(b), _ptr(xy), _ptr(inf)))
        return self._pts(xy, inf)[0]

    def round3(self, alpha):
        alpha = _np(alpha, np.uint64, (4,))
        xy, inf = np.zeros((3, 12), dtype=np.uint64), np.zeros(3, dtype=np.uint8)
        deg = C.c_size_t(0)
        _chk(lib().zkp_plonk_round3(self._h, _ptr(alpha), _ptr(xy), _ptr(inf), C.byref(deg)))
        return self._pts(xy, inf), int(deg.value)

    def round4(self, zeta):
        zeta = _np(zeta, np.uint64, (4,))
        bars = np.zeros((6, 4), dtype=np.uint64)
        _chk(lib().zkp_plonk_round4(self._h, _ptr(zeta), _ptr(bars)))
        return bars

    def round5(self, v):
        v = _np(v, np.uint64, (4,))
        xy, inf = np.zeros((2, 12), dtype=np.uint64), np.zeros(2, dtype=np.uint8)
        _chk(lib().zkp_plonk_round5(self._h, _ptr(v), _ptr(xy), _ptr(inf)))
        return self._pts(xy, inf)

    def get_poly(self, name):
        ln = C.c_size_t(0)
        _chk(lib().zkp_plonk_get_poly(self._h, POLY_IDS[name], None, 0, C.byref(ln)))
        out = np.zeros((ln.value, 4), dtype=np.uint64)
        if ln.value:
            _chk(lib().zkp_plonk_get_poly(self._h, POLY_IDS[name], _ptr(out), ln.value, C.byref(ln)))
        return out


# ----------------------------------------------------------------------------- Nova folding (nova/src), zkp_hip/nova.py
from .nova import (FInstance, FWitness, NifsProof, NovaR1CS, NovaTranscript, csr_from_dense, is_r1cs_satisfied,  # noqa: E402,F401
                   nifs_prove, nifs_prover, nifs_verify)
