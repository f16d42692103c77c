"""c_lwe_snarks_amd -- thin ctypes binding over libmfhip.so (the C ABI in include/mfhip.h).

The product is the HIP library and its C ABI; this module only exists so that pytest, bench.py and
__graft_entry__.py can drive that ABI with torch-owned device memory.  There is no CPU fallback: if the
shared library is missing, or no HIP device is usable, construction fails loudly.

(The directory is named ``c-lwe-snarks_amd``; ``c_lwe_snarks_amd.py`` at the repo root loads it under an
importable name.)
"""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MFHIP_LIB") or os.path.join(_HERE, "libmfhip.so")  # ($MFHIP_LIB: another build of the same ABI, for same-box A/B runs of the tools)
P = 0xFFFFFFFB  # GAMMA_P, reference src/lwe.h:25


class MfhError(RuntimeError):
    pass


@dataclass(frozen=True)
class Params:
    """GAMMA_* of reference src/lwe.h:14-31 as runtime values."""

    n: int = 1470
    logq: int = 736
    d: int = 1 << 15
    m: int = 21845

    @property
    def L(self):  # limbs per value
        return (self.logq + 63) // 64

    @property
    def K(self):  # limbs surviving modq
        return self.logq // 64

    @property
    def lanes(self):  # uint64 lanes of 56 bits per value in the multi-GPU sums (mfh_lanes_per_value)
        return (64 * self.K + 55) // 56

    @property
    def ctb(self):  # CT_BYTES
        return self.logq // 8

    @property
    def ctr_ct(self):  # CTR_CT, src/snark.h:8
        return self.ctb * self.n

    @property
    def ctr_s(self):
        return 0

    @property
    def ctr_as(self):
        return self.ctr_ct * self.d

    @property
    def ctr_bt(self):
        return 2 * self.ctr_ct * self.d

    @property
    def ctr_bv(self):
        return 2 * self.ctr_ct * self.d + self.ctr_ct

    @property
    def ct_limbs(self):
        return (self.n + 1) * self.L


DEBUG = Params(d=256, m=64)  # the reference's !NDEBUG parameters (src/lwe.h:18-21)
DEFAULT = Params()  # NDEBUG parameters (src/lwe.h:14-17)


class _CParams(ctypes.Structure):
    _fields_ = [("n", ctypes.c_uint32), ("logq", ctypes.c_uint32), ("d", ctypes.c_uint32), ("m", ctypes.c_uint32)]


_lib = None

EXPORTS = [
    "mfh_ctx_create", "mfh_ctx_destroy", "mfh_set_stream", "mfh_sync", "mfh_scrub_staging", "mfh_last_error", "mfh_set_seed",
    "mfh_keystream", "mfh_sample_rows", "mfh_ct_add", "mfh_ct_mul_ui", "mfh_ct_addmul_ui", "mfh_eval_rows",
    "mfh_encrypt_rows", "mfh_decrypt", "mfh_ct_smudge", "mfh_ssp_upload", "mfh_witness_poly", "mfh_version",
    "mfh_workspace_bytes", "mfh_last_kernel_ms", "mfh_set_timing", "mfh_set_overlap", "mfh_eval_rows_multi", "mfh_prove_batch", "mfh_crs_mm_image_bytes", "mfh_crs_expand_mm", "mfh_crs_set_resident_mm", "mfh_witness_poly_multi", "mfh_witness_poly_mm", "mfh_poly_h_multi", "mfh_poly_mul", "mfh_poly_add", "mfh_poly_prepare_t",
    "mfh_ssp_prepare", "mfh_poly_h", "mfh_setup_messages", "mfh_setup", "mfh_setup_image", "mfh_crs_image_set_b", "mfh_prove",
    "mfh_prove_partial", "mfh_prove_finish", "mfh_ct_to_lanes", "mfh_ct_from_lanes", "mfh_lanes_per_value", "mfh_digest128", "mfh_timing_drain", "mfh_timing_busy_ms", "mfh_timing_work_rows", "mfh_set_batch_image", "mfh_set_batch_slabs", "mfh_set_expand_path", "mfh_set_expand_periods", "mfh_set_encrypt_path", "mfh_set_batch_launch", "mfh_set_batch_bw", "mfh_set_batch_witness", "mfh_witness_poly_stream", "mfh_set_mm_chunk_rows", "mfh_set_mm_pack", "mfh_set_poly_exact", "mfh_poly_exact_fallbacks", "mfh_poly_exact_points", "mfh_set_poly_exact_points", "mfh_set_mm_stream", "mfh_add_dotp", "mfh_set_encrypt_chunks", "mfh_set_witness_per", "mfh_set_eval_path", "mfh_set_decrypt_path", "mfh_decrypt_rows",
    "mfh_crs_mm_share_bytes", "mfh_crs_expand_mm_share", "mfh_crs_set_resident_mm_share", "mfh_batch_chain", "mfh_batch_witness_cols", "mfh_batch_chain_from_w", "mfh_witness_poly_mm_cols", "mfh_prove_batch_partial", "mfh_prove_batch_finish",
    "mfh_resident_row_bytes", "mfh_crs_expand", "mfh_eval_rows_resident", "mfh_crs_set_resident",
    "mfh_witness_lanes", "mfh_witness_from_lanes", "mfh_prove_partial_w", "mfh_verify",
    "mfh_ssp_set_prg", "mfh_ssp_prg_make_t", "mfh_ssp_prg_fill",
    "mfh_resident_share_rows", "mfh_crs_expand_share", "mfh_crs_set_resident_share", "mfh_crs_set_resident_prefix",
    "mfh_prove_batch_supergroup", "mfh_prove_batch_stream_wait", "mfh_set_mm_width", "mfh_set_mm_queue", "mfh_set_mm_claim_log", "mfh_mm_claim_log_launches",
    "mfh_setup_public", "mfh_prove_public", "mfh_prove_batch_public", "mfh_vk_derive", "mfh_verify_public",
    "mfh_ssp_from_rows", "mfh_ssp_set_rows", "mfh_ssp_rows_fill", "mfh_ssp_rows_violations", "mfh_circuit_create", "mfh_circuit_destroy", "mfh_circuit_assign",
    "mfh_circuit_create_global", "mfh_circuit_create_ex", "mfh_circuit_create_out", "mfh_circuit_create_sum",
    "mfh_merkle_create", "mfh_merkle_destroy", "mfh_merkle_set_leaves", "mfh_merkle_root", "mfh_merkle_nodes", "mfh_merkle_paths",
    "mfh_sha256_records", "mfh_merkle_set_records", "mfh_merkle_update_rows", "mfh_merkle_update_records",
    "mfh_merkle_absent_rows", "mfh_merkle_insert_keys", "mfh_merkle_update_rows_cut", "mfh_merkle_update_records_cut", "mfh_merkle_insert_keys_cut",
    "mfh_merkle_remove_keys", "mfh_merkle_remove_keys_cut", "mfh_merkle_transfer_keys", "mfh_merkle_transfer_keys_cut",
    "mfh_merkle_paths_cut", "mfh_merkle_absent_rows_cut", "mfh_merkle_range_rows", "mfh_merkle_range_rows_cut",
    "mfh_merkle_load_keys", "mfh_merkle_check_table", "mfh_merkle_grow", "mfh_merkle_grow_leaves",
    "mfh_merkle_write_keys", "mfh_merkle_write_keys_cut", "mfh_merkle_block_keys", "mfh_merkle_block_keys_cut", "mfh_merkle_block_row_bytes",
]


# Entry points a library may lack and still load (calling one then raises AttributeError).  Each needs a reason: everything else is required of every library.
OPTIONAL_EXPORTS = {
    # tuning / test knobs of the persistent grid's item queues: no proof depends on them, and $MFHIP_LIB exists to time an older build of the same ABI (one that walks
    # fixed lists only) against this one through the same bench.py.  build() still requires them of the tree's own library (EXPORTS).
    "mfh_set_mm_queue": "tuning knob; older builds walk fixed lists",
    "mfh_set_mm_claim_log": "test instrumentation of mfh_set_mm_queue",
    "mfh_mm_claim_log_launches": "test instrumentation of mfh_set_mm_queue",
    # test knob of the CRS expansion's launch plan: the image does not depend on it, and an older build picks the plan from the row count alone
    "mfh_set_expand_periods": "test knob; older builds pick the periods per chunk from the row count",
    # the batch prover's streamed witness pass: the proofs do not depend on the route, and an older build runs k_witness_mm8q per super-group
    "mfh_set_batch_witness": "tuning knob; older builds run the witness pass per super-group",
    "mfh_witness_poly_stream": "the streamed pass alone (tests); older builds have mfh_witness_poly_mm only",
}


def load_library():
    """dlopen libmfhip.so; raises MfhError (never falls back) when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MfhError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    vp, u64, sz, i32, u32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
    sig = {
        "mfh_ctx_create": (i32, [ctypes.POINTER(vp), i32, ctypes.POINTER(_CParams)]),
        "mfh_ctx_destroy": (None, [vp]),
        "mfh_set_stream": (i32, [vp, vp]),
        "mfh_sync": (i32, [vp]),
        "mfh_scrub_staging": (i32, [vp]),
        "mfh_last_error": (ctypes.c_char_p, [vp]),
        "mfh_set_seed": (i32, [vp, ctypes.c_char_p]),
        "mfh_keystream": (i32, [vp, u64, vp, sz]),
        "mfh_sample_rows": (i32, [vp, u64, sz, vp]),
        "mfh_ct_add": (i32, [vp, vp, vp, vp, sz]),
        "mfh_ct_mul_ui": (i32, [vp, vp, vp, u32, sz]),
        "mfh_ct_addmul_ui": (i32, [vp, vp, vp, u32, sz]),
        "mfh_eval_rows": (i32, [vp, u64, sz, vp, vp, vp, vp, vp, i32]),
        "mfh_encrypt_rows": (i32, [vp, u64, sz, vp, vp, vp, vp]),
        "mfh_decrypt": (i32, [vp, vp, vp, sz, vp]),
        "mfh_ct_smudge": (i32, [vp, vp, sz, ctypes.c_char_p, sz, ctypes.c_char_p]),
        "mfh_ssp_upload": (i32, [vp, vp, vp, sz, sz]),
        "mfh_witness_poly": (i32, [vp, vp, ctypes.c_char_p, u32, vp]),
        "mfh_version": (ctypes.c_char_p, []),
        "mfh_workspace_bytes": (sz, [vp]),
        "mfh_last_kernel_ms": (ctypes.c_float, [vp, ctypes.c_char_p]),
        "mfh_set_timing": (i32, [vp, i32]),
        "mfh_set_overlap": (i32, [vp, i32]),
        "mfh_eval_rows_multi": (i32, [vp, u64, sz, vp, vp, u32, u32, vp, i32]),
        "mfh_poly_h_multi": (i32, [vp, vp, vp, u32]),
        "mfh_witness_poly_mm": (i32, [vp, vp, u32, ctypes.c_char_p, sz, vp, vp]),
        "mfh_witness_poly_multi": (i32, [vp, vp, u32, ctypes.c_char_p, sz, vp, vp]),
        "mfh_witness_poly_stream": (i32, [vp, vp, u32, ctypes.c_char_p, sz, vp, vp]),
        "mfh_crs_mm_image_bytes": (sz, [vp]),
        "mfh_crs_expand_mm": (i32, [vp, vp, vp]),
        "mfh_crs_set_resident_mm": (i32, [vp, vp]),
        "mfh_prove_batch": (i32, [vp, vp, vp, u32, ctypes.c_char_p, sz, vp, ctypes.c_char_p, sz, ctypes.c_char_p, vp]),
        "mfh_prove_batch_supergroup": (u32, [vp]),
        "mfh_set_mm_width": (i32, [vp, u32, i32]),
        "mfh_set_mm_queue": (i32, [vp, i32, u32, i32]),
        "mfh_set_mm_claim_log": (i32, [vp, vp, sz]),
        "mfh_mm_claim_log_launches": (u32, [vp, ctypes.POINTER(u32), u32]),
        "mfh_prove_batch_stream_wait": (i32, [vp, u32, vp]),
        "mfh_poly_mul": (i32, [vp, vp, sz, vp, sz, vp]),
        "mfh_poly_add": (i32, [vp, vp, vp, sz, vp]),
        "mfh_poly_prepare_t": (i32, [vp, vp]),
        "mfh_ssp_prepare": (i32, [vp, vp]),
        "mfh_poly_h": (i32, [vp, vp, vp]),
        "mfh_setup_messages": (i32, [vp, vp, u32, u32, u32, vp]),
        "mfh_setup": (i32, [vp, vp, u32, u32, u32, vp, vp, vp]),
        "mfh_setup_image": (i32, [vp, vp, u32, u32, u32, vp, vp, vp, vp]),
        "mfh_prove": (i32, [vp, vp, vp, ctypes.c_char_p, u32, ctypes.c_char_p, sz, ctypes.c_char_p, vp]),
        "mfh_prove_partial": (i32, [vp, vp, vp, ctypes.c_char_p, u32, u32, u32, vp]),
        "mfh_prove_finish": (i32, [vp, vp, ctypes.c_char_p, sz, ctypes.c_char_p]),
        "mfh_lanes_per_value": (u32, [vp]),
        "mfh_digest128": (i32, [vp, vp, sz, vp]),
        "mfh_ct_to_lanes": (i32, [vp, vp, sz, vp]),
        "mfh_ct_from_lanes": (i32, [vp, vp, sz, vp]),
        "mfh_add_dotp": (i32, [vp, vp, vp, vp, sz]),
        "mfh_crs_set_resident_prefix": (i32, [vp, vp, sz]),
        "mfh_resident_share_rows": (sz, [vp, u32, u32]),
        "mfh_crs_expand_share": (i32, [vp, vp, u32, u32, vp]),
        "mfh_crs_set_resident_share": (i32, [vp, vp, u32, u32]),
        "mfh_ssp_set_prg": (i32, [vp, u64, vp]),
        "mfh_ssp_prg_make_t": (i32, [vp, u64, ctypes.c_char_p, vp]),
        "mfh_ssp_prg_fill": (i32, [vp, u64, sz, sz, vp]),
        "mfh_verify": (i32, [vp, vp, u32, u32, u32, vp, vp, sz, vp]),
        "mfh_witness_lanes": (i32, [vp, vp, ctypes.c_char_p, u32, u32, vp]),
        "mfh_witness_from_lanes": (i32, [vp, vp, vp, u32, vp]),
        "mfh_prove_partial_w": (i32, [vp, vp, vp, ctypes.c_char_p, u32, u32, u32, vp, vp]),
        "mfh_resident_row_bytes": (sz, [vp]),
        "mfh_crs_expand": (i32, [vp, u64, sz, vp, vp]),
        "mfh_crs_image_set_b": (i32, [vp, sz, sz, vp, vp]),
        "mfh_eval_rows_resident": (i32, [vp, vp, sz, sz, vp, vp, vp, vp, i32]),
        "mfh_crs_set_resident": (i32, [vp, vp]),
        "mfh_timing_drain": (i32, [vp, ctypes.c_char_p, ctypes.POINTER(u64), ctypes.POINTER(ctypes.c_double), ctypes.POINTER(u64),
                                   ctypes.POINTER(ctypes.c_float)]),
        "mfh_timing_busy_ms": (ctypes.c_double, [vp]),
        "mfh_timing_work_rows": (u64, [vp]),
        "mfh_set_batch_image": (i32, [vp, i32]),
        "mfh_set_mm_chunk_rows": (i32, [vp, u32]),
        "mfh_set_mm_pack": (i32, [vp, i32]),
        "mfh_set_poly_exact": (i32, [vp, i32]),
        "mfh_poly_exact_fallbacks": (ctypes.c_long, [vp]),
        "mfh_poly_exact_points": (i32, [vp, ctypes.POINTER(u32)]),
        "mfh_set_poly_exact_points": (i32, [vp, ctypes.POINTER(u32)]),
        "mfh_set_mm_stream": (i32, [vp, i32, i32, i32, u32]),
        "mfh_set_batch_launch": (i32, [vp, u32, i32]),
        "mfh_set_batch_bw": (i32, [vp, i32]),
        "mfh_set_batch_witness": (i32, [vp, i32]),
        "mfh_set_encrypt_path": (i32, [vp, i32]),
        "mfh_set_expand_path": (i32, [vp, i32]),
        "mfh_set_expand_periods": (i32, [vp, u32]),
        "mfh_set_batch_slabs": (i32, [vp, u32]),
        "mfh_set_encrypt_chunks": (i32, [vp, u32]),
        "mfh_set_eval_path": (i32, [vp, i32]),
        "mfh_set_decrypt_path": (i32, [vp, i32]),
        "mfh_decrypt_rows": (i32, [vp, u64, sz, vp, vp, vp]),
        "mfh_set_witness_per": (i32, [vp, u32]),
        "mfh_crs_mm_share_bytes": (sz, [vp, u32, u32]),
        "mfh_crs_expand_mm_share": (i32, [vp, vp, u32, u32, vp]),
        "mfh_crs_set_resident_mm_share": (i32, [vp, vp, u32, u32]),
        "mfh_batch_chain": (i32, [vp, vp, u32, ctypes.c_char_p, sz, vp, vp, vp, vp]),
        "mfh_batch_witness_cols": (i32, [vp, vp, u32, ctypes.c_char_p, sz, vp, u32, u32, vp, sz]),
        "mfh_batch_chain_from_w": (i32, [vp, vp, u32, vp, vp, vp]),
        "mfh_witness_poly_mm_cols": (i32, [vp, vp, u32, ctypes.c_char_p, sz, vp, u32, u32, vp, sz]),
        "mfh_prove_batch_partial": (i32, [vp, vp, u32, u32, u32, ctypes.c_char_p, sz, vp, vp, vp, sz, vp]),
        "mfh_prove_batch_finish": (i32, [vp, vp, u32, vp, ctypes.c_char_p, sz, ctypes.c_char_p, vp]),
        "mfh_setup_public": (i32, [vp, vp, u32, u32, u32, u32, vp, vp, vp, vp]),
        "mfh_prove_public": (i32, [vp, vp, vp, u32, ctypes.c_char_p, u32, ctypes.c_char_p, sz, ctypes.c_char_p, vp]),
        "mfh_prove_batch_public": (i32, [vp, vp, vp, u32, u32, ctypes.c_char_p, sz, vp, ctypes.c_char_p, sz, ctypes.c_char_p, vp]),
        "mfh_vk_derive": (i32, [vp, vp, u32, u32, vp]),
        "mfh_verify_public": (i32, [vp, vp, u32, u32, u32, vp, vp, ctypes.c_char_p, sz, sz, vp]),
        "mfh_ssp_from_rows": (i32, [vp, u32, vp, vp, vp, vp]),
        "mfh_ssp_set_rows": (i32, [vp, u32, vp, vp, vp, u32]),
        "mfh_ssp_rows_fill": (i32, [vp, sz, sz, vp]),
        "mfh_ssp_rows_violations": (i32, [vp, u32, vp, sz, vp, vp]),
        "mfh_circuit_create": (i32, [vp, u32, u32, vp, u32, vp, ctypes.POINTER(vp)]),
        "mfh_circuit_create_global": (i32, [vp, u32, u32, vp, u32, vp, ctypes.POINTER(vp)]),
        "mfh_circuit_create_ex": (i32, [vp, u32, u32, vp, u32, vp, u32, vp, u32, ctypes.POINTER(vp)]),
        "mfh_circuit_create_out": (i32, [vp, u32, u32, vp, u32, vp, u32, vp, u32, vp, u32, ctypes.POINTER(vp)]),
        "mfh_circuit_create_sum": (i32, [vp, u32, u32, vp, u32, vp, u32, vp, u32, vp, u32, vp, u32, ctypes.POINTER(vp)]),
        "mfh_circuit_destroy": (None, [vp]),
        "mfh_circuit_assign": (i32, [vp, vp, u32, vp, sz, vp, sz, vp]),
        "mfh_merkle_create": (i32, [vp, u32, ctypes.POINTER(vp)]),
        "mfh_merkle_destroy": (None, [vp]),
        "mfh_merkle_set_leaves": (i32, [vp, vp, u32, u32, vp]),
        "mfh_merkle_root": (i32, [vp, vp, vp]),
        "mfh_merkle_nodes": (i32, [vp, u32, ctypes.POINTER(vp)]),
        "mfh_merkle_paths": (i32, [vp, vp, u32, vp, vp, sz]),
        "mfh_sha256_records": (i32, [vp, vp, sz, u32, u32, vp]),
        "mfh_merkle_set_records": (i32, [vp, vp, u32, u32, vp, sz, u32]),
        "mfh_merkle_update_rows": (i32, [vp, vp, u32, vp, vp, vp, sz, vp]),
        "mfh_merkle_update_records": (i32, [vp, vp, u32, vp, vp, sz, u32, vp, sz, vp, sz, vp]),
        "mfh_merkle_absent_rows": (i32, [vp, vp, vp, sz, u32, u32, u32, vp, sz, vp, sz, vp, vp]),
        "mfh_merkle_insert_keys": (i32, [vp, vp, vp, sz, u32, u32, u32, vp, sz, vp, sz, vp, sz, vp, vp, vp]),
        "mfh_merkle_update_rows_cut": (i32, [vp, vp, u32, vp, vp, u32, vp, vp, vp, vp]),
        "mfh_merkle_update_records_cut": (i32, [vp, vp, u32, vp, vp, sz, u32, vp, sz, u32, vp, vp, vp, vp]),
        "mfh_merkle_insert_keys_cut": (i32, [vp, vp, vp, sz, u32, u32, u32, vp, sz, vp, sz, u32, vp, vp, vp, vp, vp, vp]),
        "mfh_merkle_remove_keys": (i32, [vp, vp, vp, sz, u32, u32, u32, vp, sz, vp, sz, vp, vp, vp]),
        "mfh_merkle_remove_keys_cut": (i32, [vp, vp, vp, sz, u32, u32, u32, vp, sz, u32, vp, vp, vp, vp, vp, vp]),
        "mfh_merkle_transfer_keys": (i32, [vp, vp, vp, sz, u32, u32, u32, u32, vp, vp, sz, vp, vp, sz, vp, vp, vp]),
        "mfh_merkle_transfer_keys_cut": (i32, [vp, vp, vp, sz, u32, u32, u32, u32, vp, vp, sz, vp, u32, vp, vp, vp, vp, vp, vp]),
        "mfh_merkle_adjust_keys": (i32, [vp, vp, vp, sz, u32, u32, u32, u32, vp, sz, vp, vp, vp, sz, vp, vp, vp]),
        "mfh_merkle_adjust_keys_cut": (i32, [vp, vp, vp, sz, u32, u32, u32, u32, vp, sz, vp, vp, u32, vp, vp, vp, vp, vp, vp]),
        "mfh_merkle_balance_sum": (i32, [vp, vp, vp, sz, u32, u32, u32, vp, vp]),
        "mfh_merkle_write_keys": (i32, [vp, vp, vp, sz, u32, u32, u32, u32, u32, vp, sz, vp, sz, vp, sz, vp, sz, vp, vp, vp]),
        "mfh_merkle_write_keys_cut": (i32, [vp, vp, vp, sz, u32, u32, u32, u32, u32, vp, sz, vp, sz, vp, sz, u32, vp, vp, vp, vp, vp, vp]),
        "mfh_merkle_block_keys": (i32, [vp, vp, vp, sz, u32, u32, u32, u32, vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, vp, vp, sz, u32, vp, vp, vp, vp, vp, vp]),
        "mfh_merkle_block_keys_cut": (i32, [vp, vp, vp, sz, u32, u32, u32, u32, vp, vp, vp, sz, vp, vp, vp, vp, vp, sz, vp, vp, sz, u32, u32, vp, vp, vp, vp, vp, vp, vp,
                                            vp]),
        "mfh_merkle_block_row_bytes": (sz, [u32, u32, u32, u32, u32, u32, u32, u32, u32]),
        "mfh_merkle_paths_cut": (i32, [vp, vp, u32, vp, u32, vp, vp, vp]),
        "mfh_merkle_absent_rows_cut": (i32, [vp, vp, vp, sz, u32, u32, u32, vp, sz, u32, vp, vp, vp, vp, vp]),
        "mfh_merkle_range_rows": (i32, [vp, vp, vp, sz, u32, u32, vp, vp, u32, vp, vp, vp, vp, sz, vp]),
        "mfh_merkle_range_rows_cut": (i32, [vp, vp, vp, sz, u32, u32, vp, vp, u32, vp, vp, vp, u32, vp, vp, vp, vp]),
        "mfh_merkle_load_keys": (i32, [vp, vp, vp, sz, u32, u32, u32, vp, vp, u32, vp]),
        "mfh_merkle_check_table": (i32, [vp, vp, vp, sz, u32, u32, vp]),
        "mfh_merkle_grow": (i32, [vp, vp, u32, vp, sz, u32, vp, sz, vp, vp]),
        "mfh_merkle_grow_leaves": (i32, [vp, vp, u32, vp, vp]),
    }
    for name, (res, args) in sig.items():
        if name in OPTIONAL_EXPORTS and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)  # AttributeError if the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def rows_to_csr(rows):
    """(row_ptr, wire, coef) as contiguous uint32 arrays, from a CSR triple or from a sequence of rows of (wire, coef) pairs (coefficients taken mod p)"""
    if isinstance(rows, tuple) and len(rows) == 3 and all(isinstance(a, np.ndarray) for a in rows):
        row_ptr, wire, coef = rows
    else:
        lens = [len(r) for r in rows]
        row_ptr = np.zeros(len(lens) + 1, dtype=np.int64)
        np.cumsum(lens, out=row_ptr[1:])
        flat = [(int(w), int(a) % P) for r in rows for (w, a) in r]
        wire = np.array([w for w, _ in flat], dtype=np.int64)
        coef = np.array([a for _, a in flat], dtype=np.int64)
    if len(row_ptr) == 0 or min(np.min(row_ptr), np.min(wire, initial=0), np.min(coef, initial=0)) < 0:
        raise MfhError("rows: row_ptr needs nrows + 1 entries, and no entry may be negative")
    if max(np.max(row_ptr), np.max(wire, initial=0), np.max(coef, initial=0)) > 0xFFFFFFFF:
        raise MfhError("rows: entries must fit 32 bits")
    return tuple(np.ascontiguousarray(a, dtype=np.uint32) for a in (row_ptr, wire, coef))


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


CIRCUIT_MAX_WIRES = 32767  # MFH_CIRCUIT_MAX_WIRES: the most wires (nin + ngates) of a program whose wire state lives in LDS
CIRCUIT_GLOBAL = 1  # MFH_CIRCUIT_GLOBAL: mfh_circuit_create_ex flag, wire state in device memory


class CircuitProgram:
    """a compiled circuit's gate program on the device (mfh_circuit): made by Context.circuit_load, used by Context.circuit_assign.
    state: "lds" (wire state in LDS, at most CIRCUIT_MAX_WIRES wires) or "global" (wire state in device memory);
    extended: the circuit has a gate beyond XOR / AND / OR / NOT, an equality or an output (a mfh_circuit_create_ex / _out / _sum program);
    outputs: the number of computed public outputs (Circuit.output): above 0 circuit_assign writes the computed statement into bits [0, lu) of every
    witness row (mfh_circuit_create_out, or _sum);
    sums: the circuit has a weighted-sum gate (Circuit.wsum; mfh_circuit_create_sum)"""

    def __init__(self, ctx, nin, ngates, handle, state="lds", extended=False, outputs=0, sums=False):
        self._ctx, self.nin, self.ngates, self._h, self.state, self.extended, self.outputs = ctx, nin, ngates, handle, state, extended, outputs
        self.sums = sums

    def close(self):
        if self._h:
            self._ctx.lib.mfh_circuit_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _DeviceBytes:
    """n x 32 bytes of device memory that something else owns, as torch takes them without a copy (torch.as_tensor reads __cuda_array_interface__ and
    keeps this object, and with it `owner`, alive as long as the tensor)"""

    def __init__(self, ptr, n, owner):
        self.owner = owner
        self.__cuda_array_interface__ = {"shape": (n, 32), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None}


def _records(ctx, records, who):
    """(tensor, stride, length, n, host) of records as the device calls take them: a numpy uint8 [n, length], uploaded (host = True), or a torch uint8
    tensor on the context's device with stride(1) == 1 and stride(0) >= length, read in place (a column slice of a wider table is no copy)"""
    if isinstance(records, ctx.torch.Tensor):
        t = records
        if t.dtype != ctx.torch.uint8 or t.device != ctx.device or t.dim() != 2:
            raise MfhError(f"{who}: a device tensor of records is uint8 [n, length] on the context's device")
        n, length = int(t.shape[0]), int(t.shape[1])
        if (length > 1 and t.stride(1) != 1) or (n > 1 and t.stride(0) < length):
            raise MfhError(f"{who}: a device tensor of records has stride(1) == 1 and stride(0) >= length")
        return t, (int(t.stride(0)) if n > 1 else length), length, n, False
    a = np.asarray(records)
    if a.dtype != np.uint8 or a.ndim != 2:
        raise MfhError(f"{who}: records are a uint8 array [n, length]")
    n, length = a.shape
    return ctx.to_device(a).reshape(n, length), length, length, n, True


class BlockResult:
    """what MerkleTree.apply_block / apply_block_segments return.  rows: one 1-D np.uint8 view per step, its packed input row (None for a skipped step);
    index np.uint32 [nk, 2]; status np.uint8 [nk]; roots np.uint8 [nk + 1, 32]; first_update np.uint32 [nk + 1]; update_roots np.uint8 [nupd + 1, 32], the
    root behind every update; a cut call's segments and nodes (apply_block_segments)."""

    def __init__(self, tree, block, length, levels, cut, buf, row_at, index, status, r_all, first_update):
        self.block, self.length, self.levels, self.cut = block, length, levels, cut
        self.index, self.status, self.first_update = index, status, first_update
        self.update_roots = r_all[: int(first_update[-1]) + 1]
        self.roots = r_all[first_update]
        self._buf, self._row_at, self._rows = buf, row_at, None
        self.segments, self.nodes = None, None

    @property
    def rows(self):
        if self._rows is None:  # (views, made when first asked for)
            at = [int(x) for x in self._row_at]
            self._rows = [None if st else self._buf[at[j]: at[j + 1]] for j, st in enumerate(self.status)]
        return self._rows

    def rows_of(self, kind, field=None, expect=False):
        """(steps, rows [n, width]): the applied steps of one statement -- kind is Block.TRANSFER, Block.ADJUST or Block.WRITE, and for writes the field
        (lo, hi) and whether they carry an expectation -- and their rows stacked, ready for the _unpack and circuit_assign of that statement's program"""
        from .words import Block

        if kind not in (Block.TRANSFER, Block.ADJUST, Block.WRITE):
            raise MfhError("rows_of: kind is Block.TRANSFER, Block.ADJUST or Block.WRITE")
        if kind == Block.WRITE and field is None:
            raise MfhError("rows_of: a write's rows are those of one field (lo, hi)")
        steps = [j for j, s in enumerate(self.block.steps) if s[0] == kind and self.rows[j] is not None
                 and (kind != Block.WRITE or (tuple(s[2]) == tuple(int(x) for x in field) and (s[4] is not None) == bool(expect)))]
        rows = np.stack([self.rows[j] for j in steps]) if steps else np.zeros((0, 0), dtype=np.uint8)
        return steps, rows

    def bits_of(self, kind, field=None, expect=False):
        """rows_of with the rows as 0 / 1 arrays of the statement's nin bits: what Context.circuit_assign(prog, bits) takes"""
        from .words import Block

        steps, rows = self.rows_of(kind, field, expect)
        if not steps:
            return steps, rows
        ndir = (2 if kind == Block.TRANSFER else 1) * self.levels  # the direction bits: the last ceil(ndir / 8) bytes of a row
        nbits = 8 * (rows.shape[1] - (ndir + 7) // 8) + ndir
        return steps, np.unpackbits(rows, axis=1, bitorder="little")[:, :nbits]


class MerkleTree:
    """a SHA-256 Merkle tree of 2^depth leaves of 32 bytes in device memory (mfh_merkle): made by Context.merkle_tree, all leaves zero at first.
    parent = compress(IV, left || right), the node function of words.MerklePath; path_bits gives that statement's input rows for leaves of this tree."""

    def __init__(self, ctx, depth, handle):
        self._ctx, self.depth, self._h = ctx, depth, handle
        self.nin = 256 + 256 * (depth + 1) + depth  # input bits of words.MerklePath(depth)
        self._keep = []  # host leaves on their way: set_leaves only queues, the copies live until a call that waits for the stream

    def close(self):
        """frees the nodes: tensors that nodes() returned must not be used afterwards"""
        if self._h:
            self._ctx.lib.mfh_merkle_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._keep = []

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _row_bytes(self, zeros, head):
        """a statement's packed input row (csrc/merkle_rows.hpp): zero bytes where the root(s) are computed | head | depth siblings | ceil(depth / 8) index bytes"""
        return zeros + head + 32 * self.depth + (self.depth + 7) // 8

    def _unpack(self, rows, zeros, head):
        return np.unpackbits(rows, axis=1, bitorder="little")[:, : 8 * (zeros + head) + 257 * self.depth]

    @staticmethod
    def _indices(indices, who):
        idx = np.ascontiguousarray(indices, dtype=np.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() > 0xFFFFFFFF):
            raise MfhError(f"{who}: indices are in [0, 2^depth)")
        return idx.astype(np.uint32)

    def _leaves(self, leaves, who, aligned=False):
        """(tensor, host = it was uploaded); aligned: a device tensor that is not 16-byte aligned is copied"""
        c = self._ctx
        if isinstance(leaves, c.torch.Tensor):
            if leaves.dtype != c.torch.uint8 or leaves.device != c.device or not leaves.is_contiguous():
                raise MfhError(f"{who}: a device tensor of leaves is contiguous uint8 on the context's device")
            # (a clone is a fresh allocation: aligned; queued on torch's current stream, the context's)
            return (leaves.clone() if aligned and leaves.data_ptr() & 15 else leaves), False
        a = np.frombuffer(leaves, dtype=np.uint8) if isinstance(leaves, (bytes, bytearray, memoryview)) else np.asarray(leaves)
        if a.dtype != np.uint8:
            raise MfhError(f"{who}: leaves are bytes or uint8")
        return c.to_device(a), True

    def _table(self, table, who):
        """(tensor, stride, length) of a table of one record per leaf, used in place"""
        if not isinstance(table, self._ctx.torch.Tensor):
            raise MfhError(f"{who}: the table is a torch uint8 [2^depth, length] tensor on the context's device")
        tab, tstride, length, nrec, _ = _records(self._ctx, table, who)
        if nrec != 1 << self.depth:
            raise MfhError(f"{who}: the table has one record per leaf, 2^depth of them")
        return tab, tstride, length

    def _updates(self, n, head, roots, call):
        """the rows (and with roots=True the n + 1 roots) of n updates: call(rows, in_stride, roots or None) is the C call"""
        rows = np.zeros((n, self._row_bytes(64, head)), dtype=np.uint8)
        r = np.zeros((n + 1, 32), dtype=np.uint8) if roots else None
        self._ctx._chk(call(ctypes.c_void_p(rows.ctypes.data), rows.shape[1], ctypes.c_void_p(r.ctypes.data) if roots else None))
        self._keep = []
        if roots and not n:
            r[0] = np.frombuffer(self.root(), dtype=np.uint8)
        return (rows, r) if roots else rows

    def _update_bits(self, out, head, roots):
        bits = self._unpack(out[0] if roots else out, 64, head)
        return (bits, out[1]) if roots else bits

    def set_leaves(self, first, leaves):
        """leaves [first, first + n) <- leaves: bytes-like of 32 n bytes, a numpy uint8 [n, 32], or a torch uint8 tensor on the context's device, which is
        read in place when the context's stream reaches the call (mfh_merkle_set_leaves: queue-only); their ancestors are recomputed"""
        c = self._ctx
        t, host = self._leaves(leaves, "set_leaves")
        if host:
            self._keep.append(t)
        if t.numel() % 32:
            raise MfhError("set_leaves: leaves are 32 bytes each")
        c._chk(c.lib.mfh_merkle_set_leaves(c._h, self._h, int(first), t.numel() // 32, _ptr(t)))

    def set_records(self, first, records):
        """leaves [first, first + n) <- SHA-256 of the n records, hashed on the device straight into the leaves; their ancestors are recomputed
        (mfh_merkle_set_records: queue-only).  records: a numpy uint8 [n, length], uploaded, or a torch uint8 tensor [n, length] on the context's device
        with stride(1) == 1 and stride(0) >= length, read in place when the context's stream reaches the call"""
        c = self._ctx
        t, stride, length, n, host = _records(c, records, "set_records")
        if host:
            self._keep.append(t)
        c._chk(c.lib.mfh_merkle_set_records(c._h, self._h, int(first), n, _ptr(t), stride, length))

    def root(self):
        """the root's 32 bytes (mfh_merkle_root; waits for the stream)"""
        out = (ctypes.c_uint8 * 32)()
        self._ctx._chk(self._ctx.lib.mfh_merkle_root(self._ctx._h, self._h, out))
        self._keep = []
        return bytes(out)

    def nodes(self, level):
        """level `level` (0 = the leaves, depth = the root) as a torch uint8 [2^(depth - level), 32] view of the tree's memory: no copy, and ordered behind
        the tree's updates only on the context's stream"""
        p = ctypes.c_void_p()
        self._ctx._chk(self._ctx.lib.mfh_merkle_nodes(self._h, int(level), ctypes.byref(p)))
        return self._ctx.torch.as_tensor(_DeviceBytes(p.value, 1 << (self.depth - level), self), device=self._ctx.device)

    def path_rows(self, indices):
        """np.uint8 [nb, ceil(nin / 8)]: the packed input rows of words.MerklePath(depth) for the leaves at `indices` (mfh_merkle_paths; indices may repeat)"""
        idx = self._indices(indices, "path_rows")
        rows = np.zeros((len(idx), self._row_bytes(32, 32)), dtype=np.uint8)
        self._ctx._chk(self._ctx.lib.mfh_merkle_paths(self._ctx._h, self._h, len(idx), ctypes.c_void_p(idx.ctypes.data), ctypes.c_void_p(rows.ctypes.data),
                                                      rows.shape[1]))
        self._keep = []
        return rows

    @staticmethod
    def _record_array(records, nb, who):
        """the records of record_rows / record_segments as np.uint8 [nb, length]: an array of that shape, or nb bytes-likes of one length"""
        if isinstance(records, np.ndarray):
            rec = records
        else:
            rec = [np.frombuffer(bytes(r), dtype=np.uint8) for r in records]
            if len({len(r) for r in rec}) > 1:
                raise MfhError(f"{who}: the records are of one length")
            rec = np.stack(rec) if rec else np.zeros((0, 0), dtype=np.uint8)
        if rec.dtype != np.uint8 or rec.ndim != 2 or len(rec) != nb:
            raise MfhError(f"{who}: records are uint8 [nb, length], one per index")
        return rec

    def _record_rows(self, records, indices):
        paths = self.path_rows(indices)
        rec = self._record_array(records, len(paths), "record_rows")
        return np.concatenate([np.zeros((len(paths), 32), dtype=np.uint8), rec, paths[:, 64:]], axis=1), rec.shape[1]

    def record_rows(self, records, indices):
        """np.uint8 [nb, ceil(nin / 8)]: the packed input rows of words.MerkleRecord(length, depth), records[i] (a uint8 [nb, length] array, or nb
        bytes-likes of one length) being the record at leaf indices[i]: 32 zero bytes where the root is computed, the record's bytes, then the siblings
        and the index bytes of path_rows(indices).  That the record hashes to that leaf is not checked here: the root circuit_assign computes shows it."""
        return self._record_rows(records, indices)[0]

    def record_bits(self, records, indices):
        """np.uint8 [nb, nin] of 0 / 1: what Context.circuit_assign(prog, bits) takes for words.MerkleRecord(length, depth)"""
        rows, length = self._record_rows(records, indices)
        return self._unpack(rows, 32, length)

    def path_bits(self, indices):
        """np.uint8 [nb, nin] of 0 / 1: what Context.circuit_assign(prog, bits) takes for words.MerklePath(depth)"""
        return self._unpack(self.path_rows(indices), 32, 32)

    def update_rows(self, indices, new_leaves, roots=False):
        """n sequential one-leaf updates, leaf indices[k] <- new_leaves[k] in order (mfh_merkle_update_rows: depth + 1 launches for the batch; waits for the
        stream).  Returns np.uint8 [n, 128 + 32 depth + ceil(depth / 8)]: row k is the packed input row of words.MerkleUpdate(depth) taken from the tree
        as it stood before update k -- indices may repeat, and update k sees what updates 0 .. k - 1 did.  With roots=True a pair whose second element
        is np.uint8 [n + 1, 32], the roots R_0 .. R_n: statement k is MerkleUpdate.statement(R_k, R_k+1).
        new_leaves: bytes-like of 32 n bytes, a numpy uint8 [n, 32], or a torch uint8 tensor on the context's device (contiguous; copied when it is not
        16-byte aligned), read when the context's stream reaches the call -- the digests Context.sha256_records returns feed straight in."""
        c = self._ctx
        idx = self._indices(indices, "update_rows")
        t, _ = self._leaves(new_leaves, "update_rows", aligned=True)
        if t.numel() != 32 * len(idx):
            raise MfhError("update_rows: one leaf of 32 bytes per index")
        return self._updates(len(idx), 64, roots, lambda rows, stride, r: c.lib.mfh_merkle_update_rows(
            c._h, self._h, len(idx), ctypes.c_void_p(idx.ctypes.data), _ptr(t) if len(idx) else None, rows, stride, r))

    def update_bits(self, indices, new_leaves, roots=False):
        """update_rows as np.uint8 [n, 1024 + 257 depth] of 0 / 1: what Context.circuit_assign(prog, bits) takes for words.MerkleUpdate(depth)"""
        return self._update_bits(self.update_rows(indices, new_leaves, roots), 64, roots)

    def update_records(self, table, indices, new_records, roots=False):
        """n sequential one-record updates of a table of records and this tree, record indices[k] <- new_records[k] in order (mfh_merkle_update_records: one
        hash launch, two copy launches and depth + 1 tree launches for the batch; waits for the stream).  Returns np.uint8 [n, 64 + 2 length + 32 depth +
        ceil(depth / 8)]: row k is the packed input row of words.MerkleRecordUpdate(length, depth) taken from the table and the tree as they stood before
        update k -- indices may repeat, and update k sees what updates 0 .. k - 1 did.  With roots=True a pair whose second element is np.uint8 [n + 1, 32],
        the roots R_0 .. R_n: statement k is MerkleRecordUpdate.statement(R_k, R_k+1).
        table: a torch uint8 [2^depth, length] tensor on the context's device with stride(1) == 1 and stride(0) >= length (a column slice of a wider table
        is used in place), MODIFIED IN PLACE: afterwards it holds each touched record's last new value.  Leaf i of the tree must be SHA-256 of table[i]
        (the state after set_records(0, table)); that is not checked, the old root circuit_assign computes from a row shows it.
        new_records: a numpy uint8 [n, length], uploaded, or a device tensor under the table's rules, read when the context's stream reaches the call; it
        must not overlap the table."""
        c = self._ctx
        idx = self._indices(indices, "update_records")
        tab, tstride, length = self._table(table, "update_records")
        new, nstride, nlength, n, _ = _records(c, new_records, "update_records")
        if n != len(idx) or nlength != length:
            raise MfhError("update_records: one new record of the table's length per index")
        return self._updates(len(idx), 2 * length, roots, lambda rows, stride, r: c.lib.mfh_merkle_update_records(
            c._h, self._h, len(idx), ctypes.c_void_p(idx.ctypes.data), _ptr(tab), tstride, length, _ptr(new) if len(idx) else None, nstride, rows, stride, r))

    def update_record_bits(self, table, indices, new_records, roots=False):
        """update_records as np.uint8 [n, 512 + 16 length + 257 depth] of 0 / 1: what Context.circuit_assign(prog, bits) takes for
        words.MerkleRecordUpdate(length, depth)"""
        return self._update_bits(self.update_records(table, indices, new_records, roots), 2 * int(table.shape[1]), roots)

    # ---- the key calls on an indexed table: what their arguments share
    def _keys(self, table, keys, who, count="nk"):
        """(the table's tensor, its stride, its length, the keys as a contiguous np.uint8 [n, key_bytes]) of a key call"""
        tab, tstride, length = self._table(table, who)
        k = np.ascontiguousarray(keys)
        if k.dtype != np.uint8 or k.ndim != 2 or not 1 <= k.shape[1] <= 32 or length < 2 * k.shape[1]:
            raise MfhError(f"{who}: keys are uint8 [{count}, key_bytes], 1 <= key_bytes <= 32 and 2 key_bytes <= length")
        return tab, tstride, length, k

    @staticmethod
    def _payloads(payloads, nk, plen, who):
        """None, or the payloads as a contiguous np.uint8 [nk, plen]"""
        if payloads is None:
            return None
        pay = np.ascontiguousarray(payloads)
        if pay.dtype != np.uint8 or pay.shape != (nk, plen):
            raise MfhError(f"{who}: payloads are uint8 [nk, length - 2 key_bytes]")
        return pay

    @staticmethod
    def _step_head(table, keys, nrec, zeros):
        """the bytes in front of the two tails in the row of a key step with nrec records: the zeros where the tops are computed, the key, the records"""
        return zeros + np.ascontiguousarray(keys).shape[1] + nrec * int(table.shape[1])

    def _key_steps(self, who, step, table, keys, payloads=None, roots=False, cut=False, cuts=None, transfer=None):
        """the body of insert_keys, remove_keys, transfer_keys and, with cut=True, their *_segments forms (whatever `cuts` is then, _cut judges it): mfh_merkle_<step>_keys[_cut] with the rows of a statement of three
        (insert) or two (remove, transfer) records, index, status and roots allocated here.  Uncut: (rows, index) and with roots=True the nk + 1 roots; cut: (rows,
        nodes_p, nodes_s, index), from the 2 nk + 1 roots.  transfer = (to_keys, amounts, amount_bytes): `keys` are then the senders'"""
        c = self._ctx
        tab, tstride, length, k = self._keys(table, keys, who)
        nk, kb = k.shape
        vp = ctypes.c_void_p
        nrec, extra, more = 2, (), 0
        keys_args = (kb, nk, vp(k.ctypes.data), kb)
        if step == "insert":
            pay = self._payloads(payloads, nk, length - 2 * kb, who)
            nrec, extra = 3, (vp(pay.ctypes.data) if pay is not None else None, length - 2 * kb)
        if step == "transfer":
            to, amounts, ab = transfer
            to = np.ascontiguousarray(to)
            if to.dtype != np.uint8 or to.shape != k.shape:
                raise MfhError(f"{who}: from_keys and to_keys are uint8 [nk, key_bytes], one pair a transfer")
            if not isinstance(ab, (int, np.integer)) or not 1 <= ab <= 8 or length < 2 * kb + ab:
                raise MfhError(f"{who}: 1 <= amount_bytes <= 8 and 2 key_bytes + amount_bytes <= length")
            try:
                values = [int(a) for a in amounts]
            except (TypeError, ValueError):
                values = None
            if values is None or len(values) != nk or any(not 0 <= a < 1 << 64 for a in values):
                raise MfhError(f"{who}: amounts are nk integers in [0, 2^64), one a transfer")
            amt = np.array(values, dtype=np.uint64).reshape(nk)
            more = kb + int(ab)  # the row has k_from | k_to | the amount where the other steps' rows have the key
            keys_args = (kb, int(ab), nk, vp(k.ctypes.data), vp(to.ctypes.data), kb, vp(amt.ctypes.data))
        head = self._step_head(table, keys, nrec, 128 if cut else 64) + more
        if not cut:
            rows = np.zeros((nk, head + 64 * self.depth + (2 * self.depth + 7) // 8), dtype=np.uint8)
            out = (vp(rows.ctypes.data), rows.shape[1])
            r = np.zeros((nk + 1, 32), dtype=np.uint8) if roots else None
        else:
            rows, out, keep = self._cut(cuts, who, nk, lambda c0: head + 64 * c0 + (2 * c0 + 7) // 8, 2 * nk)
            r = np.zeros((2 * nk + 1, 32), dtype=np.uint8)
        index = np.zeros((nk, 2), dtype=np.uint32)
        status = np.zeros(nk, dtype=np.uint8)
        call = getattr(c.lib, f"mfh_merkle_{step}_keys" + ("_cut" if cut else ""))
        c._chk(call(c._h, self._h, _ptr(tab), tstride, length, *keys_args, *extra, *out, vp(r.ctypes.data) if r is not None else None,
                    vp(index.ctypes.data), vp(status.ctypes.data)))
        if nk:
            self._keep = []  # (the call waited for the stream)
        elif r is not None:
            r[0] = np.frombuffer(self.root(), dtype=np.uint8)
        if not cut:
            return (rows, index, r) if roots else (rows, index)
        nodes = self._cut_nodes(rows, r)
        return rows, nodes[0::2], nodes[1::2], index

    def _key_step_bits(self, out, head):
        """the uncut rows of a key step as 0 / 1"""
        return (np.unpackbits(out[0], axis=1, bitorder="little")[:, : 8 * head + 514 * self.depth],) + tuple(out[1:])

    def _absent(self, table, keys, who, want_rows):
        c = self._ctx
        tab, tstride, length, k = self._keys(table, keys, who, "nq")
        nq, kb = k.shape
        index = np.zeros(nq, dtype=np.uint32)
        status = np.zeros(nq, dtype=np.uint8)
        rows = np.zeros((nq, self._row_bytes(32, kb + length)), dtype=np.uint8) if want_rows else None
        vp = ctypes.c_void_p
        c._chk(c.lib.mfh_merkle_absent_rows(c._h, self._h, _ptr(tab), tstride, length, kb, nq, vp(k.ctypes.data), kb, vp(rows.ctypes.data) if want_rows else None,
                                            rows.shape[1] if want_rows else 0, vp(index.ctypes.data), vp(status.ctypes.data)))
        if nq:
            self._keep = []  # (the call waited for the stream)
        return rows, index, status

    def locate_keys(self, table, keys):
        """(index uint32 [nq], status uint8 [nq]): for every key the record of the INDEXED table (words.MerkleAbsent has the data model) that decides it
        -- status 0, absent: the record with lo < key < hi; 1, present: the record whose own key it is; 2, no record (only in a malformed table), index
        0xFFFFFFFF.  mfh_merkle_absent_rows with no rows: one launch that streams the table's keys, whatever nq; waits for the stream.
        table: a torch uint8 [2^depth, length] tensor on the context's device under update_records' rules, only read; the records may stand in any
        order.  keys: np.uint8 [nq, key_bytes], in any order, repeats allowed, neither all-zero nor all-0xFF."""
        _, index, status = self._absent(table, keys, "locate_keys", False)
        return index, status

    def absent_rows(self, table, keys):
        """(rows, index, status): locate_keys, and np.uint8 [nq, 32 + key_bytes + length + 32 depth + ceil(depth / 8)] rows: row k is the packed input
        row of words.MerkleAbsent(key_bytes, length, depth) for keys[k] and the located record (mfh_merkle_absent_rows).  The row of a present key
        (status 1) is complete and does not hold; the row of status 2 has the key alone."""
        return self._absent(table, keys, "absent_rows", True)

    def absent_bits(self, table, keys):
        """absent_rows with the rows as np.uint8 [nq, 256 + 8 key_bytes + 8 length + 257 depth] of 0 / 1: what Context.circuit_assign(prog, bits) takes
        for words.MerkleAbsent(key_bytes, length, depth)"""
        rows, index, status = self._absent(table, keys, "absent_bits", True)
        return self._unpack(rows, 32, np.ascontiguousarray(keys).shape[1] + int(table.shape[1])), index, status

    def insert_keys(self, table, keys, payloads=None, roots=False):
        """(rows, index): nk sequential key inserts into an INDEXED table (words.MerkleAbsent has the data model) and this tree in one call
        (mfh_merkle_insert_keys; waits for the stream).  Insert j changes the hi of the record whose range holds keys[j] and writes the record (keys[j] | the old
        hi | payloads[j]) into the lowest inert slot; a later key may fall into a range an earlier one has split.  rows is np.uint8 [nk, 64 + key_bytes + 3
        length + 64 depth + ceil(2 depth / 8)]: row j is the packed input row of words.MerkleInsert(key_bytes, length, depth) taken from table and tree as
        they stood before insert j.  index is np.uint32 [nk, 2]: (the slot whose hi changed, the slot that received the new record).  With roots=True a
        triple whose last element is np.uint8 [nk + 1, 32], the roots R_0 .. R_nk: statement j is MerkleInsert.statement(R_j, R_j+1, keys[j]).
        table: under update_records' rules, MODIFIED IN PLACE.  keys: np.uint8 [nk, key_bytes] under locate_keys' rules, all different.  payloads: None (all
        zero) or np.uint8 [nk, length - 2 key_bytes].  MfhError with the library's text, table and tree untouched, when a key is a member already, no record
        holds a key, or the table has fewer than nk inert slots."""
        return self._key_steps("insert_keys", "insert", table, keys, payloads, roots)

    def insert_bits(self, table, keys, payloads=None, roots=False):
        """insert_keys with the rows as np.uint8 [nk, 512 + 8 key_bytes + 24 length + 514 depth] of 0 / 1: what Context.circuit_assign(prog, bits) takes for
        words.MerkleInsert(key_bytes, length, depth)"""
        return self._key_step_bits(self.insert_keys(table, keys, payloads, roots), self._step_head(table, keys, 3, 64))

    # ---- the path cut into level ranges (words.MerkleSegment): one row array a segment, and the published node pairs
    def _cut(self, cuts, who, n0, row0, nupper, upper=128):
        """(the row arrays: n0 rows of row0 bytes for segment 0, nupper rows a MerkleSegment -- upper=64: a MerkleClimb, whose tail starts at byte 64 --, the C
        arguments ncuts, h_cuts, h_rows, h_strides)"""
        from .words import CircuitError, segment_levels

        try:
            ranges = segment_levels(self.depth, [int(x) for x in cuts])
        except (CircuitError, TypeError, ValueError):
            raise MfhError(f"{who}: cuts are 1 <= c_0 < .. < c_G-1 < depth, at least one") from None
        rows = [np.zeros((n0, row0(ranges[0][1])), dtype=np.uint8)]
        rows += [np.zeros((nupper, upper + 32 * (hi - lo) + (hi - lo + 7) // 8), dtype=np.uint8) for lo, hi in ranges[1:]]
        c_cuts = np.array([lo for lo, _ in ranges[1:]], dtype=np.uint32)
        ptrs = (ctypes.c_void_p * len(rows))(*[r.ctypes.data for r in rows])
        strides = (ctypes.c_size_t * len(rows))(*[r.shape[1] for r in rows])
        return rows, (len(c_cuts), ctypes.c_void_p(c_cuts.ctypes.data), ptrs, strides), c_cuts

    def _cut_nodes(self, rows, r):
        """np.uint8 [n, G + 1, 2, 32], the published pairs (X_g, X_g') of every update in digest byte order: the heads of its upper segments' rows, then (R_k, R_k+1)"""
        n, G = len(r) - 1, len(rows) - 1
        nodes = np.zeros((n, G + 1, 2, 32), dtype=np.uint8)
        for g in range(G):
            nodes[:, g] = rows[g + 1][:, :64].reshape(n, 2, 8, 4)[..., ::-1].reshape(n, 2, 32)
        nodes[:, G, 0], nodes[:, G, 1] = r[:-1], r[1:]
        return nodes

    def _cut_unpack(self, rows, cuts, head0):
        edges = [0] + [int(x) for x in cuts] + [self.depth]
        levels = [hi - lo for lo, hi in zip(edges, edges[1:])]
        per = head0(levels[0])
        return [np.unpackbits(r, axis=1, bitorder="little")[:, : per if g == 0 else 1024 + 257 * levels[g]] for g, r in enumerate(rows)]

    def update_segments(self, indices, new_leaves, cuts, roots=False):
        """update_rows with the path cut at levels `cuts` (words.segment_levels; mfh_merkle_update_rows_cut: one more launch a chunk).  Returns (rows, nodes):
        rows is a list of G + 1 arrays, rows[0][k] the packed input row of words.MerkleUpdate(c_0) of update k -- over the subtree of height c_0 that holds
        the leaf -- and rows[g][k], g >= 1, that of words.MerkleSegment(c_g - c_g-1); nodes is np.uint8 [n, G + 1, 2, 32], the published pairs (X_g, X_g') of
        every update in digest byte order, (X_G, X_G') = (R_k, R_k+1): MerkleUpdate.statement(*nodes[k, 0]) and MerkleSegment.chain(nodes[k]) are the G + 1
        statements of update k.  With roots=True a triple whose last element is the n + 1 roots."""
        c = self._ctx
        idx = self._indices(indices, "update_segments")
        t, _ = self._leaves(new_leaves, "update_segments", aligned=True)
        if t.numel() != 32 * len(idx):
            raise MfhError("update_segments: one leaf of 32 bytes per index")
        rows, cargs, keep = self._cut(cuts, "update_segments", len(idx), lambda c0: 128 + 32 * c0 + (c0 + 7) // 8, len(idx))
        r = np.zeros((len(idx) + 1, 32), dtype=np.uint8)
        c._chk(c.lib.mfh_merkle_update_rows_cut(c._h, self._h, len(idx), ctypes.c_void_p(idx.ctypes.data), _ptr(t) if len(idx) else None, *cargs,
                                                ctypes.c_void_p(r.ctypes.data)))
        self._keep = []
        if not len(idx):
            r[0] = np.frombuffer(self.root(), dtype=np.uint8)
        nodes = self._cut_nodes(rows, r)
        return (rows, nodes, r) if roots else (rows, nodes)

    def update_segment_bits(self, indices, new_leaves, cuts, roots=False):
        """update_segments with every segment's rows as 0 / 1 arrays: what Context.circuit_assign takes for MerkleUpdate(c_0) and the MerkleSegments"""
        out = self.update_segments(indices, new_leaves, cuts, roots)
        return (self._cut_unpack(out[0], cuts, lambda c0: 1024 + 257 * c0),) + tuple(out[1:])

    def update_record_segments(self, table, indices, new_records, cuts, roots=False):
        """update_records with the path cut at levels `cuts` (mfh_merkle_update_records_cut): as update_segments, rows[0][k] being the packed input row of
        words.MerkleRecordUpdate(length, c_0)"""
        c = self._ctx
        idx = self._indices(indices, "update_record_segments")
        tab, tstride, length = self._table(table, "update_record_segments")
        new, nstride, nlength, n, _ = _records(c, new_records, "update_record_segments")
        if n != len(idx) or nlength != length:
            raise MfhError("update_record_segments: one new record of the table's length per index")
        rows, cargs, keep = self._cut(cuts, "update_record_segments", n, lambda c0: 64 + 2 * length + 32 * c0 + (c0 + 7) // 8, n)
        r = np.zeros((n + 1, 32), dtype=np.uint8)
        c._chk(c.lib.mfh_merkle_update_records_cut(c._h, self._h, n, ctypes.c_void_p(idx.ctypes.data), _ptr(tab), tstride, length, _ptr(new) if n else None, nstride,
                                                   *cargs, ctypes.c_void_p(r.ctypes.data)))
        self._keep = []
        if not n:
            r[0] = np.frombuffer(self.root(), dtype=np.uint8)
        nodes = self._cut_nodes(rows, r)
        return (rows, nodes, r) if roots else (rows, nodes)

    def update_record_segment_bits(self, table, indices, new_records, cuts, roots=False):
        """update_record_segments with every segment's rows as 0 / 1 arrays"""
        out = self.update_record_segments(table, indices, new_records, cuts, roots)
        length = int(table.shape[1])
        return (self._cut_unpack(out[0], cuts, lambda c0: 512 + 16 * length + 257 * c0),) + tuple(out[1:])

    def insert_key_segments(self, table, keys, cuts, payloads=None):
        """insert_keys with the path cut at levels `cuts` (mfh_merkle_insert_keys_cut).  Returns (rows, nodes_p, nodes_s, index): rows[0][j] is the packed input
        row of words.MerkleInsert(key_bytes, length, c_0, joined=False) of insert j; rows[g], g >= 1, holds one words.MerkleSegment row per UPDATE, row 2 j that
        of p's update of insert j and row 2 j + 1 that of s's; nodes_p and nodes_s are np.uint8 [nk, G + 1, 2, 32], the published pairs of the two updates:
        segment 0's statement is statement(*nodes_p[j, 0], *nodes_s[j, 0], keys[j]), the upper ones MerkleSegment.chain(nodes_p[j]) and chain(nodes_s[j]), and
        nodes_p[j, G, 1] == nodes_s[j, G, 0] is the root between the two updates, which becomes public.  index as insert_keys gives it."""
        return self._key_steps("insert_key_segments", "insert", table, keys, payloads, cut=True, cuts=cuts)

    def insert_key_segment_bits(self, table, keys, cuts, payloads=None):
        """insert_key_segments with every segment's rows as 0 / 1 arrays"""
        out = self.insert_key_segments(table, keys, cuts, payloads)
        head = self._step_head(table, keys, 3, 128)
        return (self._cut_unpack(out[0], cuts, lambda c0: 8 * head + 514 * c0),) + tuple(out[1:])

    # ---- the READ path cut into level ranges (words.MerkleClimb): one row array a segment, and the published nodes
    def _climb_nodes(self, rows):
        """np.uint8 [n, G + 1, 32], the published nodes X_g of every statement in digest byte order: the heads of its upper segments' rows, then the root"""
        n, G = len(rows[0]), len(rows) - 1
        nodes = np.zeros((n, G + 1, 32), dtype=np.uint8)
        for g in range(G):
            nodes[:, g] = rows[g + 1][:, :32].reshape(n, 8, 4)[..., ::-1].reshape(n, 32)
        nodes[:, G] = np.frombuffer(self.root(), dtype=np.uint8)
        return nodes

    def _climb_unpack(self, rows, cuts, head0):
        edges = [0] + [int(x) for x in cuts] + [self.depth]
        levels = [hi - lo for lo, hi in zip(edges, edges[1:])]
        return [np.unpackbits(r, axis=1, bitorder="little")[:, : (head0 if g == 0 else 512) + 257 * levels[g]] for g, r in enumerate(rows)]

    def path_segments(self, indices, cuts):
        """path_rows with the path cut at levels `cuts` (words.segment_levels; mfh_merkle_paths_cut: ONE launch a chunk, straight from the tree's nodes).
        Returns (rows, nodes): rows is a list of G + 1 arrays, rows[0][k] the packed input row of words.MerklePath(c_0) of statement k -- over the subtree of
        height c_0 that holds the leaf -- and rows[g][k], g >= 1, that of words.MerkleClimb(c_g - c_g-1); nodes is np.uint8 [n, G + 1, 32], the published nodes
        X_g of every statement in digest byte order, nodes[:, G] the root: MerklePath.statement(nodes[k, 0]) and MerkleClimb.chain(nodes[k]) are the G + 1
        statements of statement k.  The tree is only read; waits for the stream."""
        return self._path_segments(indices, cuts, "path_segments")

    def _path_segments(self, indices, cuts, who):
        c = self._ctx
        idx = self._indices(indices, who)
        rows, cargs, keep = self._cut(cuts, who, len(idx), lambda c0: 64 + 32 * c0 + (c0 + 7) // 8, len(idx), upper=64)
        c._chk(c.lib.mfh_merkle_paths_cut(c._h, self._h, len(idx), ctypes.c_void_p(idx.ctypes.data), *cargs))
        self._keep = []
        return rows, self._climb_nodes(rows)

    def path_segment_bits(self, indices, cuts):
        """path_segments with every segment's rows as 0 / 1 arrays: what Context.circuit_assign takes for MerklePath(c_0) and the MerkleClimbs"""
        rows, nodes = self.path_segments(indices, cuts)
        return self._climb_unpack(rows, cuts, 512), nodes

    def _record_segments(self, records, indices, cuts):
        rows, nodes = self._path_segments(indices, cuts, "record_segments")
        rec = self._record_array(records, len(rows[0]), "record_segments")
        rows[0] = np.concatenate([np.zeros((len(rec), 32), dtype=np.uint8), rec, rows[0][:, 64:]], axis=1)
        return rows, nodes, rec.shape[1]

    def record_segments(self, records, indices, cuts):
        """record_rows with the path cut at levels `cuts`: as path_segments, rows[0][k] being the packed input row of words.MerkleRecord(length, c_0) -- the
        record spliced on the host in place of the leaf, as record_rows does -- and segment 0's statement MerkleRecord.statement(nodes[k, 0])"""
        return self._record_segments(records, indices, cuts)[:2]

    def record_segment_bits(self, records, indices, cuts):
        """record_segments with every segment's rows as 0 / 1 arrays"""
        rows, nodes, length = self._record_segments(records, indices, cuts)
        return self._climb_unpack(rows, cuts, 256 + 8 * length), nodes

    def absent_segments(self, table, keys, cuts):
        """absent_rows with the path cut at levels `cuts` (mfh_merkle_absent_rows_cut).  Returns (rows, nodes, index, status): rows and nodes as path_segments
        gives them, rows[0][k] being the packed input row of words.MerkleAbsent(key_bytes, length, c_0) for keys[k] and the located record, and segment 0's
        statement MerkleAbsent(..).statement(nodes[k, 0], keys[k]); index and status as locate_keys gives them.  The row set of a present key (status 1) is
        complete and segment 0 does not hold; a query of status 2 has the key alone in segment 0, all-zero rows above it and all-zero nodes below the root."""
        c = self._ctx
        tab, tstride, length, k = self._keys(table, keys, "absent_segments", "nq")
        nq, kb = k.shape
        index = np.zeros(nq, dtype=np.uint32)
        status = np.zeros(nq, dtype=np.uint8)
        rows, cargs, keep = self._cut(cuts, "absent_segments", nq, lambda c0: 32 + kb + length + 32 * c0 + (c0 + 7) // 8, nq, upper=64)
        vp = ctypes.c_void_p
        c._chk(c.lib.mfh_merkle_absent_rows_cut(c._h, self._h, _ptr(tab), tstride, length, kb, nq, vp(k.ctypes.data), kb, *cargs, vp(index.ctypes.data),
                                                vp(status.ctypes.data)))
        self._keep = []
        return rows, self._climb_nodes(rows), index, status

    def absent_segment_bits(self, table, keys, cuts):
        """absent_segments with every segment's rows as 0 / 1 arrays"""
        rows, nodes, index, status = self.absent_segments(table, keys, cuts)
        head0 = 256 + 8 * (np.ascontiguousarray(keys).shape[1] + int(table.shape[1]))
        return self._climb_unpack(rows, cuts, head0), nodes, index, status

    # ---- range reads (words.MerkleLink): the records of a key range in key order, their rows, and the same with the path cut
    def _range(self, table, lo, hi, who, max_links, cut=False, cuts=None, want_rows=True):
        """the body of count_range, range_rows and range_segments (cut=True, whatever `cuts` is then: _cut judges it): mfh_merkle_range_rows[_cut] with count,
        index, keys, status and rows allocated here.  Returns (rows or the list of row arrays, index, keys, status, count); rows are cut to the links written (none unless the status is 0)"""
        c = self._ctx
        tab, tstride, length = self._table(table, who)
        lo, hi = bytes(lo), bytes(hi)
        kb = len(lo)
        if len(hi) != kb or not 1 <= kb <= 32 or length < 2 * kb:
            raise MfhError(f"{who}: lo and hi are key_bytes bytes each, 1 <= key_bytes <= 32 and 2 key_bytes <= length")
        vp = ctypes.c_void_p
        a, b = np.frombuffer(lo, dtype=np.uint8), np.frombuffer(hi, dtype=np.uint8)
        count = ctypes.c_uint32(0)
        status = np.zeros(1, dtype=np.uint8)

        def call(m, index, keys, rows_args):
            fn = c.lib.mfh_merkle_range_rows_cut if cut else c.lib.mfh_merkle_range_rows
            c._chk(fn(c._h, self._h, _ptr(tab), tstride, length, kb, vp(a.ctypes.data), vp(b.ctypes.data), m, ctypes.byref(count),
                      vp(index.ctypes.data) if index is not None else None, vp(keys.ctypes.data) if keys is not None else None, *rows_args, vp(status.ctypes.data)))
            self._keep = []  # (the call waited for the stream)

        if max_links is None or not want_rows:  # the count query: flags and scan alone
            c._chk(c.lib.mfh_merkle_range_rows(c._h, self._h, _ptr(tab), tstride, length, kb, vp(a.ctypes.data), vp(b.ctypes.data), 0, ctypes.byref(count), None, None,
                                               None, 0, vp(status.ctypes.data)))
            self._keep = []
            if not want_rows:
                return None, None, None, int(status[0]), int(count.value)
            max_links = int(count.value)
        if not isinstance(max_links, (int, np.integer)) or max_links < 0 or max_links > 0xFFFFFFFF:
            raise MfhError(f"{who}: max_links is a number of links, or None to ask for the count first")
        m = int(max_links)
        index = np.zeros(m, dtype=np.uint32)
        keys = np.zeros((m, 2, kb), dtype=np.uint8)
        if not cut:
            rows = np.zeros((m, self._row_bytes(32, length)), dtype=np.uint8)
            call(m, index, keys, (vp(rows.ctypes.data), rows.shape[1]))
        else:
            rows, cargs, keep = self._cut(cuts, who, m, lambda c0: 32 + length + 32 * c0 + (c0 + 7) // 8, m, upper=64)
            call(m, index, keys, cargs)
        st, n = int(status[0]), int(count.value)
        wrote = n if st != 1 else 0  # index and keys
        nrows = n if st == 0 else 0
        rows = [r[:nrows] for r in rows] if cut else rows[:nrows]
        return rows, index[:wrote], keys[:wrote], st, n

    def count_range(self, table, lo, hi):
        """the number of links of the key range [lo, hi] of an INDEXED table (words.MerkleLink; words.MerkleAbsent has the data model): the live records with
        record.hi >= lo and record.lo <= hi -- in a well-formed table the members inside [lo, hi] plus one.  mfh_merkle_range_rows with max_links = 0: two
        launches that stream the table's keys once; waits for the stream.  table: under locate_keys' rules, only read.  lo, hi: key_bytes bytes each, lo <= hi,
        neither all-zero nor all-0xFF."""
        return self._range(table, lo, hi, "count_range", None, want_rows=False)[4]

    def range_rows(self, table, lo, hi, max_links=None):
        """(rows, index, keys, status): the links of the key range [lo, hi] in key order (mfh_merkle_range_rows; waits for the stream).  keys is np.uint8 [n, 2,
        key_bytes], link i's (lo, hi): with members k_1 < .. < k_n-1 inside the range, (p, k_1), (k_1, k_2), .., (k_n-1, s) -- keys[1:, 0] are exactly the
        members of the set inside [lo, hi].  index is np.uint32 [n], their slots; rows is np.uint8 [n, 32 + length + 32 depth + ceil(depth / 8)], row i the
        packed input row of words.MerkleLink(key_bytes, length, depth, reveal) of link i for any `reveal`.
        status 0: the links chain across the range.  1: more than max_links links; everything comes back empty (count_range says how many).  2: the selected
        records do not chain, the table is malformed; index and keys are given, no rows.  max_links = None asks for the count first (one more pass over the
        table's keys); at most 2^16 links a call.
        A present-key lookup is the range [k, k]: link 1 is (k, its successor), its row's record carries k's payload -- and link 0 publishes k's predecessor,
        link 1 its successor, to whoever gets the statements."""
        return self._range(table, lo, hi, "range_rows", max_links)[:4]

    def range_bits(self, table, lo, hi, max_links=None):
        """range_rows with the rows as np.uint8 [n, 256 + 8 length + 257 depth] of 0 / 1: what Context.circuit_assign(prog, bits) takes for
        words.MerkleLink(key_bytes, length, depth, reveal)"""
        rows, index, keys, status = self.range_rows(table, lo, hi, max_links)
        return self._unpack(rows, 32, int(table.shape[1])), index, keys, status

    def range_segments(self, table, lo, hi, cuts, max_links=None):
        """range_rows with the path cut at levels `cuts` (mfh_merkle_range_rows_cut).  Returns (rows, nodes, index, keys, status): rows and nodes as
        path_segments gives them, rows[0][i] being the packed input row of words.MerkleLink(key_bytes, length, c_0, reveal) of link i; a verifier builds segment
        0's statements with MerkleLink.chain_cut(nodes[:, 0], lo, hi, keys, shown) and link i's upper ones with MerkleClimb.chain(nodes[i]).  The published
        nodes reveal which subtrees hold the links' records."""
        rows, index, keys, status, _ = self._range(table, lo, hi, "range_segments", max_links, cut=True, cuts=cuts)
        return rows, self._climb_nodes(rows), index, keys, status

    def range_segment_bits(self, table, lo, hi, cuts, max_links=None):
        """range_segments with every segment's rows as 0 / 1 arrays"""
        rows, nodes, index, keys, status = self.range_segments(table, lo, hi, cuts, max_links)
        return self._climb_unpack(rows, cuts, 256 + 8 * int(table.shape[1])), nodes, index, keys, status

    # ---- removes: the inverse of insert_keys
    def remove_keys(self, table, keys, roots=False):
        """(rows, index): nk sequential key removes from an INDEXED table (words.MerkleAbsent has the data model) and this tree in one call
        (mfh_merkle_remove_keys; waits for the stream).  Remove j zeroes the live record whose own key is keys[j] (it becomes inert, as indexed_records leaves
        unused slots) and hands its hi to the live record whose hi was keys[j]; an earlier remove of the batch may have taken a neighbour already.  rows is
        np.uint8 [nk, 64 + key_bytes + 2 length + 64 depth + ceil(2 depth / 8)]: row j is the packed input row of words.MerkleRemove(key_bytes, length, depth)
        taken from table and tree as they stood before remove j.  index is np.uint32 [nk, 2]: (the slot whose hi changed, the slot that was zeroed).  With
        roots=True a triple whose last element is np.uint8 [nk + 1, 32], the roots R_0 .. R_nk: statement j is MerkleRemove.statement(R_j, R_j+1, keys[j]).
        table: under update_records' rules, MODIFIED IN PLACE.  keys: np.uint8 [nk, key_bytes] under locate_keys' rules, all different.  MfhError with the
        library's text, table and tree untouched, when a key is not a member or no live record has a member as its hi.  With all-zero inert slots,
        insert_keys of a batch followed by remove_keys of the same keys restores the table's bytes and the root."""
        return self._key_steps("remove_keys", "remove", table, keys, roots=roots)

    def remove_bits(self, table, keys, roots=False):
        """remove_keys with the rows as np.uint8 [nk, 512 + 8 key_bytes + 16 length + 514 depth] of 0 / 1: what Context.circuit_assign(prog, bits) takes for
        words.MerkleRemove(key_bytes, length, depth)"""
        return self._key_step_bits(self.remove_keys(table, keys, roots), self._step_head(table, keys, 2, 64))

    def remove_key_segments(self, table, keys, cuts):
        """remove_keys with the path cut at levels `cuts` (mfh_merkle_remove_keys_cut).  Returns (rows, nodes_p, nodes_s, index): rows[0][j] is the packed input
        row of words.MerkleRemove(key_bytes, length, c_0, joined=False) of remove j; rows[g], g >= 1, holds one words.MerkleSegment row per UPDATE, row 2 j that
        of p's update of remove j and row 2 j + 1 that of s's; nodes_p and nodes_s are np.uint8 [nk, G + 1, 2, 32], the published pairs of the two updates:
        segment 0's statement is statement(*nodes_p[j, 0], *nodes_s[j, 0], keys[j]), the upper ones MerkleSegment.chain(nodes_p[j]) and chain(nodes_s[j]), and
        nodes_p[j, G, 1] == nodes_s[j, G, 0] is the root between the two updates, which becomes public.  index as remove_keys gives it."""
        return self._key_steps("remove_key_segments", "remove", table, keys, cut=True, cuts=cuts)

    def remove_key_segment_bits(self, table, keys, cuts):
        """remove_key_segments with every segment's rows as 0 / 1 arrays"""
        out = self.remove_key_segments(table, keys, cuts)
        head = self._step_head(table, keys, 2, 128)
        return (self._cut_unpack(out[0], cuts, lambda c0: 8 * head + 514 * c0),) + tuple(out[1:])

    # ---- transfers: a ledger on the indexed table, a balance in the payload
    def transfer_keys(self, table, from_keys, to_keys, amounts, amount_bytes=8, roots=False):
        """(rows, index): nk sequential transfers between the accounts of an INDEXED table whose records carry a balance (words.MerkleTransfer has the data
        model: bytes [2 key_bytes, 2 key_bytes + amount_bytes) of a record, big-endian) and this tree in one call (mfh_merkle_transfer_keys; waits for the
        stream).  Transfer j takes amounts[j] from the record whose own key is from_keys[j] and adds it to the record whose own key is to_keys[j]; an account
        may occur in any number of steps and may spend what an earlier step of the batch delivered.  rows is np.uint8 [nk, 64 + 2 key_bytes + amount_bytes +
        2 length + 64 depth + ceil(2 depth / 8)]: row j is the packed input row of words.MerkleTransfer(key_bytes, length, depth, amount_bytes) taken from
        table and tree as they stood before transfer j.  index is np.uint32 [nk, 2]: (the sender's slot, the receiver's).  With roots=True a triple whose last
        element is np.uint8 [nk + 1, 32], the roots R_0 .. R_nk: statement j is MerkleTransfer.statement(R_j, R_j+1, from_keys[j], to_keys[j], amounts[j]).
        table: under update_records' rules, MODIFIED IN PLACE.  from_keys, to_keys: np.uint8 [nk, key_bytes] under locate_keys' rules, from_keys[j] !=
        to_keys[j].  amounts: nk integers below 2^(8 amount_bytes).  MfhError with the library's text, table and tree untouched, when a sender or a receiver
        is not a member, a step overdraws its sender or takes its receiver past 2^(8 amount_bytes) - 1."""
        return self._key_steps("transfer_keys", "transfer", table, from_keys, roots=roots, transfer=(to_keys, amounts, amount_bytes))

    def transfer_bits(self, table, from_keys, to_keys, amounts, amount_bytes=8, roots=False):
        """transfer_keys with the rows as np.uint8 [nk, 512 + 16 key_bytes + 8 amount_bytes + 16 length + 514 depth] of 0 / 1: what
        Context.circuit_assign(prog, bits) takes for words.MerkleTransfer(key_bytes, length, depth, amount_bytes)"""
        head = self._step_head(table, from_keys, 2, 64) + np.ascontiguousarray(from_keys).shape[1] + int(amount_bytes)
        return self._key_step_bits(self.transfer_keys(table, from_keys, to_keys, amounts, amount_bytes, roots), head)

    def transfer_key_segments(self, table, from_keys, to_keys, amounts, cuts, amount_bytes=8):
        """transfer_keys with the path cut at levels `cuts` (mfh_merkle_transfer_keys_cut).  Returns (rows, nodes_p, nodes_s, index): rows[0][j] is the packed
        input row of words.MerkleTransfer(key_bytes, length, c_0, amount_bytes, joined=False) of transfer j; rows[g], g >= 1, holds one words.MerkleSegment
        row per UPDATE, row 2 j that of p's update of transfer j and row 2 j + 1 that of s's; nodes_p and nodes_s are np.uint8 [nk, G + 1, 2, 32], the
        published pairs of the two updates: segment 0's statement is statement(*nodes_p[j, 0], *nodes_s[j, 0], from_keys[j], to_keys[j], amounts[j]), the
        upper ones MerkleSegment.chain(nodes_p[j]) and chain(nodes_s[j]), and nodes_p[j, G, 1] == nodes_s[j, G, 0] is the root between the two updates,
        which becomes public.  index as transfer_keys gives it."""
        return self._key_steps("transfer_key_segments", "transfer", table, from_keys, cut=True, cuts=cuts, transfer=(to_keys, amounts, amount_bytes))

    def transfer_key_segment_bits(self, table, from_keys, to_keys, amounts, cuts, amount_bytes=8):
        """transfer_key_segments with every segment's rows as 0 / 1 arrays"""
        out = self.transfer_key_segments(table, from_keys, to_keys, amounts, cuts, amount_bytes)
        head = self._step_head(table, from_keys, 2, 128) + np.ascontiguousarray(from_keys).shape[1] + int(amount_bytes)
        return (self._cut_unpack(out[0], cuts, lambda c0: 8 * head + 514 * c0),) + tuple(out[1:])

    # ---- one-record steps by key: deposits and withdrawals, writes
    def _record_step(self, who, name, table, nk, pub, args, roots, cut, cuts):
        """what _adjust and _write end with: mfh_merkle_<name>[_cut] with rows (`pub` bytes of public pieces in a row's head), index, status and roots allocated
        here.  table: what _keys made of it; args: the call's arguments between `length` and the rows, whose arrays stay alive in the caller"""
        c = self._ctx
        tab, tstride, length = table
        vp = ctypes.c_void_p
        head = 64 + pub + length
        if not cut:
            rows = np.zeros((nk, head + 32 * self.depth + (self.depth + 7) // 8), dtype=np.uint8)
            out = (vp(rows.ctypes.data), rows.shape[1])
        else:
            rows, out, keep = self._cut(cuts, who, nk, lambda c0: head + 32 * c0 + (c0 + 7) // 8, nk)
        r = np.zeros((nk + 1, 32), dtype=np.uint8) if roots or cut else None
        index = np.zeros(nk, dtype=np.uint32)
        status = np.zeros(nk, dtype=np.uint8)
        call = getattr(c.lib, f"mfh_merkle_{name}_cut" if cut else f"mfh_merkle_{name}")
        c._chk(call(c._h, self._h, _ptr(tab), tstride, length, *args, *out, vp(r.ctypes.data) if r is not None else None, vp(index.ctypes.data),
                    vp(status.ctypes.data)))
        if nk:
            self._keep = []  # (the call waited for the stream)
        elif r is not None:
            r[0] = np.frombuffer(self.root(), dtype=np.uint8)
        if not cut:
            return (rows, index, r) if roots else (rows, index)
        return rows, self._cut_nodes(rows, r), index

    # ---- deposits and withdrawals: what funds and drains the ledger, and its supply
    def _adjust(self, who, table, keys, amounts, sides, amount_bytes, roots=False, cut=False, cuts=None):
        """the body of adjust_keys and, with cut=True, adjust_key_segments: its argument checks, then _record_step"""
        tab, tstride, length, k = self._keys(table, keys, who)
        nk, kb = k.shape
        vp = ctypes.c_void_p
        ab = amount_bytes
        if not isinstance(ab, (int, np.integer)) or not 1 <= ab <= 8 or length < 2 * kb + ab:
            raise MfhError(f"{who}: 1 <= amount_bytes <= 8 and 2 key_bytes + amount_bytes <= length")
        try:
            values = [int(a) for a in amounts]
            dirs = [0] * nk if sides is None else [int(x) for x in sides]
        except (TypeError, ValueError):
            values = dirs = None
        if values is None or len(values) != nk or any(not 0 <= a < 1 << 64 for a in values):
            raise MfhError(f"{who}: amounts are nk integers in [0, 2^64), one a step")
        if len(dirs) != nk or any(x not in (0, 1) for x in dirs):
            raise MfhError(f"{who}: sides are nk values 0 (a deposit) or 1 (a withdrawal), one a step")
        amt = np.array(values, dtype=np.uint64).reshape(nk)
        side = np.array(dirs, dtype=np.uint8).reshape(nk)
        args = (kb, int(ab), nk, vp(k.ctypes.data), kb, vp(amt.ctypes.data), vp(side.ctypes.data) if sides is not None else None)
        return self._record_step(who, "adjust_keys", (tab, tstride, length), nk, kb + int(ab) + 1, args, roots, cut, cuts)

    def adjust_keys(self, table, keys, amounts, sides=None, amount_bytes=8, roots=False):
        """(rows, index): nk sequential DEPOSITS and WITHDRAWALS on the accounts of an INDEXED table whose records carry a balance (words.MerkleTransfer has the
        data model: bytes [2 key_bytes, 2 key_bytes + amount_bytes) of a record, big-endian) and this tree in one call (mfh_merkle_adjust_keys; waits for the
        stream).  Step j adds amounts[j] to the balance of the record whose own key is keys[j] (sides[j] = 0, a deposit) or takes it off (sides[j] = 1, a
        withdrawal); sides=None: all deposits.  An account may occur in any number of steps, and a withdrawal may spend what an earlier deposit of the batch
        delivered.  rows is np.uint8 [nk, 64 + key_bytes + amount_bytes + 1 + length + 32 depth + ceil(depth / 8)]: row j is the packed input row of
        words.MerkleAdjust(key_bytes, length, depth, amount_bytes) taken from table and tree as they stood before step j.  index is np.uint32 [nk]: the
        account's slot.  With roots=True a triple whose last element is np.uint8 [nk + 1, 32], the roots R_0 .. R_nk: statement j is
        MerkleAdjust.statement(R_j, R_j+1, keys[j], amounts[j], sides[j]).
        table: under update_records' rules, MODIFIED IN PLACE.  keys: np.uint8 [nk, key_bytes] under locate_keys' rules, repeats allowed.  amounts: nk integers
        below 2^(8 amount_bytes).  MfhError with the library's text, table and tree untouched, when a key is not a member, a withdrawal overdraws its account
        or a deposit takes it past 2^(8 amount_bytes) - 1."""
        return self._adjust("adjust_keys", table, keys, amounts, sides, amount_bytes, roots)

    def adjust_bits(self, table, keys, amounts, sides=None, amount_bytes=8, roots=False):
        """adjust_keys with the rows as np.uint8 [nk, 512 + 8 (key_bytes + amount_bytes + 1) + 8 length + 257 depth] of 0 / 1: what
        Context.circuit_assign(prog, bits) takes for words.MerkleAdjust(key_bytes, length, depth, amount_bytes)"""
        out = self.adjust_keys(table, keys, amounts, sides, amount_bytes, roots)
        head = np.ascontiguousarray(keys).shape[1] + int(amount_bytes) + 1 + int(table.shape[1])
        return (self._unpack(out[0], 64, head),) + tuple(out[1:])

    def adjust_key_segments(self, table, keys, amounts, cuts, sides=None, amount_bytes=8):
        """adjust_keys with the path cut at levels `cuts` (mfh_merkle_adjust_keys_cut).  Returns (rows, nodes, index), rows and nodes shaped as
        update_record_segments returns them: rows[0][j] is the packed input row of words.MerkleAdjust(key_bytes, length, c_0, amount_bytes) of step j --
        the statement itself over the subtree of height c_0, it has one pair of tops -- and rows[g][j], g >= 1, that of words.MerkleSegment(c_g - c_g-1);
        nodes is np.uint8 [nk, G + 1, 2, 32], the published pairs of every step, (X_G, X_G') = (R_j, R_j+1): segment 0's statement is
        MerkleAdjust.statement(*nodes[j, 0], keys[j], amounts[j], sides[j]), the upper ones MerkleSegment.chain(nodes[j]).  index as adjust_keys gives it."""
        return self._adjust("adjust_key_segments", table, keys, amounts, sides, amount_bytes, cut=True, cuts=cuts)

    def adjust_key_segment_bits(self, table, keys, amounts, cuts, sides=None, amount_bytes=8):
        """adjust_key_segments with every segment's rows as 0 / 1 arrays"""
        out = self.adjust_key_segments(table, keys, amounts, cuts, sides, amount_bytes)
        head = 64 + np.ascontiguousarray(keys).shape[1] + int(amount_bytes) + 1 + int(table.shape[1])
        return (self._cut_unpack(out[0], cuts, lambda c0: 8 * head + 257 * c0),) + tuple(out[1:])

    # ---- writes by key, plain and compare-and-set: the put of the keyed store
    @staticmethod
    def _field_values(who, what, values, nk, F):
        """np.uint8 [nk, F], contiguous: an array of that shape, or nk bytes-likes of F bytes"""
        try:
            if isinstance(values, np.ndarray):
                v = values
            else:
                items = [bytes(x) for x in values]
                v = np.frombuffer(b"".join(items), dtype=np.uint8).reshape(len(items), F) if all(len(x) == F for x in items) else None
        except (TypeError, ValueError):
            v = None
        if v is None or v.dtype != np.uint8 or v.shape != (nk, F):
            raise MfhError(f"{who}: {what} are np.uint8 [nk, hi - lo] or nk bytes-likes of hi - lo bytes, one a step")
        return np.ascontiguousarray(v)

    def _write(self, who, table, keys, values, field, expect, roots=False, cut=False, cuts=None):
        """the body of write_keys and, with cut=True, write_key_segments: its argument checks, then _record_step"""
        tab, tstride, length, k = self._keys(table, keys, who)
        nk, kb = k.shape
        vp = ctypes.c_void_p
        try:
            lo, hi = field
        except (TypeError, ValueError):
            lo = hi = None
        if not all(isinstance(x, (int, np.integer)) for x in (lo, hi)) or not 2 * kb <= lo < hi <= length:
            raise MfhError(f"{who}: the field is (lo, hi) with 2 key_bytes <= lo < hi <= length")
        lo, hi = int(lo), int(hi)
        F = hi - lo
        val = self._field_values(who, "values", values, nk, F)
        exp = None if expect is None else self._field_values(who, "expectations", expect, nk, F)
        args = (kb, lo, hi, nk, vp(k.ctypes.data), kb, vp(val.ctypes.data), F, vp(exp.ctypes.data) if exp is not None else None, F)
        return self._record_step(who, "write_keys", (tab, tstride, length), nk, kb + (F if exp is None else 2 * F), args, roots, cut, cuts)

    def write_keys(self, table, keys, values, field, expect=None, roots=False):
        """(rows, index): nk sequential WRITES BY KEY on an INDEXED table and this tree in one call (mfh_merkle_write_keys; waits for the stream).  Step j sets
        bytes [lo, hi) = field of the record whose own key is keys[j] to values[j]; with `expect` only if those bytes are expect[j] at that step (compare-and-
        set), else the whole call is refused.  A key may occur in any number of steps, and a step sees what the earlier steps left: an expectation may be one
        that only an earlier write of the batch satisfies.  rows is np.uint8 [nk, 64 + key_bytes + F (2 F with expect) + length + 32 depth + ceil(depth / 8)],
        F = hi - lo: row j is the packed input row of words.MerkleWrite(key_bytes, length, depth, field, expect is not None) taken from table and tree as they
        stood before step j.  index is np.uint32 [nk]: the record's slot.  With roots=True a triple whose last element is np.uint8 [nk + 1, 32], the roots R_0 ..
        R_nk: statement j is MerkleWrite.statement(R_j, R_j+1, keys[j], [expect[j],] values[j]).
        table: under update_records' rules, MODIFIED IN PLACE.  keys: np.uint8 [nk, key_bytes] under locate_keys' rules, repeats allowed.  values, expect:
        np.uint8 [nk, F] or nk bytes-likes of F bytes.  field: 2 key_bytes <= lo < hi <= length, the keys are never writable.  MfhError with the library's text,
        table and tree untouched, when a key is not a member or a field is not what was expected at its step."""
        return self._write("write_keys", table, keys, values, field, expect, roots)

    def write_bits(self, table, keys, values, field, expect=None, roots=False):
        """write_keys with the rows as np.uint8 [nk, 512 + 8 (key_bytes + F [+ F]) + 8 length + 257 depth] of 0 / 1: what Context.circuit_assign(prog, bits)
        takes for words.MerkleWrite(key_bytes, length, depth, field, expect is not None)"""
        out = self.write_keys(table, keys, values, field, expect, roots)
        head = out[0].shape[1] - 64 - 32 * self.depth - (self.depth + 7) // 8
        return (self._unpack(out[0], 64, head),) + tuple(out[1:])

    def write_key_segments(self, table, keys, values, field, cuts, expect=None):
        """write_keys with the path cut at levels `cuts` (mfh_merkle_write_keys_cut).  Returns (rows, nodes, index), rows and nodes shaped as
        update_record_segments returns them: rows[0][j] is the packed input row of words.MerkleWrite(key_bytes, length, c_0, field, expect is not None) of
        step j -- the statement itself over the subtree of height c_0, it has one pair of tops -- and rows[g][j], g >= 1, that of words.MerkleSegment(c_g -
        c_g-1); nodes is np.uint8 [nk, G + 1, 2, 32], the published pairs of every step, (X_G, X_G') = (R_j, R_j+1): segment 0's statement is
        MerkleWrite.statement(*nodes[j, 0], keys[j], [expect[j],] values[j]), the upper ones MerkleSegment.chain(nodes[j]).  index as write_keys gives it."""
        return self._write("write_key_segments", table, keys, values, field, expect, cut=True, cuts=cuts)

    def write_key_segment_bits(self, table, keys, values, field, cuts, expect=None):
        """write_key_segments with every segment's rows as 0 / 1 arrays"""
        out = self.write_key_segments(table, keys, values, field, cuts, expect)
        lo, hi = field
        head = 64 + np.ascontiguousarray(keys).shape[1] + (1 if expect is None else 2) * (int(hi) - int(lo)) + int(table.shape[1])
        return (self._cut_unpack(out[0], cuts, lambda c0: 8 * head + 257 * c0),) + tuple(out[1:])

    # ---- blocks: transfers, adjusts and writes in any order in one call
    def _block(self, who, table, block, skip_failed, cut=False, cuts=None):
        """the body of apply_block and, with cut=True, apply_block_segments: the argument checks, the block's arrays, mfh_merkle_block_keys[_cut]"""
        from .words import Block

        c = self._ctx
        vp = ctypes.c_void_p
        tab, tstride, length = self._table(table, who)
        if not isinstance(block, Block):
            raise MfhError(f"{who}: the block is a words.Block")
        K, A, nk = block.key_bytes, block.amount_bytes, len(block)
        if length < 2 * K + A:
            raise MfhError(f"{who}: 2 key_bytes + amount_bytes <= length")
        col = block.columns()  # (made once a block, in one pass over its steps)
        if col["field_hi"] > length:
            raise MfhError(f"{who}: a write's field is (lo, hi) with 2 key_bytes <= lo < hi <= length")
        kinds, keys, keys_to, amounts, sides, fields = (col[x] for x in ("kinds", "keys", "keys_to", "amounts", "sides", "fields"))
        value_at, expect_at, values, expect = (col[x] for x in ("value_at", "expect_at", "values", "expect"))
        if cut:
            rows_g, cut_args, keep = self._cut(cuts, who, 0, lambda c0: 0, col["updates"])
            d0 = int(keep[0])
        else:
            d0 = self.depth
        # every step's row bytes (csrc/merkle_rows.hpp; mfh_merkle_block_row_bytes says the same of one step), by kind
        one = 64 + K + length + 32 * d0 + (d0 + 7) // 8
        written = (fields[:, 1] - fields[:, 0]).astype(np.uint64) * np.where(expect_at != 0xFFFFFFFFFFFFFFFF, 2, 1).astype(np.uint64)
        rowb = np.where(kinds == Block.TRANSFER, (128 if cut else 64) + 2 * K + A + 2 * length + 64 * d0 + (2 * d0 + 7) // 8,
                        np.where(kinds == Block.ADJUST, one + A + 1, one + written)).astype(np.uint64)
        row_at = np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(rowb, dtype=np.uint64)])
        buf = np.zeros(int(row_at[-1]) or 1, dtype=np.uint8)
        r_all = np.zeros((2 * nk + 1, 32), dtype=np.uint8)
        index = np.full((nk, 2), 0xFFFFFFFF, dtype=np.uint32)
        status = np.zeros(nk, dtype=np.uint8)
        first_update = np.zeros(nk + 1, dtype=np.uint32)
        args = (c._h, self._h, _ptr(tab), tstride, length, K, A, nk, vp(kinds.ctypes.data), vp(keys.ctypes.data), vp(keys_to.ctypes.data), K, vp(amounts.ctypes.data),
                vp(sides.ctypes.data), vp(fields.ctypes.data), vp(value_at.ctypes.data), vp(values.ctypes.data), col["values_bytes"], vp(expect_at.ctypes.data),
                vp(expect.ctypes.data), col["expect_bytes"], int(bool(skip_failed)))
        outs = (vp(row_at.ctypes.data), vp(r_all.ctypes.data), vp(index.ctypes.data), vp(status.ctypes.data), vp(first_update.ctypes.data))
        try:
            if cut:
                rows_g[0] = buf.reshape(1, -1)
                ncuts, h_cuts, _, _ = cut_args
                ptrs = (vp * len(rows_g))(*[r.ctypes.data for r in rows_g])
                strides = (ctypes.c_size_t * len(rows_g))(*[r.shape[1] for r in rows_g])
                c._chk(c.lib.mfh_merkle_block_keys_cut(*args, ncuts, h_cuts, ptrs, strides, *outs))
            else:
                c._chk(c.lib.mfh_merkle_block_keys(*args, vp(buf.ctypes.data), *outs))
        except MfhError as e:
            e.status, e.index = status, index  # (filled when the refusal came behind the search)
            raise
        if nk:
            self._keep = []  # (the call waited for the stream)
        else:
            r_all[0] = np.frombuffer(self.root(), dtype=np.uint8)
        res = BlockResult(self, block, length, d0, cut, buf, row_at, index, status, r_all, first_update)
        if cut:
            nupd = int(first_update[nk])
            res.segments = [r[:nupd] for r in rows_g[1:]]
            res.nodes = self._cut_nodes([None] + res.segments, r_all[: nupd + 1])
        return res

    def apply_block(self, table, block, skip_failed=False):
        """a BlockResult: the steps of a words.Block -- transfers, adjusts and writes in any order -- applied in order to an INDEXED table whose records
        carry a balance and to this tree in ONE call (mfh_merkle_block_keys: one search, one build launch; waits for the stream).  Byte for byte what
        transfer_keys, adjust_keys and write_keys give when run once per step: result.rows[j] is step j's packed input row, that of its kind's statement,
        taken from table and tree as they stood before step j; result.index is np.uint32 [nk, 2], (the sender's slot, the receiver's) or (the slot,
        0xFFFFFFFF); result.status np.uint8 [nk]; result.roots np.uint8 [nk + 1, 32], R_0 .. R_nk: block.statements(length, depth, result.roots,
        result.status) are the statements.  table: under update_records' rules, MODIFIED IN PLACE.
        skip_failed=False: MfhError with the library's text, table and tree untouched, when any step has a status -- 1 the key (a sender) is no member, 2 a
        receiver is none, 3 an overdraft and 4 an overflow of the running balance, 5 the running field is not what the step expects; the error carries
        .status and .index.  skip_failed=True: the steps with a status are left out (no row: result.rows[j] is None; R_j+1 = R_j) and the rest applied as
        if the block had been given without them."""
        return self._block("apply_block", table, block, skip_failed)

    def apply_block_segments(self, table, block, cuts, skip_failed=False):
        """apply_block with the path cut at levels `cuts` (mfh_merkle_block_keys_cut).  result.rows[j] is step j's segment-0 row -- that of
        words.MerkleTransfer(.., c_0, joined=False), or MerkleAdjust / MerkleWrite at depth c_0; result.segments[g - 1] is np.uint8 [nupd, ..], one
        words.MerkleSegment row per UPDATE for the level range g >= 1; result.nodes np.uint8 [nupd, G + 1, 2, 32], the published pairs of every update;
        result.first_update np.uint32 [nk + 1]: step j's updates are [first_update[j], first_update[j + 1]), two of a transfer, none of a skipped step."""
        return self._block("apply_block_segments", table, block, skip_failed, cut=True, cuts=cuts)

    def total_balance(self, table, key_bytes, amount_bytes=8):
        """(sum, live): the SUPPLY of an indexed table whose records carry a balance -- the sum, a Python int, of the balances (bytes [2 key_bytes, 2 key_bytes
        + amount_bytes), big-endian) of all live records (lo < hi), and their number (mfh_merkle_balance_sum: two launches, a 128-bit sum, no atomics; waits
        for the stream).  What stands in the balance bytes of a slot that is not live does not count.  transfer_keys leaves the sum as it is; adjust_keys
        changes it by the batch's deposits less its withdrawals.  table: under update_records' rules, only read."""
        c = self._ctx
        who = "total_balance"
        tab, tstride, length = self._table(table, who)
        if not all(isinstance(x, (int, np.integer)) for x in (key_bytes, amount_bytes)) or not 1 <= key_bytes <= 32 or not 1 <= amount_bytes <= 8 \
                or length < 2 * key_bytes + amount_bytes:
            raise MfhError(f"{who}: 1 <= key_bytes <= 32, 1 <= amount_bytes <= 8 and 2 key_bytes + amount_bytes <= length")
        total = (ctypes.c_uint64 * 2)()
        live = ctypes.c_uint32()
        c._chk(c.lib.mfh_merkle_balance_sum(c._h, self._h, _ptr(tab), tstride, length, int(key_bytes), int(amount_bytes), total, ctypes.byref(live)))
        self._keep = []
        return int(total[0]) | int(total[1]) << 64, int(live.value)

    def _packed(self, what, who, name, none_ok=False, pad=False):
        """(tensor or None, n, width) of the packed keys or payloads of load_keys: a contiguous uint8 [n, width] device tensor taken as it is, or a host array / list
        uploaded (words._keys_array parses keys; pad=True: a list of payloads, zero-padded to the longest)"""
        from .words import CircuitError, _keys_array

        c = self._ctx
        if what is None and none_ok:
            return None, None, 0
        if isinstance(what, c.torch.Tensor):
            if what.dtype != c.torch.uint8 or what.device != c.device or what.dim() != 2 or not what.is_contiguous():
                raise MfhError(f"{who}: a device tensor of {name} is contiguous uint8 [n, width] on the context's device")
            return what, int(what.shape[0]), int(what.shape[1])
        if pad and not isinstance(what, np.ndarray):
            items = [bytes(p) for p in what]
            width = max((len(p) for p in items), default=0)
            a = np.zeros((len(items), width), dtype=np.uint8)
            for i, p in enumerate(items):
                a[i, : len(p)] = np.frombuffer(p, dtype=np.uint8)
        elif pad:
            a = np.ascontiguousarray(what)
            if a.dtype != np.uint8 or a.ndim != 2:
                raise CircuitError(f"{who}: payloads are uint8 [n, payload_bytes]")
        else:
            a = np.ascontiguousarray(_keys_array(what, who))
        n, width = a.shape
        return (c.to_device(a) if a.size else None), n, width

    def load_keys(self, table, keys, payloads=None):
        """(status, where): the WHOLE indexed table of the set `keys` and this tree, built on the device (mfh_merkle_load_keys: a device sort of the keys, one
        launch that writes every record, the tree as set_records(0, table) makes it; waits for the stream once, for the status).  On status 0 (where = None)
        the table holds the bytes of words.indexed_records(keys, depth, length, payloads).  Status 2, where = the lowest index of a key that is all-zero or
        all-0xFF; status 1, where = (i, j), the two lowest indices of the smallest key given twice; with either NOTHING of table or tree is written.
        table: under update_records' rules, MODIFIED IN PLACE (bytes behind `length` in a wider stride stay).  keys: np.uint8 [n, key_bytes] or a list of
        bytes-likes of one length (words._keys_array), in any order, uploaded; or a contiguous torch uint8 [n, key_bytes] tensor on the context's device, taken
        as it is.  payloads: None (all zero), np.uint8 [n, payload_bytes], a list of bytes-likes (zero-padded to the longest), or a device tensor, in the
        order of the keys.  CircuitError / MfhError with the library's text for more than 2^depth - 1 keys, key_bytes outside [1, 32] or 2 key_bytes +
        payload_bytes > length."""
        c = self._ctx
        who = "load_keys"
        tab, tstride, length = self._table(table, who)
        k, nk, kb = self._packed(keys, who, "keys")
        pay, npay, pb = self._packed(payloads, who, "payloads", none_ok=True, pad=True)
        if pay is None or pb == 0:
            pay, pb = None, 0  # (no payload bytes at all is no payload)
        elif npay != nk:
            raise MfhError(f"{who}: one payload per key, in the order of the keys")
        status = (ctypes.c_uint32 * 3)()
        c._chk(c.lib.mfh_merkle_load_keys(c._h, self._h, _ptr(tab), tstride, length, kb, nk, _ptr(k), _ptr(pay), pb, status))
        if nk:
            self._keep = []  # (the call waited for the stream)
        else:
            self._keep += [x for x in (k, pay) if x is not None]
        st = int(status[0])
        return st, (None if st == 0 else int(status[1]) if st == 2 else (int(status[1]), int(status[2])))

    def check_table(self, table, key_bytes):
        """(status, live, where): does the indexed table still have the invariant every key statement is sound relative to, and does this tree belong to it
        (mfh_merkle_check_table: only reads; waits for the stream)?  live = the number of live records.  Status 0 (where = None): all good.  1: the chain of
        the live records sorted by (lo, slot) breaks, where = the slot words.indexed_check reports (0xFFFFFFFF without any live record).  2: where = the lowest
        slot whose record does not hash to its leaf.  3: where = (level, index) of the lowest wrong inner node, the leaves' parents being level 1.  A defect of
        a lower status hides those of a higher one.  table: under update_records' rules, only read."""
        c = self._ctx
        who = "check_table"
        tab, tstride, length = self._table(table, who)
        if not isinstance(key_bytes, (int, np.integer)) or not 1 <= key_bytes <= 32 or length < 2 * key_bytes:
            raise MfhError(f"{who}: 1 <= key_bytes <= 32 and 2 key_bytes <= length")
        out = (ctypes.c_uint32 * 4)()
        c._chk(c.lib.mfh_merkle_check_table(c._h, self._h, _ptr(tab), tstride, length, int(key_bytes), out))
        self._keep = []
        st = int(out[0])
        return st, int(out[1]), (None if st == 0 else (int(out[2]), int(out[3])) if st == 3 else int(out[2]))

    def grow(self, new_depth, table=None, length=None, out=None, roots=False):
        """a NEW MerkleTree of new_depth > depth whose leftmost subtree is this tree and whose other leaves are all inert, and with `table` the grown table
        (mfh_merkle_grow, mfh_merkle_grow_leaves: copies, constants and new_depth - depth compressions -- no record is hashed and no level rebuilt).  This
        tree and `table` are only read and stay valid.  The new root is words.grown_root(root, depth, new_depth, length): a public function of the old one.
        table: the table of this tree under update_records' rules; the result is then (tree, new_table), new_table a uint8 [2^new_depth, length] tensor
        holding words.indexed_grow(table, new_depth): the old records, then all-zero (inert) ones.  out: that tensor preallocated, uint8 [2^new_depth, >=
        length] under the same rules (a wider stride, a column slice of a wider table; bytes behind `length` stay as they were); it must not overlap
        `table`.  Without `out` a contiguous one is allocated.
        table=None, length=L: the tree of L-byte records alone, for a table kept elsewhere.  Neither: a tree of leaves (set_leaves; the inert leaf is 32
        zero bytes).  roots=True appends (R, R'), the old and the new root as bytes, to the result, and waits for the stream once; without it the call only
        queues work on the context's stream."""
        c = self._ctx
        who = "grow"
        if not isinstance(new_depth, (int, np.integer)):
            raise MfhError(f"{who}: new_depth is an integer")
        new_depth = int(new_depth)
        h = ctypes.c_void_p()
        r = (ctypes.c_uint8 * 64)() if roots else None
        new = None
        if table is None and length is None:
            if out is not None:
                raise MfhError(f"{who}: out goes with a table")
            c._chk(c.lib.mfh_merkle_grow_leaves(c._h, self._h, new_depth, ctypes.byref(h), r))
        elif table is None:
            if out is not None:
                raise MfhError(f"{who}: out goes with a table")
            if not isinstance(length, (int, np.integer)) or length < 0:
                raise MfhError(f"{who}: length is the records' length in bytes")
            c._chk(c.lib.mfh_merkle_grow(c._h, self._h, new_depth, None, 0, int(length), None, 0, ctypes.byref(h), r))
        else:
            tab, tstride, tlength = self._table(table, who)
            if length is not None and length != tlength:
                raise MfhError(f"{who}: length is the table's")
            if not self.depth < new_depth <= 24:
                raise MfhError(f"{who}: new_depth must be above the tree's depth and at most 24")
            if out is None:
                new, nstride = c.empty((tlength << new_depth)).reshape(1 << new_depth, tlength), tlength
            else:
                wide, nstride, olength, nrec, _ = _records(c, out, who) if isinstance(out, c.torch.Tensor) else (None, 0, 0, 0, False)
                if wide is None or nrec != 1 << new_depth or olength < tlength:
                    raise MfhError(f"{who}: out is a torch uint8 [2^new_depth, >= length] tensor on the context's device")
                new = wide[:, :tlength]
            c._chk(c.lib.mfh_merkle_grow(c._h, self._h, new_depth, _ptr(tab), tstride, tlength, _ptr(new), nstride, ctypes.byref(h), r))
        if roots:
            self._keep = []  # (the call waited for the stream)
        tree = MerkleTree(c, new_depth, h)
        res = (tree,) + ((new,) if table is not None else ()) + (((bytes(r[:32]), bytes(r[32:])),) if roots else ())
        return res[0] if len(res) == 1 else res


class Context:
    """One prover context on one GPU (one process per GPU).  Mirrors the reference's implicit global state:
    an `rng_t` seeded from the CRS seed (src/snark.c:59,119) plus the parameter macros.
    own_stream=True keeps the library on the non-blocking stream the context creates for itself (what a C caller gets who never calls mfh_set_stream):
    nothing then orders its work against torch's streams but sync() and the caller's own waits."""

    def __init__(self, params: Params = DEFAULT, device: int = 0, own_stream: bool = False):
        import torch

        if not torch.cuda.is_available():
            raise MfhError("no HIP device visible: the MI355X path has no CPU fallback")
        self.torch = torch
        self.lib = load_library()
        self.params = params
        self.device = torch.device("cuda", device)
        self._h = ctypes.c_void_p()
        cp = _CParams(params.n, params.logq, params.d, params.m)
        rc = self.lib.mfh_ctx_create(ctypes.byref(self._h), device, ctypes.byref(cp))
        if rc != 0:
            raise MfhError(f"mfh_ctx_create failed ({rc})")
        if not own_stream:
            # run on torch's current stream so torch allocations/copies and our kernels are ordered
            self.set_stream(torch.cuda.current_stream(self.device))

    def close(self):
        if self._h:
            self.lib.mfh_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            raise MfhError(f"libmfhip error {rc}: {self.lib.mfh_last_error(self._h).decode()}")

    # -- helpers ---------------------------------------------------------------------------------------
    def empty(self, nbytes):
        return self.torch.empty(int(nbytes), dtype=self.torch.uint8, device=self.device)

    def zeros(self, nbytes):
        return self.torch.zeros(int(nbytes), dtype=self.torch.uint8, device=self.device)

    def to_device(self, arr):
        a = np.ascontiguousarray(arr)
        if not a.flags.writeable:  # read-only file mappings (files.crs_map): the host tensor is only a copy source
            import warnings

            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)
                return self.torch.from_numpy(a.view(np.uint8).reshape(-1)).to(self.device)
        return self.torch.from_numpy(a.view(np.uint8).reshape(-1)).to(self.device)

    def to_host(self, t, dtype=np.uint8):
        return t.cpu().numpy().view(dtype)

    def sync(self):
        self._chk(self.lib.mfh_sync(self._h))

    def set_stream(self, stream):
        """run the calls that follow on `stream` (mfh_set_stream): a torch.cuda.Stream, or None for HIP's null stream.  The caller waits for the context's
        work (sync()) before it switches; sample_rows alone may be followed by a switch at once (include/mfhip.h)."""
        self._chk(self.lib.mfh_set_stream(self._h, ctypes.c_void_p(stream.cuda_stream if stream is not None else 0)))

    def scrub_staging(self):
        """wait for the copies out of the context's pinned staging (witness bits, deltas, smudging terms) and zero it (mfh_scrub_staging); returns 0"""
        rc = self.lib.mfh_scrub_staging(self._h)
        self._chk(rc)
        return rc

    def workspace_bytes(self):
        """capacity of the context's main device workspace in bytes (mfh_workspace_bytes): grow-only, in 1 MiB steps"""
        return int(self.lib.mfh_workspace_bytes(self._h))

    def set_timing(self, on=True):
        self._chk(self.lib.mfh_set_timing(self._h, 1 if on else 0))

    def set_overlap(self, mode=1):
        """0 = one stream, 1 = two streams with the queueing order picked automatically, 2 = b_w first, 3 = chain first"""
        self._chk(self.lib.mfh_set_overlap(self._h, int(mode)))

    def set_batch_image(self, on=True):
        """prove_batch with more than 31 proofs: expand the CRS once per call into a transient image and stream it per group (default) or not"""
        self._chk(self.lib.mfh_set_batch_image(self._h, 1 if on else 0))

    def set_batch_slabs(self, nslabs=0):
        """prove_batch: 0 = row slabs only when the image does not fit HBM, n = always n slabs (each expanded once and streamed for every group)"""
        self._chk(self.lib.mfh_set_batch_slabs(self._h, int(nslabs)))

    def set_expand_path(self, path=0):
        """crs_expand_mm*: 0 = barrier-free writer (MFMA transposition), 1 = LDS-tile writer"""
        self._chk(self.lib.mfh_set_expand_path(self._h, int(path)))

    def set_expand_periods(self, periods=0):
        """barrier-free writer of crs_expand_mm* and of prove_batch's transient image: periods of 23 AES blocks per chunk, 0 = picked from the row count, 2 .. 10 forced (tests:
        the image does not depend on it)"""
        if not 0 <= int(periods) <= 0xFFFFFFFF:
            raise MfhError("set_expand_periods: 0 or 2 .. 10")
        self._chk(self.lib.mfh_set_expand_periods(self._h, int(periods)))

    def set_encrypt_path(self, path=0):
        """encrypt_rows / setup: 0 = by batch size, 1 = VALU kernel, 2 = matrix-core kernel (<sk, a> as a Toeplitz int8 GEMM)"""
        self._chk(self.lib.mfh_set_encrypt_path(self._h, int(path)))

    def set_eval_path(self, path=0):
        """eval_rows / prove: 0 = tile kernel (k_eval, default), 1 = wave-autonomous kernel (k_eval_w, logq 736; measured 4 % slower)"""
        self._chk(self.lib.mfh_set_eval_path(self._h, int(path)))

    def set_encrypt_chunks(self, chunks=0):
        """k_encrypt_mm: column chunks per row (0 = picked from the batch size)"""
        self._chk(self.lib.mfh_set_encrypt_chunks(self._h, int(chunks)))

    def set_witness_per(self, statements=0):
        """statements per witness GEMM pass of the batch chain (0 = one pass per super-group of up to 255)"""
        self._chk(self.lib.mfh_set_witness_per(self._h, int(statements)))

    def set_batch_launch(self, groups_per_launch=4, merge_regions=True):
        """streaming regime of prove_batch: groups of 31 proofs per pass over a region's image; S and AS groups in one launch or two"""
        self._chk(self.lib.mfh_set_batch_launch(self._h, int(groups_per_launch), 1 if merge_regions else 0))

    def set_batch_bw(self, merged=True):
        """b_w of all super-groups of a call in one streaming launch per 8 of them (default) or one launch per super-group"""
        self._chk(self.lib.mfh_set_batch_bw(self._h, 1 if merged else 0))

    def set_batch_witness(self, streamed=True):
        """the witness pass of a streaming prove_batch call as one streaming launch over the SSP image (default) or k_witness_mm8q per super-group"""
        self._chk(self.lib.mfh_set_batch_witness(self._h, 1 if streamed else 0))

    def set_mm_stream(self, map=0, persistent=False, sync_mode=0, spin_max=64):
        """layout of a streaming launch with several groups: slot map (0 | 1), persistent one-workgroup-per-CU grid, rendezvous of the sharers (0 | 1 | 2)"""
        self._chk(self.lib.mfh_set_mm_stream(self._h, int(map), int(persistent), int(sync_mode), int(spin_max)))

    def set_mm_width(self, per_xcd=32, early_chain=False):
        """workgroups per XCD of the persistent S / AS launch (32 = every CU); early_chain: chain / epilogues queued beside the streaming launches"""
        self._chk(self.lib.mfh_set_mm_width(self._h, int(per_xcd), 1 if early_chain else 0))

    def set_mm_queue(self, mode=1, start_shift=0, prefix=-8):
        """persistent grid: 0 = every workgroup walks its fixed list of items, 1 = workgroups claim items from per-XCD queues and steal from the other XCDs' at the end.
        prefix: rounds of the fixed list run before the first claim (< 0: all but the last -prefix); start_shift (tests): begin in the queue of XCD x + start_shift"""
        self._chk(self.lib.mfh_set_mm_queue(self._h, int(mode), int(start_shift), int(prefix)))

    def set_mm_claim_log(self, log):
        """tests: a zeroed uint32 device tensor in which the persistent launches of the following calls record who ran which item; None: no log"""
        if log is None:
            self._chk(self.lib.mfh_set_mm_claim_log(self._h, None, 0))
        else:
            self._chk(self.lib.mfh_set_mm_claim_log(self._h, log.data_ptr(), log.numel()))

    def mm_claim_log_launches(self):
        """one dict per persistent launch recorded in the claim log since set_mm_claim_log: where its section starts and the shape that indexes it"""
        out = (ctypes.c_uint32 * (16 * 12))()
        n = int(self.lib.mfh_mm_claim_log_launches(self._h, out, 16))
        keys = ("offset", "nchunks", "nblk", "ngt", "ngr", "map", "tgs", "width", "coeff_bytes", "queue", "prefix", "shift")
        return [dict(zip(keys, (int(x) for x in out[12 * i:12 * i + 12]))) for i in range(n)]

    def set_mm_pack(self, on=True):
        """streaming kernels hand their partial products to the epilogue recombined (default) or as int32 (rounds 1 - 5): same results"""
        self._chk(self.lib.mfh_set_mm_pack(self._h, 1 if on else 0))

    def set_poly_exact(self, mode=1):
        """batches of h = (v^2 - 1) / t try the exact-division path (two cyclic products of half the length, checked on the device) before Euclidean division: same results.
        0 / False: never; 1 / True: unless a recent batch failed the check (64 batches of Euclidean division alone follow); 2: always"""
        self._chk(self.lib.mfh_set_poly_exact(self._h, int(mode)))

    def poly_exact_fallbacks(self):
        """statements whose exact-division result failed the device check since the last call (they were recomputed by Euclidean division); -1: no exact path for this t"""
        return int(self.lib.mfh_poly_exact_fallbacks(self._h))

    def exact_points(self):
        """the four points at which the exact-division path checks h(r) t(r) = v(r)^2 - 1 for the prepared t (drawn per preparation unless pinned)"""
        out = (ctypes.c_uint32 * 4)()
        self._chk(self.lib.mfh_poly_exact_points(self._h, out))
        return [int(x) for x in out]

    def set_exact_points(self, pts):
        """pin those points from the next poly_prepare_t on: four distinct values in [2, p - 1); None: draw them per preparation again"""
        if pts is None:
            self._chk(self.lib.mfh_set_poly_exact_points(self._h, None))
            return
        pts = [int(x) for x in pts]
        if len(pts) != 4 or not all(0 <= x < 2**32 for x in pts):
            raise MfhError(f"set_exact_points: four uint32 values, got {pts!r}")
        self._chk(self.lib.mfh_set_poly_exact_points(self._h, (ctypes.c_uint32 * 4)(*pts)))

    def set_mm_chunk_rows(self, rows=0):
        """rows per row chunk of the matrix-core launches (<= 131071; 0 = default): smaller values force several chunks"""
        self._chk(self.lib.mfh_set_mm_chunk_rows(self._h, int(rows)))

    def timing_drain(self, which):
        """(launch count, total ms, total rows) of the launches of kind `which` since the last drain"""
        n, rows, ms, last = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_double(), ctypes.c_float()
        self._chk(self.lib.mfh_timing_drain(self._h, which.encode(), ctypes.byref(n), ctypes.byref(ms), ctypes.byref(rows), ctypes.byref(last)))
        return n.value, ms.value, rows.value

    def timing_busy_ms(self):
        """union of the spans of the launches the last timing_drain matched (ms): < total ms when two streams overlapped"""
        return float(self.lib.mfh_timing_busy_ms(self._h))

    def timing_work_rows(self):
        """rows x evaluations served by the launches the last timing_drain matched"""
        return int(self.lib.mfh_timing_work_rows(self._h))

    def last_kernel_ms(self, which):
        return float(self.lib.mfh_last_kernel_ms(self._h, which.encode()))

    # -- reference-shaped operations ----------------------------------------------------------------------
    def set_seed(self, seed: bytes):
        """rng_init(rng, seed) -- src/entropy.c:58-61."""
        assert len(seed) == 40
        self._chk(self.lib.mfh_set_seed(self._h, bytes(seed)))

    def keystream(self, off, nbytes, out=None):
        """rng_seek(off); rng_gen(nbytes) -- src/entropy.c:46-56, src/aes.c:104-144."""
        out = self.empty(nbytes) if out is None else out
        self._chk(self.lib.mfh_keystream(self._h, off, _ptr(out), nbytes))
        return out

    def sample_rows(self, off, nrows):
        """mpz2_urandommv for nrows rows -- src/entropy.h:62-66.  Returns uint8 tensor of nrows*n*L*8 bytes."""
        p = self.params
        out = self.empty(nrows * p.n * p.L * 8)
        self._chk(self.lib.mfh_sample_rows(self._h, off, nrows, _ptr(out)))
        return out

    def ct_add(self, a, b, count=1, out=None):
        out = self.empty(a.numel()) if out is None else out
        self._chk(self.lib.mfh_ct_add(self._h, _ptr(out), _ptr(a), _ptr(b), count))
        return out

    def ct_mul_ui(self, a, x, count=1, out=None):
        out = self.empty(a.numel()) if out is None else out
        self._chk(self.lib.mfh_ct_mul_ui(self._h, _ptr(out), _ptr(a), x, count))
        return out

    def ct_addmul_ui(self, rop, a, x, count=1):
        self._chk(self.lib.mfh_ct_addmul_ui(self._h, _ptr(rop), _ptr(a), x, count))
        return rop

    def eval_rows(self, off, nrows, c8, coeff0, coeff1=None, rop0=None, rop1=None, accumulate=False):
        """eval_poly (src/lwe.c:176-186) for one or two coefficient vectors; returns (rop0, rop1)."""
        p = self.params
        if rop0 is None:
            rop0 = self.empty(p.ct_limbs * 8)
        if coeff1 is not None and rop1 is None:
            rop1 = self.empty(p.ct_limbs * 8)
        self._chk(self.lib.mfh_eval_rows(self._h, off, nrows, _ptr(c8), _ptr(coeff0), _ptr(coeff1), _ptr(rop0), _ptr(rop1),
                                         1 if accumulate else 0))
        return rop0, rop1

    def eval_rows_multi(self, off, nrows, c8, coeffs, nvec, out=None, accumulate=False, coeff_bytes=4):
        """coeffs: nvec x nrows uint32 on the device (vector-major) -> nvec ciphertexts (vector-major); matrix-core path.
        coeff_bytes = 1: every coefficient < 256 (up to 127 vectors); 4: any uint32 (up to 31 vectors)"""
        out = self.empty(nvec * self.params.ct_limbs * 8) if out is None else out
        self._chk(self.lib.mfh_eval_rows_multi(self._h, off, nrows, _ptr(c8), _ptr(coeffs), nvec, coeff_bytes, _ptr(out), 1 if accumulate else 0))
        return out

    def encrypt_rows(self, off, nrows, sk, msg, err, out=None):
        """regev_encrypt2 + ct_export batch (src/lwe.c:78-97,115-119)."""
        p = self.params
        out = self.empty(nrows * p.ctb) if out is None else out
        self._chk(self.lib.mfh_encrypt_rows(self._h, off, nrows, _ptr(sk), _ptr(msg), _ptr(err), _ptr(out)))
        return out

    def decrypt(self, sk, cts, count, out=None):
        """regev_decrypt (src/lwe.c:105-111) of `count` full ciphertexts -> count uint32"""
        out = self.empty(4 * count) if out is None else out
        self._chk(self.lib.mfh_decrypt(self._h, _ptr(sk), _ptr(cts), count, _ptr(out)))
        return out

    def set_decrypt_path(self, path=0):
        """decrypt: 0 = by batch size, 1 = VALU kernel, 2 = matrix-core kernel"""
        self._chk(self.lib.mfh_set_decrypt_path(self._h, int(path)))

    def decrypt_rows(self, off, nrows, sk, c8, out=None):
        """regev_decrypt of nrows seed-compressed ciphertexts (a regenerated from the stream at off + i * CTR_CT, b = c8[i]) -> nrows uint32"""
        out = self.empty(4 * nrows) if out is None else out
        self._chk(self.lib.mfh_decrypt_rows(self._h, off, nrows, _ptr(sk), _ptr(c8), _ptr(out)))
        return out

    def ct_smudge(self, cts, count, mag: bytes, maglen, sign: bytes):
        self._chk(self.lib.mfh_ct_smudge(self._h, _ptr(cts), count, bytes(mag), maglen, bytes(sign)))
        return cts

    def ssp_upload(self, ssp_host_u64: np.ndarray, d_ssp=None, first_slot=0, nslots=None):
        p = self.params
        nslots = p.m + 3 if nslots is None else nslots
        if d_ssp is None:
            d_ssp = self.empty((p.m + 3) * p.d * 4)
        a = np.ascontiguousarray(ssp_host_u64)
        self._chk(self.lib.mfh_ssp_upload(self._h, ctypes.c_void_p(a.ctypes.data), _ptr(d_ssp), first_slot, nslots))
        return d_ssp

    def ssp_from_rows(self, rows, d_ssp=None):
        """the SSP of a constraint system given row by row (mfh_ssp_from_rows): rows = (row_ptr, wire, coef) arrays in CSR form, or a sequence of rows
        each a sequence of (wire, coef) pairs; row j asks v_0(r_j) + sum_i a_i v_i(r_j) in {-1, +1} at r_j = j + 2.  Returns the device SSP (written in full)."""
        p = self.params
        row_ptr, wire, coef = rows_to_csr(rows)
        if d_ssp is None:
            d_ssp = self.empty((p.m + 3) * p.d * 4)
        self._chk(self.lib.mfh_ssp_from_rows(self._h, len(row_ptr) - 1, ctypes.c_void_p(row_ptr.ctypes.data), ctypes.c_void_p(wire.ctypes.data),
                                             ctypes.c_void_p(coef.ctypes.data), _ptr(d_ssp)))
        return d_ssp

    def ssp_set_rows(self, rows, lu_max=0):
        """register the constraint system as its rows (mfh_ssp_set_rows): rows as for ssp_from_rows (e.g. circuit.Compiled.rows); afterwards d_ssp=None means
        this SSP in the setup, prover and verifier calls (call ssp_prepare(None) first).  rows=None unregisters and frees."""
        if rows is None:
            self._chk(self.lib.mfh_ssp_set_rows(self._h, 0, None, None, None, 0))
            return
        row_ptr, wire, coef = rows_to_csr(rows)
        self._chk(self.lib.mfh_ssp_set_rows(self._h, len(row_ptr) - 1, ctypes.c_void_p(row_ptr.ctypes.data), ctypes.c_void_p(wire.ctypes.data),
                                            ctypes.c_void_p(coef.ctypes.data), int(lu_max)))

    def ssp_rows_fill(self, first_slot, nslots):
        """slots [first_slot, first_slot + nslots) of the registered row SSP in the dense layout (mfh_ssp_rows_fill): nslots * d uint32 on the device"""
        out = self.empty(max(nslots, 1) * self.params.d * 4)
        self._chk(self.lib.mfh_ssp_rows_fill(self._h, first_slot, nslots, _ptr(out)))
        return out

    def ssp_rows_violations(self, witness_bits_list):
        """the row check (mfh_ssp_rows_violations): for each statement's witness bits (rows of circuit_assign, or bytes as prove_batch takes them) the number of
        rows of the registered row SSP it violates and the smallest violated row index (0xFFFFFFFF when there is none) -> (count, first), np.uint32 arrays.
        circuit.Compiled.row_source names a reported row."""
        nb = len(witness_bits_list)
        count, first = np.zeros(nb, dtype=np.uint32), np.full(nb, 0xFFFFFFFF, dtype=np.uint32)
        bits, stride = self._pack_bits(witness_bits_list)
        self._chk(self.lib.mfh_ssp_rows_violations(self._h, nb, bits if nb else None, stride, ctypes.c_void_p(count.ctypes.data), ctypes.c_void_p(first.ctypes.data)))
        return count, first

    def circuit_load(self, compiled, state="lds"):
        """the gate program of circuit.Compiled on the device: levelised and uploaded once; close() frees it.  state: "lds" (the wire state in LDS, at
        most CIRCUIT_MAX_WIRES wires), "global" (in device memory, up to m - 1 wires) or "auto" (lds up to CIRCUIT_MAX_WIRES wires, else global).
        The entry point, by what the circuit holds, the first that applies, each in the kind `state` names:
          a weighted-sum gate (Circuit.wsum, Compiled.terms)                                        mfh_circuit_create_sum
          computed public outputs (Circuit.output, Compiled.outputs)                                mfh_circuit_create_out
          a MAJ / SUM3 / CONST / LUT2 gate or an equality (Compiled.program, Compiled.equal)        mfh_circuit_create_ex
          XOR / AND / OR / NOT gates and assertions alone                                           mfh_circuit_create ("lds"), mfh_circuit_create_global"""
        if state not in ("lds", "global", "auto"):
            raise MfhError(f"circuit_load: state must be 'lds', 'global' or 'auto', got {state!r}")
        gates = np.ascontiguousarray(compiled.gates, dtype=np.uint32).reshape(-1, 3)
        asserts = np.ascontiguousarray(compiled.asserts, dtype=np.uint32).reshape(-1, 2)
        # a program description without program / equal (gates, asserts, nwires alone) is one of the four original ops
        program = np.ascontiguousarray(getattr(compiled, "program", np.zeros((0, 4))), dtype=np.uint32).reshape(-1, 4)
        equal = np.ascontiguousarray(getattr(compiled, "equal", np.zeros((0, 2))), dtype=np.uint32).reshape(-1, 2)
        outputs = np.ascontiguousarray(getattr(compiled, "outputs", np.zeros((0, 2))), dtype=np.uint32).reshape(-1, 2)
        terms = np.ascontiguousarray(getattr(compiled, "terms", np.zeros((0, 2))), dtype=np.uint32).reshape(-1, 2)
        sums = bool((program[:, 0] == 8).any())  # MFH_GATE_WSUM
        extended = len(equal) > 0 or len(outputs) > 0 or bool((program[:, 0] > 3).any())
        nin = compiled.nwires - len(gates)
        if state == "auto":
            state = "lds" if compiled.nwires <= CIRCUIT_MAX_WIRES else "global"
        h = ctypes.c_void_p()

        def arr(x):
            return ctypes.c_void_p(x.ctypes.data)

        flags = CIRCUIT_GLOBAL if state == "global" else 0
        ex = [self._h, nin, len(program), arr(program), len(asserts), arr(asserts), len(equal), arr(equal)]
        if sums:
            self._chk(self.lib.mfh_circuit_create_sum(*ex, len(outputs), arr(outputs), len(terms), arr(terms), flags, ctypes.byref(h)))
        elif len(outputs):
            self._chk(self.lib.mfh_circuit_create_out(*ex, len(outputs), arr(outputs), flags, ctypes.byref(h)))
        elif extended:
            self._chk(self.lib.mfh_circuit_create_ex(*ex, flags, ctypes.byref(h)))
        else:
            create = self.lib.mfh_circuit_create if state == "lds" else self.lib.mfh_circuit_create_global
            self._chk(create(self._h, nin, len(gates), arr(gates), len(asserts), arr(asserts), ctypes.byref(h)))
        return CircuitProgram(self, nin, len(gates), h, state, extended, len(outputs), sums)

    def circuit_assign(self, prog, bits):
        """witnesses of nb statements on the device (mfh_circuit_assign): bits = uint8 [nb, nin] of 0 / 1, public bits then private bits (whatever stands
        at the position of a computed public output is ignored: the witness row carries the computed bit there).
        Returns (witness, holds): witness uint8 [nb, (m + 7) // 8], row b = Circuit.assign of statement b (prove_batch takes it as it is);
        holds bool [nb] = Circuit.holds"""
        bits = np.asarray(bits, dtype=np.uint8)
        if bits.ndim != 2 or bits.shape[1] != prog.nin:
            raise MfhError(f"circuit_assign: bits must be [nb, {prog.nin}] (public then private bits), got {bits.shape}")
        nb = bits.shape[0]
        packed = np.ascontiguousarray(np.packbits(bits & 1, axis=1, bitorder="little"))
        stride = (self.params.m + 7) // 8
        witness = np.zeros((nb, stride), dtype=np.uint8)
        holds = np.zeros(nb, dtype=np.uint8)
        self._chk(self.lib.mfh_circuit_assign(self._h, prog._h, nb, ctypes.c_void_p(packed.ctypes.data), packed.shape[1], ctypes.c_void_p(witness.ctypes.data),
                                              stride, ctypes.c_void_p(holds.ctypes.data)))
        return witness, holds.astype(bool)

    def sha256_records(self, records):
        """torch uint8 [n, 32] on the device: SHA-256 of each of n records of one length, what hashlib.sha256(record).digest() gives
        (mfh_sha256_records: one launch of k_sha256_records, queue-only).  records: a numpy uint8 [n, length], uploaded (the call then waits for the
        stream, the upload being its own), or a torch uint8 tensor [n, length] on the context's device with stride(1) == 1 and stride(0) >= length, read
        in place when the context's stream reaches the call: a column slice of a wider table is no copy."""
        t, stride, length, n, host = _records(self, records, "sha256_records")
        out = self.torch.empty((n, 32), dtype=self.torch.uint8, device=self.device)
        self._chk(self.lib.mfh_sha256_records(self._h, _ptr(t), stride, length, n, _ptr(out)))
        if host:
            self.sync()
        return out

    def merkle_tree(self, depth):
        """a MerkleTree of 2^depth zero leaves on this context's device (mfh_merkle_create: 1 <= depth <= 24); close() frees it, before the context"""
        h = ctypes.c_void_p()
        self._chk(self.lib.mfh_merkle_create(self._h, int(depth), ctypes.byref(h)))
        return MerkleTree(self, int(depth), h)

    def ssp_to_host_u64(self, d_ssp):
        """the device SSP in the reference's host layout: (m + 3) * d uint64 (files.ssp_write, the oracle, the shim's setup())"""
        p = self.params
        return self.to_host(d_ssp[: (p.m + 3) * p.d * 4], np.uint32).astype(np.uint64)

    def witness_poly(self, d_ssp, witness_bits: bytes, delta):
        out = self.empty(self.params.d * 4)
        self._chk(self.lib.mfh_witness_poly(self._h, _ptr(d_ssp), bytes(witness_bits), delta, _ptr(out)))
        return out

    # -- polynomial step, setup, prover ---------------------------------------------------------------------
    def poly_mul(self, a, la, b, lb):
        out = self.empty((la + lb - 1) * 4)
        self._chk(self.lib.mfh_poly_mul(self._h, _ptr(a), la, _ptr(b), lb, _ptr(out)))
        return out

    def poly_add(self, a, b, count):
        """a + b over F_p, `count` coefficients (nmod_poly_add, src/snark.c:161)"""
        out = self.empty(count * 4)
        self._chk(self.lib.mfh_poly_add(self._h, _ptr(a), _ptr(b), count, _ptr(out)))
        return out

    def ssp_prepare(self, d_ssp):
        """per-SSP precomputation for the division by t(x) (src/snark.c:169)"""
        self._chk(self.lib.mfh_ssp_prepare(self._h, _ptr(d_ssp)))

    def poly_prepare_t(self, d_t):
        self._chk(self.lib.mfh_poly_prepare_t(self._h, _ptr(d_t)))

    def poly_h(self, d_v):
        out = self.empty(self.params.d * 4)
        self._chk(self.lib.mfh_poly_h(self._h, _ptr(d_v), _ptr(out)))
        return out

    def poly_h_many(self, d_v, nb):
        """h_k = floor((v_k^2 - 1) / t) for nb polynomials side by side (mfh_poly_h_multi): one set of launches for the batch"""
        out = self.empty(nb * self.params.d * 4)
        self._chk(self.lib.mfh_poly_h_multi(self._h, _ptr(d_v), _ptr(out), nb))
        return out

    def setup_messages(self, d_ssp, alpha, beta, s):
        p = self.params
        out = self.empty((2 * p.d + p.m) * 4)
        self._chk(self.lib.mfh_setup_messages(self._h, _ptr(d_ssp), alpha, beta, s, _ptr(out)))
        return out

    def setup(self, d_ssp, alpha, beta, s, d_sk, d_err, out=None):
        """setup() (src/snark.c:57-115): returns the device CRS, (2d+m)*CT_BYTES bytes in stream order."""
        p = self.params
        out = self.empty((2 * p.d + p.m) * p.ctb) if out is None else out
        self._chk(self.lib.mfh_setup(self._h, _ptr(d_ssp), alpha, beta, s, _ptr(d_sk), _ptr(d_err), _ptr(out)))
        return out

    def setup_image(self, d_ssp, alpha, beta, s, d_sk, d_err, out=None, rows=None):
        """setup() leaving the expanded rows behind: returns (device CRS, row image for set_resident)"""
        p = self.params
        out = self.empty((2 * p.d + p.m) * p.ctb) if out is None else out
        rows = self.empty((2 * p.d + p.m) * self.resident_row_bytes()) if rows is None else rows
        self._chk(self.lib.mfh_setup_image(self._h, _ptr(d_ssp), alpha, beta, s, _ptr(d_sk), _ptr(d_err), _ptr(out), _ptr(rows)))
        return out, rows

    def prove(self, d_crs, d_ssp, witness_bits: bytes, delta, smudge_mag: bytes, smudge_sign: bytes, maglen=80, out=None):
        """prover() (src/snark.c:117-190): returns 5 ciphertexts h | hat_h | hat_v | v_w | b_w."""
        p = self.params
        out = self.empty(5 * p.ct_limbs * 8) if out is None else out
        assert len(smudge_mag) == 5 * maglen and len(smudge_sign) == 5
        self._chk(self.lib.mfh_prove(self._h, _ptr(d_crs), _ptr(d_ssp), bytes(witness_bits), delta, bytes(smudge_mag), maglen,
                                     bytes(smudge_sign), _ptr(out)))
        return out

    def crs_expand_mm(self, d_crs, out=None):
        """the CRS expanded once for the matrix-core batch prover (11.3 GB at the default instance, MFMA A-fragment order)"""
        out = self.empty(int(self.lib.mfh_crs_mm_image_bytes(self._h))) if out is None else out
        self._chk(self.lib.mfh_crs_expand_mm(self._h, _ptr(d_crs), _ptr(out)))
        return out

    def set_resident_mm(self, image):
        self._resident_mm = image
        self._chk(self.lib.mfh_crs_set_resident_mm(self._h, _ptr(image)))

    def witness_poly_many(self, d_ssp, witness_bits_list, deltas, mm=True):
        """w polynomials of up to 256 (mm) / 12 statements in one read of the SSP, or of any number by the batch prover's streamed pass (mm="stream")
        -> len x d uint32 on the device"""
        p = self.params
        nb = len(witness_bits_list)
        stride = (p.m + 6) // 8
        bits = b"".join(bytes(w[:stride]).ljust(stride, b"\0") for w in witness_bits_list)
        dl = (ctypes.c_uint32 * nb)(*[int(x) for x in deltas])
        out = self.empty(nb * p.d * 4)
        fn = self.lib.mfh_witness_poly_stream if mm == "stream" else self.lib.mfh_witness_poly_mm if mm else self.lib.mfh_witness_poly_multi
        self._chk(fn(self._h, _ptr(d_ssp), nb, bits, stride, ctypes.cast(dl, ctypes.c_void_p), _ptr(out)))
        return out

    def prove_batch(self, d_crs, d_ssp, witness_bits_list, deltas, smudge_mags, smudge_signs, maglen=80, out=None):
        """prover() for len(witness_bits_list) statements under one CRS: regions expanded once per group of 31, MAC on the matrix cores"""
        p = self.params
        nb = len(witness_bits_list)
        stride = (p.m + 6) // 8
        bits = b"".join(bytes(w[:stride]).ljust(stride, b"\0") for w in witness_bits_list)
        dl = (ctypes.c_uint32 * nb)(*[int(x) for x in deltas])
        mags = b"".join(bytes(x) for x in smudge_mags)
        signs = b"".join(bytes(x) for x in smudge_signs)
        assert len(mags) == nb * 5 * maglen and len(signs) == nb * 5
        out = self.empty(nb * 5 * p.ct_limbs * 8) if out is None else out
        self._chk(self.lib.mfh_prove_batch(self._h, _ptr(d_crs), _ptr(d_ssp), nb, bits, stride, ctypes.cast(dl, ctypes.c_void_p), mags, maglen,
                                           signs, _ptr(out)))
        return out

    def prove_batch_supergroup(self):
        """statements per super-group of the last prove_batch call (255 streaming, 248 regenerating; 0 before the first call)"""
        return int(self.lib.mfh_prove_batch_supergroup(self._h))

    def prove_batch_stream_wait(self, upto, stream):
        """make the torch stream `stream` wait until statements [0, upto) of the last prove_batch call are final in its output"""
        self._chk(self.lib.mfh_prove_batch_stream_wait(self._h, int(upto), ctypes.c_void_p(stream.cuda_stream)))

    # -- row-sharded batch prover (one process per GPU; dist.prove_batch_sharded drives the sequence) ----------------
    def _pack_bits(self, witness_bits_list):
        stride = (self.params.m + 6) // 8
        return b"".join(bytes(w[:stride]).ljust(stride, b"\0") for w in witness_bits_list), stride

    def crs_expand_mm_share(self, d_crs, rank, world, out=None):
        """rank's row shares of the S | AS | BT+BV regions expanded in MFMA A-fragment order (45 GB per GPU for the 2^20-constraint CRS on 8)"""
        out = self.empty(int(self.lib.mfh_crs_mm_share_bytes(self._h, rank, world))) if out is None else out
        self._chk(self.lib.mfh_crs_expand_mm_share(self._h, _ptr(d_crs), rank, world, _ptr(out)))
        return out

    def set_resident_mm_share(self, image, rank, world):
        self._resident_mm = image
        self._chk(self.lib.mfh_crs_set_resident_mm_share(self._h, _ptr(image), rank, world))

    def batch_chain(self, d_ssp, witness_bits_list, deltas, out=None):
        """w | h | v of the statements (src/snark.c:141-169): int32 tensor [3][len][d] (the uint32 coefficients' bit patterns)"""
        p = self.params
        nb = len(witness_bits_list)
        out = self.torch.empty((3, nb, p.d), dtype=self.torch.int32, device=self.device) if out is None else out
        if nb == 0:
            return out
        bits, stride = self._pack_bits(witness_bits_list)
        dl = (ctypes.c_uint32 * nb)(*[int(x) for x in deltas])
        self._chk(self.lib.mfh_batch_chain(self._h, _ptr(d_ssp), nb, bits, stride, ctypes.cast(dl, ctypes.c_void_p), _ptr(out[0]), _ptr(out[1]), _ptr(out[2])))
        return out

    def batch_witness_cols(self, d_ssp, witness_bits_list, deltas, col0, ncols, out=None):
        """coefficients [col0, col0 + ncols) of w of every statement: int32 tensor [len][ncols]"""
        nb = len(witness_bits_list)
        out = self.torch.empty((nb, ncols), dtype=self.torch.int32, device=self.device) if out is None else out
        if nb == 0 or ncols == 0:
            return out
        bits, stride = self._pack_bits(witness_bits_list)
        dl = (ctypes.c_uint32 * nb)(*[int(x) for x in deltas])
        self._chk(self.lib.mfh_batch_witness_cols(self._h, _ptr(d_ssp), nb, bits, stride, ctypes.cast(dl, ctypes.c_void_p), int(col0), int(ncols), _ptr(out), int(ncols)))
        return out

    def batch_chain_from_w(self, d_ssp, whv):
        """whv: int32 [3][n][d] with the whole w polynomials in whv[0]; fills whv[1] = h and whv[2] = v"""
        n = whv.shape[1]
        if n:
            self._chk(self.lib.mfh_batch_chain_from_w(self._h, _ptr(d_ssp), n, _ptr(whv[0]), _ptr(whv[1]), _ptr(whv[2])))
        return whv

    def prove_batch_partial(self, d_crs, rank, world, witness_bits_list, d_w, d_h, d_v, coef_stride, out=None):
        """rank's row shares of the five ciphertexts of every statement: len x 5 partial ciphertexts (no delta ct_t term, un-smudged)"""
        p = self.params
        nb = len(witness_bits_list)
        need = nb * 5 * p.ct_limbs * 8
        out = self.empty(need) if out is None else out
        if out.numel() * out.element_size() < need:
            raise MfhError(f"prove_batch_partial: `out` holds {out.numel() * out.element_size()} bytes, {nb} statements need {need}")
        bits, stride = self._pack_bits(witness_bits_list)
        self._chk(self.lib.mfh_prove_batch_partial(self._h, _ptr(d_crs), rank, world, nb, bits, stride, _ptr(d_w), _ptr(d_h), _ptr(d_v), int(coef_stride),
                                                   _ptr(out)))
        return out

    def prove_batch_finish(self, d_crs, deltas, smudge_mags, smudge_signs, d_proofs, maglen=80):
        """b_w += delta ct_t, then the smudging, on len(deltas) summed proofs in place"""
        nb = len(deltas)
        if nb == 0:
            return d_proofs
        dl = (ctypes.c_uint32 * nb)(*[int(x) for x in deltas])
        mags = b"".join(bytes(x) for x in smudge_mags)
        signs = b"".join(bytes(x) for x in smudge_signs)
        assert len(mags) == nb * 5 * maglen and len(signs) == nb * 5
        self._chk(self.lib.mfh_prove_batch_finish(self._h, _ptr(d_crs), nb, ctypes.cast(dl, ctypes.c_void_p), mags, maglen, signs, _ptr(d_proofs)))
        return d_proofs

    # -- row-sharded prover (one process per GPU; see dist.py) ------------------------------------------------
    def prove_partial(self, d_crs, d_ssp, witness_bits: bytes, delta, rank, world, out=None):
        p = self.params
        out = self.empty(5 * p.ct_limbs * 8) if out is None else out
        self._chk(self.lib.mfh_prove_partial(self._h, _ptr(d_crs), _ptr(d_ssp), bytes(witness_bits), delta, rank, world, _ptr(out)))
        return out

    def prove_finish(self, d_proof, smudge_mag: bytes, smudge_sign: bytes, maglen=80):
        self._chk(self.lib.mfh_prove_finish(self._h, _ptr(d_proof), bytes(smudge_mag), maglen, bytes(smudge_sign)))
        return d_proof

    def digest128(self, d_buf, nbytes=None):
        """128-bit digest of a device buffer (a cache key, not a cryptographic hash): (lo, hi)"""
        h = (ctypes.c_uint64 * 2)()
        n = d_buf.numel() * d_buf.element_size() if nbytes is None else int(nbytes)
        self._chk(self.lib.mfh_digest128(self._h, _ptr(d_buf), n, ctypes.cast(h, ctypes.c_void_p)))
        return int(h[0]), int(h[1])

    def ct_to_lanes(self, d_cts, count, out=None):
        p = self.params
        out = self.torch.empty(count * (p.n + 1) * p.lanes, dtype=self.torch.int64, device=self.device) if out is None else out
        self._chk(self.lib.mfh_ct_to_lanes(self._h, _ptr(d_cts), count, _ptr(out)))
        return out

    def ct_from_lanes(self, d_lanes, count, out=None):
        p = self.params
        out = self.empty(count * p.ct_limbs * 8) if out is None else out
        self._chk(self.lib.mfh_ct_from_lanes(self._h, _ptr(d_lanes), count, _ptr(out)))
        return out

    def add_dotp(self, rop, a, b, length):
        """mpz_add_dotp (src/lwe.c:20-28) on device values"""
        self._chk(self.lib.mfh_add_dotp(self._h, _ptr(rop), _ptr(a), _ptr(b), length))
        return rop

    # -- resident (materialised) CRS ------------------------------------------------------------------------------
    def resident_row_bytes(self):
        return int(self.lib.mfh_resident_row_bytes(self._h))

    def crs_expand(self, off, nrows, c8, out=None):
        """expand rows (a-vectors from the stream + b from c8) once into the streaming layout"""
        out = self.empty(nrows * self.resident_row_bytes()) if out is None else out
        self._chk(self.lib.mfh_crs_expand(self._h, off, nrows, _ptr(c8), _ptr(out)))
        return out

    def crs_image_set_b(self, image, first_row, nrows, c8):
        """coordinate n (the b's) of rows [first_row, first_row + nrows) of a row image expanded with c8 = None"""
        self._chk(self.lib.mfh_crs_image_set_b(self._h, int(first_row), int(nrows), _ptr(c8), _ptr(image)))
        return image

    def eval_rows_resident(self, rows, first_row, nrows, coeff0, coeff1=None, rop0=None, rop1=None, accumulate=False):
        p = self.params
        if rop0 is None:
            rop0 = self.empty(p.ct_limbs * 8)
        if coeff1 is not None and rop1 is None:
            rop1 = self.empty(p.ct_limbs * 8)
        self._chk(self.lib.mfh_eval_rows_resident(self._h, _ptr(rows), first_row, nrows, _ptr(coeff0), _ptr(coeff1), _ptr(rop0), _ptr(rop1),
                                                  1 if accumulate else 0))
        return rop0, rop1

    def set_resident(self, rows):
        self._resident = rows  # keep the tensor alive
        self._chk(self.lib.mfh_crs_set_resident(self._h, _ptr(rows)))

    def witness_lanes(self, d_ssp, witness_bits: bytes, rank, world, out=None):
        out = self.torch.empty(self.params.d, dtype=self.torch.int64, device=self.device) if out is None else out
        self._chk(self.lib.mfh_witness_lanes(self._h, _ptr(d_ssp), bytes(witness_bits), rank, world, _ptr(out)))
        return out

    def prove_partial_w(self, d_crs, d_ssp, witness_bits: bytes, delta, rank, world, wlanes, out=None):
        p = self.params
        out = self.empty(5 * p.ct_limbs * 8) if out is None else out
        self._chk(self.lib.mfh_prove_partial_w(self._h, _ptr(d_crs), _ptr(d_ssp), bytes(witness_bits), delta, rank, world, _ptr(wlanes), _ptr(out)))
        return out

    def verify(self, d_ssp, alpha, beta, s, d_sk, d_proofs, count=1):
        """verifier() (src/snark.c:192-250) for `count` proofs on the device; returns a uint8 tensor of accept bits"""
        ok = self.empty(count)
        self._chk(self.lib.mfh_verify(self._h, _ptr(d_ssp), alpha, beta, s, _ptr(d_sk), _ptr(d_proofs), count, _ptr(ok)))
        return ok

    # -- public inputs: bits [0, lu) of a statement's m - 1 input bits are public (include/mfhip.h; the reference fixes l_u = 0) ---------------------
    def setup_public(self, d_ssp, alpha, beta, s, lu, d_sk, d_err, out=None, rows=None, image=False):
        """setup() with rows v[0..lu) encrypting 0: returns the device CRS, or (CRS, expanded rows) with image=True"""
        p = self.params
        out = self.empty((2 * p.d + p.m) * p.ctb) if out is None else out
        if image and rows is None:
            rows = self.empty((2 * p.d + p.m) * self.resident_row_bytes())
        self._chk(self.lib.mfh_setup_public(self._h, _ptr(d_ssp), alpha, beta, s, lu, _ptr(d_sk), _ptr(d_err), _ptr(out), _ptr(rows if image else None)))
        return (out, rows) if image else out

    def prove_public(self, d_crs, d_ssp, lu, bits: bytes, delta, smudge_mag: bytes, smudge_sign: bytes, maglen=80, out=None):
        """one proof of the statement bits[0, lu) with the witness bits[lu, m - 1): 5 ciphertexts h | hat_h | hat_v | v_w | b_w"""
        p = self.params
        out = self.empty(5 * p.ct_limbs * 8) if out is None else out
        assert len(smudge_mag) == 5 * maglen and len(smudge_sign) == 5
        stride = (p.m + 6) // 8
        self._chk(self.lib.mfh_prove_public(self._h, _ptr(d_crs), _ptr(d_ssp), lu, bytes(bits[:stride]).ljust(stride, b"\0"), delta, bytes(smudge_mag),
                                            maglen, bytes(smudge_sign), _ptr(out)))
        return out

    def prove_batch_public(self, d_crs, d_ssp, lu, bits_list, deltas, smudge_mags, smudge_signs, maglen=80, out=None):
        """prove_batch with a statement per proof (bits_list[b][0, lu)); proof b equals prove_public of statement b"""
        p = self.params
        nb = len(bits_list)
        bits, stride = self._pack_bits(bits_list)
        dl = (ctypes.c_uint32 * nb)(*[int(x) for x in deltas])
        mags = b"".join(bytes(x) for x in smudge_mags)
        signs = b"".join(bytes(x) for x in smudge_signs)
        assert len(mags) == nb * 5 * maglen and len(signs) == nb * 5
        out = self.empty(nb * 5 * p.ct_limbs * 8) if out is None else out
        self._chk(self.lib.mfh_prove_batch_public(self._h, _ptr(d_crs), _ptr(d_ssp), lu, nb, bits, stride, ctypes.cast(dl, ctypes.c_void_p), mags,
                                                  maglen, signs, _ptr(out)))
        return out

    def derive_vk(self, d_ssp, s, lu):
        """the verification key [t(s), v_0(s), v_1(s) .. v_lu(s)] mod p: lu + 2 uint32 on the device"""
        vk = self.empty((lu + 2) * 4)
        self._chk(self.lib.mfh_vk_derive(self._h, _ptr(d_ssp), s, lu, _ptr(vk)))
        return vk

    def verify_public(self, d_vk, lu, alpha, beta, d_sk, d_proofs, statements, count=None):
        """verifier() with statements (bytes each, bit i = u_i; bits lu and above ignored) from the verification key; a uint8 tensor of accept bits"""
        count = len(statements) if count is None else count
        ub = max(1, (lu + 7) // 8)
        st = b"".join(bytes(u[:ub]).ljust(ub, b"\0") for u in statements)
        ok = self.empty(count)
        self._chk(self.lib.mfh_verify_public(self._h, _ptr(d_vk), lu, alpha, beta, _ptr(d_sk), _ptr(d_proofs), st, ub, count, _ptr(ok)))
        return ok

    # -- generator-defined SSP (BASELINE configs 4/5): pass d_ssp=None to the SSP-consuming calls afterwards ---------
    def ssp_prg_make_t(self, seed64, witness_bits: bytes):
        t = self.empty(self.params.d * 4)
        self._chk(self.lib.mfh_ssp_prg_make_t(self._h, seed64, bytes(witness_bits), _ptr(t)))
        return t

    def ssp_set_prg(self, seed64, d_t):
        self._prg_t = d_t  # keep alive
        self._chk(self.lib.mfh_ssp_set_prg(self._h, seed64, _ptr(d_t)))

    def ssp_prg_fill(self, seed64, first_slot, nslots):
        out = self.empty(nslots * self.params.d * 4)
        self._chk(self.lib.mfh_ssp_prg_fill(self._h, seed64, first_slot, nslots, _ptr(out)))
        return out

    # -- sharded resident CRS (one share per rank) -------------------------------------------------------------------
    def crs_expand_share(self, d_crs, rank, world, out=None):
        rows = int(self.lib.mfh_resident_share_rows(self._h, rank, world))
        out = self.empty(rows * self.resident_row_bytes()) if out is None else out
        self._chk(self.lib.mfh_crs_expand_share(self._h, _ptr(d_crs), rank, world, _ptr(out)))
        return out

    def set_resident_share(self, image, rank, world):
        self._resident = image
        self._chk(self.lib.mfh_crs_set_resident_share(self._h, _ptr(image), rank, world))

    def set_resident_prefix(self, image, nrows_resident):
        """only stream rows [0, nrows_resident) are resident; the rest is regenerated"""
        self._resident = image
        self._chk(self.lib.mfh_crs_set_resident_prefix(self._h, _ptr(image), nrows_resident))
