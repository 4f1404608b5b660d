"""ctypes binding of include/gosnark_hip.h (the same C ABI a cgo binding would use)."""
import ctypes
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None
_LOCK = threading.Lock()
_INIT_DEVICE = None

u64p = ctypes.POINTER(ctypes.c_uint64)
u32p = ctypes.POINTER(ctypes.c_uint32)
u8p = ctypes.POINTER(ctypes.c_uint8)
intp = ctypes.POINTER(ctypes.c_int)
Handle = ctypes.c_uint64


class GosnarkHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libgosnark_hip: status %d: %s" % (code, msg))
        self.code = code


class Timing(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_float) for n in
                 ("total_ms", "plan_ms", "accumulate_ms", "reduce_ms", "poly_ms", "h2d_ms", "acc_g1_ms", "acc_g2_ms")]
                + [("acc_g1_launches", ctypes.c_uint32), ("acc_g2_launches", ctypes.c_uint32),
                   ("acc_g1_terms", ctypes.c_uint64), ("acc_g2_terms", ctypes.c_uint64),
                   ("acc_g1_adds", ctypes.c_uint64), ("acc_g2_adds", ctypes.c_uint64),
                   ("window_bits", ctypes.c_uint32), ("fallbacks", ctypes.c_uint32),
                   ("plan_digits", ctypes.c_uint64), ("plan_entries", ctypes.c_uint64), ("heavy_buckets", ctypes.c_uint32), ("reserved", ctypes.c_uint32)])


class Memory(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("device_total_bytes", "device_free_bytes", "library_bytes", "object_bytes", "table_bytes",
                                               "workspace_bytes", "objects", "evictions")]


CHECK_MAX = 8
KEY_CHECKS = ("coefs A", "coefs B", "A", "B1", "B2", "IC", "C", "H")
PTAU_CHECKS = ("g1", "g2", "tau", "tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2")


class CheckResult(ctypes.Structure):
    _fields_ = ([(n, ctypes.c_int32) for n in ("ok", "lhs_g2", "rhs_g2", "lhs_inf", "rhs_inf", "reserved")]
                + [("lhs", ctypes.c_uint64 * 16), ("rhs", ctypes.c_uint64 * 16)])


class CheckReport(ctypes.Structure):
    _fields_ = [("nchecks", ctypes.c_uint32), ("failed", ctypes.c_uint32), ("check", CheckResult * CHECK_MAX)]


class SolveOpts(ctypes.Structure):
    _fields_ = [("narrow", ctypes.c_uint32), ("run_max_rows", ctypes.c_uint32)]


class SolveStats(ctypes.Structure):
    _fields_ = [(n, ctypes.c_uint64) for n in ("solved", "unsolved", "checks", "stuck", "levels", "launches", "wide_launches", "widest_level")]


class KeyCheckInput(ctypes.Structure):
    _fields_ = ([(n, Handle) for n in ("a", "b1", "b2", "ic", "c", "h", "key_system", "circuit_system", "tau_g1", "tau_g2", "alpha_tau_g1",
                                       "beta_tau_g1")]
                + [("delta2", ctypes.c_uint64 * 24), ("challenge", ctypes.c_uint64 * 4), ("log2_domain", ctypes.c_uint64), ("npublic", ctypes.c_uint64)])


def lib_path():
    # GS_LIB: development aid for A/B runs of two builds inside one GPU session
    return os.environ.get("GS_LIB") or os.path.join(_HERE, "libgosnark_hip.so")


# name -> (argtypes); every function returns int status unless listed in _NONSTATUS
_SIGS = {
    "gs_init": [intp, ctypes.c_int],
    "gs_free": [Handle],
    "gs_len": [Handle, ctypes.POINTER(ctypes.c_size_t)],
    "gs_g1_upload": [u64p, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_g2_upload": [u64p, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_g1_download": [Handle, u64p, ctypes.c_size_t],
    "gs_g2_download": [Handle, u64p, ctypes.c_size_t],
    "gs_g1_fixed_base": [u64p, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_g2_fixed_base": [u64p, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_scalars_upload": [u64p, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_scalars_download": [Handle, u64p, ctypes.c_size_t],
    "gs_scalars_update": [Handle, u64p, ctypes.c_size_t],
    "gs_msm_g1": [Handle, u64p, ctypes.c_size_t, ctypes.c_size_t, u64p, intp],
    "gs_msm_g2": [Handle, u64p, ctypes.c_size_t, ctypes.c_size_t, u64p, intp],
    "gs_msm_g1_resident": [Handle, ctypes.c_size_t, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, intp],
    "gs_msm_g2_resident": [Handle, ctypes.c_size_t, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, intp],
    "gs_msm_g1_begin": [Handle, ctypes.c_size_t, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p],
    "gs_msm_g2_begin": [Handle, ctypes.c_size_t, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p],
    "gs_msm_end": [ctypes.c_uint64, u64p, intp],
    "gs_g1_sum_affine": [u64p, intp, ctypes.c_size_t, u64p, intp],
    "gs_g2_sum_affine": [u64p, intp, ctypes.c_size_t, u64p, intp],
    "gs_poly_mul": [u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p],
    "gs_poly_div": [u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p, u64p],
    "gs_poly_add": [u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p],
    "gs_poly_sub": [u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p],
    "gs_poly_eval": [u64p, ctypes.c_size_t, u64p, u64p],
    "gs_lagrange_interpolation": [u64p, ctypes.c_size_t, u64p],
    "gs_zpoly": [ctypes.c_size_t, u64p],
    "gs_r1cs_to_px": [ctypes.c_size_t, ctypes.c_size_t, u32p, u32p, u64p, u32p, u32p, u64p, u32p, u32p, u64p,
                      u64p, u64p, u64p, u64p, u64p],
    "gs_r1cs_upload": [ctypes.c_size_t, ctypes.c_size_t, u32p, u32p, u64p, u32p, u32p, u64p, u32p, u32p, u64p, ctypes.POINTER(Handle)],
    "gs_r1cs_px": [Handle, Handle, ctypes.POINTER(Handle)],
    "gs_r1cs_check": [Handle, Handle, ctypes.c_size_t, u64p, u32p, u64p],
    "gs_r1cs_solve_plan": [Handle, u32p, ctypes.c_size_t, ctypes.POINTER(SolveOpts), ctypes.POINTER(Handle), ctypes.POINTER(SolveStats)],
    "gs_r1cs_solve_unsolved": [Handle, ctypes.c_size_t, u32p, u64p],
    "gs_r1cs_solve": [Handle, ctypes.c_size_t, u64p, ctypes.POINTER(Handle), u64p, u32p],
    "gs_solve_abi_sizes": [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)],
    "gs_r1cs_upload_domain": [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, u32p, u32p, u64p, u32p, u32p, u64p, u32p, u32p, u64p,
                              ctypes.POINTER(Handle)],
    "gs_groth16_pk_derive_eval_domain": [Handle, ctypes.c_size_t],
    "gs_groth16_pk_set_eval_domain": [Handle, Handle, ctypes.c_size_t],
    "gs_g1_upload_affine_mont": [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_g2_upload_affine_mont": [ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_r1cs_upload_zkey": [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_groth16_pk_create_domain": [Handle, Handle, Handle, Handle, Handle, u64p, u64p, u64p, u64p, u64p,
                                    ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_g1_lagrange": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(Handle)],
    "gs_g2_lagrange": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_r1cs_colsum_g1": [Handle, Handle, Handle, Handle, ctypes.POINTER(Handle)],
    "gs_r1cs_colsum_g2": [Handle, Handle, Handle, Handle, ctypes.POINTER(Handle)],
    "gs_g1_scale": [Handle, u64p, ctypes.POINTER(Handle)],
    "gs_g1_download_affine_mont": [Handle, ctypes.c_void_p, ctypes.c_size_t],
    "gs_g2_download_affine_mont": [Handle, ctypes.c_void_p, ctypes.c_size_t],
    "gs_g1_scale_powers": [Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, u64p, ctypes.POINTER(Handle)],
    "gs_g2_scale_powers": [Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, u64p, ctypes.POINTER(Handle)],
    "gs_groth16_key_check": [ctypes.POINTER(KeyCheckInput), ctypes.POINTER(CheckReport)],
    "gs_ptau_check": [Handle, Handle, Handle, Handle, u64p, ctypes.c_size_t, u64p, ctypes.POINTER(CheckReport)],
    "gs_check_abi_sizes": [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)],
    "gs_g1_lagrange_levels": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_g2_lagrange_levels": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_g1_lagrange_levels_check": [Handle, Handle, ctypes.c_size_t, u64p, ctypes.POINTER(CheckResult)],
    "gs_g2_lagrange_levels_check": [Handle, Handle, ctypes.c_size_t, u64p, ctypes.POINTER(CheckResult)],
    "gs_g2_subgroup_check": [Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, u64p],
    "gs_g1_decompress": [u64p, u8p, ctypes.c_size_t, ctypes.POINTER(Handle), u8p, u64p, u64p],
    "gs_g2_decompress": [u64p, u8p, ctypes.c_size_t, ctypes.POINTER(Handle), u8p, u64p, u64p],
    "gs_g1_compress": [Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, u8p],
    "gs_g2_compress": [Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, u8p],
    "gs_groth16_pk_create": [Handle, Handle, Handle, Handle, Handle, u64p, u64p, u64p, u64p, u64p,
                             u64p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_groth16_prove": [Handle, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p, u64p, u64p, intp],
    "gs_groth16_prove_resident": [Handle, Handle, Handle, u64p, u64p, u64p, intp],
    "gs_groth16_prove_r1cs": [Handle, Handle, Handle, ctypes.POINTER(Handle), u64p, u64p, u64p, intp],
    "gs_groth16_prove_witness": [Handle, Handle, Handle, u64p, u64p, u64p, intp],
    "gs_groth16_prove_witness_begin": [Handle, Handle, Handle, u64p, u64p, u64p],
    "gs_groth16_pk_set_eval": [Handle, Handle],
    "gs_pk_eval_count": [Handle, ctypes.POINTER(ctypes.c_size_t)],
    "gs_pinocchio_pk_set_eval": [Handle, Handle],
    "gs_groth16_pk_set_quot": [Handle, Handle],
    "gs_pinocchio_pk_set_quot": [Handle, Handle],
    "gs_pk_quot_count": [Handle, ctypes.POINTER(ctypes.c_size_t)],
    "gs_groth16_pk_derive_quot": [Handle],
    "gs_pinocchio_pk_derive_quot": [Handle],
    "gs_groth16_pk_derive_eval": [Handle, ctypes.c_size_t],
    "gs_pinocchio_pk_derive_eval": [Handle, ctypes.c_size_t],
    "gs_pinocchio_prove_witness_begin": [Handle, Handle, Handle, u64p],
    "gs_groth16_prove_begin": [Handle, Handle, Handle, u64p, u64p, u64p],
    "gs_groth16_prove_end": [ctypes.c_uint64, u64p, intp],
    "gs_groth16_prove_host_begin": [Handle, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p, u64p, u64p],
    "gs_groth16_prove_witness_host_begin": [Handle, Handle, u64p, ctypes.c_size_t, u64p, u64p, u64p],
    "gs_groth16_prove_witness_host": [Handle, Handle, u64p, ctypes.c_size_t, u64p, u64p, u64p, intp],
    "gs_pinocchio_prove_host_begin": [Handle, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p],
    "gs_pinocchio_prove_witness_host_begin": [Handle, Handle, u64p, ctypes.c_size_t, u64p],
    "gs_pinocchio_prove_witness_host": [Handle, Handle, u64p, ctypes.c_size_t, u64p, intp],
    "gs_ticket_cancel": [ctypes.c_uint64],
    "gs_groth16_pk_create_shard": [Handle, Handle, Handle, Handle, Handle, u64p, u64p, u64p, u64p, u64p, u64p, ctypes.c_size_t,
                                   ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_groth16_pk_shard": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_groth16_prove_partials": [Handle, Handle, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, intp],
    "gs_groth16_finish": [Handle, u64p, intp, u64p, u64p, u64p, intp],
    "gs_groth16_setup": [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, u32p, u32p, u64p, u32p, u32p, u64p, u32p, u32p, u64p,
                         u64p, ctypes.POINTER(Handle), u64p],
    "gs_groth16_pk_export": [Handle, ctypes.c_int, u64p, ctypes.c_size_t],
    "gs_pinocchio_setup": [ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, u32p, u32p, u64p, u32p, u32p, u64p, u32p, u32p, u64p,
                           u64p, ctypes.POINTER(Handle), u64p],
    "gs_pinocchio_pk_export": [Handle, ctypes.c_int, u64p, ctypes.c_size_t],
    "gs_pinocchio_pk_create": [Handle, Handle, Handle, Handle, Handle, Handle, Handle, Handle, u64p,
                               ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_pinocchio_prove": [Handle, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p, intp],
    "gs_pinocchio_prove_resident": [Handle, Handle, Handle, u64p, intp],
    "gs_pinocchio_prove_witness": [Handle, Handle, Handle, u64p, intp],
    "gs_pinocchio_prove_begin": [Handle, Handle, Handle, u64p],
    "gs_pinocchio_prove_end": [ctypes.c_uint64, u64p, intp],
    "gs_device_count": [],
    "gs_set_device": [ctypes.c_int],
    "gs_get_device": [],
    "gs_handle_device": [Handle],
    "gs_scalars_clone": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(Handle)],
    "gs_g1_clone": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(Handle)],
    "gs_g2_clone": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(Handle)],
    "gs_groth16_pk_shard_to": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(Handle)],
    "gs_comm_unique_id": [ctypes.POINTER(ctypes.c_uint8)],
    "gs_comm_init_rank": [ctypes.POINTER(ctypes.c_uint8), ctypes.c_int, ctypes.c_int],
    "gs_comm_init_local": [],
    "gs_comm_info": [intp, intp, intp, u64p],
    "gs_comm_allgather": [ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p],
    "gs_msm_g1_multi": [ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.c_int, u64p, intp, intp],
    "gs_msm_g2_multi": [ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.c_int, u64p, intp, intp],
    "gs_groth16_prove_multi": [ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.c_int, u64p, u64p, u64p, intp, intp],
    "gs_groth16_prove_sharded": [Handle, Handle, Handle, u64p, u64p, u64p, intp],
    "gs_groth16_witness_values": [Handle, Handle, Handle, ctypes.POINTER(Handle), ctypes.POINTER(ctypes.c_uint32)],
    "gs_groth16_prove_partials_values": [Handle, Handle, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, intp],
    "gs_groth16_partials_values_begin": [Handle, Handle, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p],
    "gs_groth16_partials_end": [ctypes.c_uint64, u64p, intp],
    "gs_groth16_prove_multi_values": [ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.c_int, u64p, u64p, u64p, intp, intp],
    "gs_groth16_prove_sharded_values": [Handle, Handle, Handle, u64p, u64p, u64p, intp],
    "gs_scalars_scatter": [Handle, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(Handle)],
    "gs_msm_g1_sharded": [Handle, Handle, u64p, intp],
    "gs_msm_g2_sharded": [Handle, Handle, u64p, intp],
    "gs_groth16_prove_batch": [ctypes.POINTER(Handle), ctypes.c_int, ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.c_size_t,
                               u64p, u64p, u64p, intp],
    "gs_pinocchio_pk_shard": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_pinocchio_pk_shard_to": [Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.POINTER(Handle)],
    "gs_pinocchio_prove_partials": [Handle, Handle, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, intp],
    "gs_pinocchio_witness_values": [Handle, Handle, Handle, ctypes.POINTER(Handle), ctypes.POINTER(ctypes.c_uint32)],
    "gs_pinocchio_prove_partials_values": [Handle, Handle, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, intp],
    "gs_pinocchio_combine": [u64p, intp, ctypes.c_size_t, u64p, intp],
    "gs_pinocchio_prove_multi": [ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.c_int, u64p, intp, intp],
    "gs_pinocchio_prove_multi_values": [ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.c_int, u64p, intp, intp],
    "gs_pinocchio_prove_sharded": [Handle, Handle, Handle, u64p, intp],
    "gs_pinocchio_prove_sharded_values": [Handle, Handle, Handle, u64p, intp],
    "gs_pinocchio_prove_batch": [ctypes.POINTER(Handle), ctypes.c_int, ctypes.POINTER(Handle), ctypes.POINTER(Handle), ctypes.c_size_t, u64p, intp],
    "gs_last_timing": [ctypes.POINTER(Timing)],
    "gs_device_timing": [ctypes.c_int, ctypes.POINTER(Timing)],
    "gs_set_window_bits": [ctypes.c_int],
    "gs_set_eval_basis": [ctypes.c_int],
    "gs_memory_query": [ctypes.POINTER(Memory)],
    "gs_handle_bytes": [Handle, u64p, u64p],
    "gs_release_tables": [Handle],
    "gs_set_table_policy": [ctypes.c_int],
    "gs_build_tables": [Handle, ctypes.c_int],
    "gs_set_memory_limit": [ctypes.c_uint64],
    "gs_alloc_counters": [u64p, u64p],
    "gs_abi_sizes": [ctypes.POINTER(ctypes.c_size_t), ctypes.POINTER(ctypes.c_size_t)],
    "gs_trim": [],
    "gs_verify_set_strict": [ctypes.c_int],
    "gs_pairing": [u64p, u64p, u64p],
    "gs_pairing_check": [u64p, u64p, ctypes.c_size_t, intp],
    "gs_groth16_verify": [u64p, u64p, u64p, u64p, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p, u64p, u64p, intp],
    "gs_pinocchio_verify": [u64p, u64p, u64p, u64p, u64p, u64p, u64p, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p, intp, intp],
    "gs_pairing_product": [Handle, ctypes.c_size_t, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, intp],
    "gs_groth16_verify_each": [u64p, u64p, u64p, u64p, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p, u64p, u64p, ctypes.c_size_t, intp,
                               ctypes.POINTER(ctypes.c_uint64)],
    "gs_pinocchio_verify_each": [u64p, u64p, u64p, u64p, u64p, u64p, u64p, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t,
                                 intp, intp, ctypes.POINTER(ctypes.c_uint64)],
    "gs_pairing_each": [Handle, ctypes.c_size_t, Handle, ctypes.c_size_t, ctypes.c_size_t, u64p, intp],
    "gs_groth16_vk_create": [u64p, u64p, u64p, u64p, u64p, ctypes.c_size_t, ctypes.POINTER(Handle)],
    "gs_groth16_verify_each_keys": [ctypes.POINTER(Handle), ctypes.c_size_t, u32p, u64p, u64p, u64p, u64p, ctypes.c_size_t, intp,
                                    ctypes.POINTER(ctypes.c_uint64)],
    "gs_groth16_verify_batch": [u64p, u64p, u64p, u64p, u64p, ctypes.c_size_t, u64p, ctypes.c_size_t, u64p, u64p, u64p, ctypes.c_size_t, u64p, intp],
}
EXPORTS = sorted(list(_SIGS) + ["gs_shutdown", "gs_last_error", "gs_version", "gs_comm_destroy"])


def load_library():
    """dlopen libgosnark_hip.so (built by `make -C go-snark-study_amd/csrc` / __graft_entry__.build()).
    Fails loudly when it is missing: there is no other implementation to fall back to."""
    global _LIB
    with _LOCK:
        if _LIB is not None:
            return _LIB
        path = lib_path()
        try:
            # torch ships its own libamdhip64/libhsa-runtime64 (same sonames as /opt/rocm's): when a process
            # uses both torch and this library (bench.py, smoke()), torch's copies must be the ones that get
            # loaded first, otherwise two HSA runtimes end up in the process and device discovery fails.
            import torch  # noqa: F401
        except ImportError:
            pass
        if not os.path.exists(path):
            raise GosnarkHipError(-1, "%s not found: build it with __graft_entry__.build() "
                                  "(hipcc --offload-arch=gfx950); there is no CPU fallback" % path)
        lib = ctypes.CDLL(path)
        missing = [n for n in EXPORTS if not hasattr(lib, n)]
        if missing:
            raise GosnarkHipError(-1, "%s lacks symbols declared in include/gosnark_hip.h: %s" % (path, missing))
        for name, args in _SIGS.items():
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = ctypes.c_int
        lib.gs_last_error.restype = ctypes.c_char_p
        lib.gs_version.restype = ctypes.c_char_p
        lib.gs_shutdown.restype = None
        lib.gs_comm_destroy.restype = None
        # gs_timing / gs_memory are written through our pointers: a library built from another revision of the header must not
        # be handed these structs (gs_timing grew by 24 bytes in round 4 without anything noticing)
        tb, mb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        lib.gs_abi_sizes(ctypes.byref(tb), ctypes.byref(mb))
        if tb.value != ctypes.sizeof(Timing) or mb.value != ctypes.sizeof(Memory):
            raise GosnarkHipError(-1, "%s writes gs_timing / gs_memory of %d / %d bytes, this binding expects %d / %d: rebuild the library"
                                  % (path, tb.value, mb.value, ctypes.sizeof(Timing), ctypes.sizeof(Memory)))
        ib, rb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        lib.gs_check_abi_sizes(ctypes.byref(ib), ctypes.byref(rb))
        if ib.value != ctypes.sizeof(KeyCheckInput) or rb.value != ctypes.sizeof(CheckReport):
            raise GosnarkHipError(-1, "%s takes gs_key_check_input / gs_check_report of %d / %d bytes, this binding expects %d / %d: rebuild the library"
                                  % (path, ib.value, rb.value, ctypes.sizeof(KeyCheckInput), ctypes.sizeof(CheckReport)))
        ob, sb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        lib.gs_solve_abi_sizes(ctypes.byref(ob), ctypes.byref(sb))
        if ob.value != ctypes.sizeof(SolveOpts) or sb.value != ctypes.sizeof(SolveStats):
            raise GosnarkHipError(-1, "%s takes gs_solve_opts / gs_solve_stats of %d / %d bytes, this binding expects %d / %d: rebuild the library"
                                  % (path, ob.value, sb.value, ctypes.sizeof(SolveOpts), ctypes.sizeof(SolveStats)))
        _LIB = lib
        return lib


def check(status):
    if status != 0:
        raise GosnarkHipError(status, load_library().gs_last_error().decode("utf-8", "replace"))


# ---- the call layer: every module of the package reaches a status-returning gs_* entry point through these ---------------------
def call(name, *args):
    """Entry point `name` of the library on args as its _SIGS row takes them; a non-zero status raises GosnarkHipError."""
    check(getattr(load_library(), name)(*args))


def raw(x):
    """The gs_handle integer of a DeviceHandle, either scheme's DevicePk, a DeviceR1CS (anything with .handle or .h), an int, or
    None (0: 'no object')."""
    x = getattr(x, "handle", x)
    return 0 if x is None else int(getattr(x, "h", x))


def harr(xs):
    """Handle array of a list of whatever raw() takes."""
    return (Handle * len(xs))(*[raw(x) for x in xs])


def result(words, flags=1, rows=1):
    """(uint64 result buffer of rows x words, its rows x flags infinity flags) for a call that writes affine points."""
    return np.zeros(words if rows == 1 else (rows, words), dtype=np.uint64), (ctypes.c_int * (flags * rows))()


def rs_limbs(r, s):
    """The randomness of a Groth16 proof reduced mod r -> its two limb pointers."""
    rs = ints_to_u64([r % R, s % R])
    return ptr64(rs[0]), ptr64(rs[1])


def ticket_cell():
    """Out-parameter of a *_begin call: pass ctypes.byref(t), the ticket is t.value."""
    return ctypes.c_uint64(0)


class HandleCell:
    """gs_handle in/out parameter.  Pass .ref; .result() is `existing` when the caller gave an object to overwrite, else a new
    DeviceHandle of what the library created."""

    def __init__(self, existing=None):
        self.existing, self.cell = existing, Handle(raw(existing))
        self.ref = ctypes.byref(self.cell)

    def result(self):
        return self.existing if self.existing is not None else DeviceHandle(self.cell.value)


def csr_args(csrs):
    """Three CSR triples (row_ptr, col, val) -> the nine pointers of gs_r1cs_upload* / gs_r1cs_to_px / gs_*_setup (an empty matrix
    still hands over one readable element)."""
    args = []
    for rp, cl, vl in csrs:
        rp = np.ascontiguousarray(rp, dtype=np.uint32)
        cl = np.ascontiguousarray(cl, dtype=np.uint32)
        vl = np.ascontiguousarray(vl, dtype=np.uint64).reshape(-1, 4)
        if cl.size == 0:
            cl, vl = np.zeros(1, dtype=np.uint32), np.zeros((1, 4), dtype=np.uint64)
        args += [ptr32(rp), ptr32(cl), ptr64(vl)]
    return args


def affine_words(points, g2_flags):
    """Affine tuples or None (infinity), points[i] in G2 where g2_flags[i] -> (flat uint64 limbs, c_int infinity flags)."""
    flat, infs = [], []
    for p, g2 in zip(points, g2_flags):
        if p is None:
            flat += [0] * (4 if g2 else 2)
        else:
            flat += ([p[0][0], p[0][1], p[1][0], p[1][1]] if g2 else [p[0], p[1]])
        infs.append(int(p is None))
    arr = ints_to_u64(flat).reshape(-1) if flat else np.zeros(0, dtype=np.uint64)
    return arr, (ctypes.c_int * max(len(infs), 1))(*infs)


def init(device=None):
    """gs_init on `device` (default: LOCAL_RANK or 0): one process drives one GPU.  `device` may also be a list of HIP
    ordinals -- one logical device (context) per entry, the same ordinal may repeat (see include/gosnark_hip.h)."""
    global _INIT_DEVICE
    if device is None:
        if _INIT_DEVICE is not None:          # already initialised: keep it
            return
        device = int(os.environ.get("LOCAL_RANK", "0"))
    devices = tuple(int(d) for d in device) if isinstance(device, (list, tuple)) else (int(device),)
    if _INIT_DEVICE == devices:
        return
    call("gs_init", (ctypes.c_int * len(devices))(*devices), len(devices))
    _INIT_DEVICE = devices


def device_count():
    return load_library().gs_device_count()


def set_device(logical):
    """Objects created by this host thread from now on live on logical device `logical`."""
    call("gs_set_device", int(logical))


def get_device():
    return load_library().gs_get_device()


def handle_device(handle):
    return load_library().gs_handle_device(raw(handle))


def shutdown():
    """gs_shutdown: every handle dies, streams / pinned buffers / workspaces are returned; init() may be called again."""
    global _INIT_DEVICE
    load_library().gs_shutdown()
    _INIT_DEVICE = None


def version():
    return load_library().gs_version().decode()


# ---- integer <-> limb array helpers -------------------------------------------------------------
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def ints_to_u64(vals, words=4):
    """list of non-negative Python ints -> np.uint64 array [len, words] (little-endian limbs)."""
    nbytes = 8 * words
    buf = b"".join(int(v).to_bytes(nbytes, "little") for v in vals)
    return np.frombuffer(buf, dtype="<u8").reshape(len(vals), words).copy()


def u64_to_ints(arr, words=4):
    a = np.ascontiguousarray(arr, dtype="<u8").reshape(-1, words)
    buf = a.tobytes()
    nbytes = 8 * words
    return [int.from_bytes(buf[i * nbytes:(i + 1) * nbytes], "little") for i in range(a.shape[0])]


def ptr64(a):
    if a is None:
        return None
    assert a.dtype == np.uint64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(u64p)


def ptr32(a):
    assert a.dtype == np.uint32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(u32p)


def g1_points_to_u64(points):
    """[(X, Y, Z), ...] Jacobian ints -> [n, 12] uint64"""
    flat = [c for p in points for c in p]
    return ints_to_u64(flat).reshape(len(points), 12)


def g2_points_to_u64(points):
    """[((X0,X1),(Y0,Y1),(Z0,Z1)), ...] -> [n, 24] uint64"""
    flat = [c for p in points for xy in p for c in xy]
    return ints_to_u64(flat).reshape(len(points), 24)


def g1_tuples(a):
    """[n, 12] uint64 -> [(X, Y, Z), ...] ints"""
    v = u64_to_ints(a)
    return [(v[3 * i], v[3 * i + 1], v[3 * i + 2]) for i in range(len(v) // 3)]


def g2_tuples(a):
    """[n, 24] uint64 -> [((X0,X1),(Y0,Y1),(Z0,Z1)), ...] ints"""
    v = u64_to_ints(a)
    return [((v[6 * i], v[6 * i + 1]), (v[6 * i + 2], v[6 * i + 3]), (v[6 * i + 4], v[6 * i + 5])) for i in range(len(v) // 6)]


def u64_rows(x):
    """ints (reduced mod r here) or an [n, 4] uint64 limb array (taken as it is: the device reduces any value < 2^256) -> contiguous
    [n, 4] uint64"""
    if isinstance(x, np.ndarray):
        return np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4)
    return ints_to_u64([v % R for v in x])


class DeviceHandle:
    """RAII wrapper of a gs_handle."""

    def __init__(self, h):
        self.h = int(h)

    def free(self):
        """gs_free.  Safe while tickets that read the object are outstanding (the library defers the release); if the call
        fails all the same (foreign handle) the handle is kept so that the failure is not silent."""
        if self.h:
            lib = load_library()
            rc = lib.gs_free(self.h)
            if rc == 0 or lib.gs_device_count() == 0:     # after gs_shutdown every handle is already gone
                self.h = 0
            else:
                check(rc)

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def __len__(self):
        return _count("gs_len", self)


def _count(name, h):
    n = ctypes.c_size_t(0)
    call(name, raw(h), ctypes.byref(n))
    return int(n.value)


def pk_eval_count(pk_handle):
    """gs_pk_eval_count: evaluation-basis points a resident Groth16 / Pinocchio key holds (0 = none)."""
    return _count("gs_pk_eval_count", pk_handle)


def pk_quot_count(pk_handle):
    """gs_pk_quot_count: quotient-basis points a resident Groth16 / Pinocchio key holds (0 = none: the h-sum divides px by Z)."""
    return _count("gs_pk_quot_count", pk_handle)


def _upload(name, arr, words):
    init()
    a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, words)
    cell = HandleCell()
    call(name, ptr64(a), a.shape[0], cell.ref)
    return cell.result()


def g1_upload(points_u64):
    return _upload("gs_g1_upload", points_u64, 12)


def g2_upload(points_u64):
    return _upload("gs_g2_upload", points_u64, 24)


def byte_ptr(buf):
    """A uint8 array of any alignment, writable or not (a memory-mapped file section) -> (void pointer, the array that keeps it alive)."""
    a = np.ascontiguousarray(buf).reshape(-1).view(np.uint8)
    return ctypes.c_void_p(a.ctypes.data if a.size else None), a


def _upload_affine_mont(name, buf, point_bytes):
    init()
    p, a = byte_ptr(buf)
    if a.size % point_bytes:
        raise ValueError("%s: %d bytes are not a whole number of %d-byte points" % (name, a.size, point_bytes))
    cell = HandleCell()
    call(name, p, a.size // point_bytes, cell.ref)
    return cell.result()


def g1_upload_affine_mont(buf):
    """gs_g1_upload_affine_mont: n x 64 bytes as a snarkjs .zkey holds G1 points -> a base-array handle."""
    return _upload_affine_mont("gs_g1_upload_affine_mont", buf, 64)


def g2_upload_affine_mont(buf):
    return _upload_affine_mont("gs_g2_upload_affine_mont", buf, 128)


def _download_affine_mont(name, handle, point_bytes, out, n):
    n = len(handle) if n is None else int(n)
    if out is None:
        out = np.zeros(n * point_bytes, dtype=np.uint8)
    a = out.reshape(-1).view(np.uint8) if isinstance(out, np.ndarray) else None
    if a is None or not a.flags.c_contiguous or not a.flags.writeable or a.size != n * point_bytes:
        raise ValueError("%s: the output must be a writable contiguous uint8 array of %d bytes" % (name, n * point_bytes))
    call(name, raw(handle), ctypes.c_void_p(a.ctypes.data if a.size else None), n)
    return out


def g1_download_affine_mont(handle, out=None, n=None):
    """gs_g1_download_affine_mont: the first n points (default: all) of a G1 base array as the n x 64 bytes a .zkey holds, into `out` (a
    writable uint8 array, e.g. a section of a memory-mapped output file) or a new array."""
    return _download_affine_mont("gs_g1_download_affine_mont", handle, 64, out, n)


def g2_download_affine_mont(handle, out=None, n=None):
    return _download_affine_mont("gs_g2_download_affine_mont", handle, 128, out, n)


def g1_lagrange(powers, log2_n, off=0, odd_half=False):
    """gs_g1_lagrange: the inverse transform of 2^log2_n points of `powers` from index `off`, in the group -> a base-array handle
    (odd_half: the odd entries of the transform of twice the size, from 2^(log2_n + 1) - 1 or 2^(log2_n + 1) points)."""
    cell = HandleCell()
    call("gs_g1_lagrange", raw(powers), int(off), int(log2_n), int(bool(odd_half)), cell.ref)
    return cell.result()


def g2_lagrange(powers, log2_n, off=0):
    cell = HandleCell()
    call("gs_g2_lagrange", raw(powers), int(off), int(log2_n), cell.ref)
    return cell.result()


def r1cs_colsum(r1cs, basis_a=None, basis_b=None, basis_c=None, g2=False):
    """gs_r1cs_colsum_g1 / _g2: out[s] = sum_j a_js Ba[j] + b_js Bb[j] + c_js Bc[j] over the rows j of a resident R1CS, for every
    variable s; None leaves a matrix out -> a base-array handle of nvars points."""
    cell = HandleCell()
    call("gs_r1cs_colsum_g2" if g2 else "gs_r1cs_colsum_g1", raw(r1cs), raw(basis_a), raw(basis_b), raw(basis_c), cell.ref)
    return cell.result()


def r1cs_check(r1cs, w, cap=16):
    """gs_r1cs_check: which of ALL n constraints of a resident three-matrix R1CS a resident witness breaks -> (count, the first
    min(cap, count) violated rows in ascending order, their (A w, B w, C w) as an [rows, 3, 4] uint64 array, canonical)."""
    cap = int(cap)
    if cap < 0:
        raise ValueError("gs_r1cs_check: cap = %d" % cap)
    count = ctypes.c_uint64(0)
    rows, values = np.zeros(cap, dtype=np.uint32), np.zeros((cap, 3, 4), dtype=np.uint64)
    call("gs_r1cs_check", raw(r1cs), raw(w), cap, ctypes.byref(count), ptr32(rows) if cap else None, ptr64(values) if cap else None)
    k = min(cap, int(count.value))
    return int(count.value), rows[:k], values[:k]


NO_FAILED_ROW = 0xFFFFFFFF


def r1cs_solve_plan(r1cs, input_vars, narrow=0, run_max_rows=0):
    """gs_r1cs_solve_plan: the level plan of a resident three-matrix R1CS for the given input variables -> (plan handle, SolveStats)."""
    iv = np.ascontiguousarray([int(v) for v in input_vars], dtype=np.uint32)
    opts, stats, cell = SolveOpts(int(narrow), int(run_max_rows)), SolveStats(), HandleCell()
    call("gs_r1cs_solve_plan", raw(r1cs), ptr32(iv) if iv.size else None, iv.size, ctypes.byref(opts), cell.ref, ctypes.byref(stats))
    return cell.result(), stats


def r1cs_solve_unsolved(plan):
    """gs_r1cs_solve_unsolved: the variables no row defines, ascending."""
    count = ctypes.c_uint64(0)
    call("gs_r1cs_solve_unsolved", raw(plan), 0, None, ctypes.byref(count))
    out = np.zeros(int(count.value), dtype=np.uint32)
    if out.size:
        call("gs_r1cs_solve_unsolved", raw(plan), out.size, ptr32(out), ctypes.byref(count))
    return [int(v) for v in out]


def r1cs_solve(plan, inputs, into=None):
    """gs_r1cs_solve: inputs = one list of integers (any value below 2^256, counted mod r) per witness, in the plan's input order;
    into = None, or one resident vector (or None) per witness to overwrite -> (handles, nfailed list, first_failed_row list with None
    for 'none')."""
    nwit = len(inputs)
    flat = [int(v) for row in inputs for v in row]
    iw = ints_to_u64(flat) if flat else np.zeros((1, 4), dtype=np.uint64)
    into = [None] * nwit if into is None else list(into)
    if len(into) != nwit:
        raise ValueError("gs_r1cs_solve: %d witnesses but %d vectors to overwrite" % (nwit, len(into)))
    handles = harr(into) if nwit else (Handle * 1)()
    nfailed, first = np.zeros(max(nwit, 1), dtype=np.uint64), np.zeros(max(nwit, 1), dtype=np.uint32)
    call("gs_r1cs_solve", raw(plan), nwit, ptr64(iw), handles, ptr64(nfailed), ptr32(first))
    out = [x if x is not None else DeviceHandle(handles[b]) for b, x in enumerate(into)]
    return out, [int(x) for x in nfailed[:nwit]], [None if int(x) == NO_FAILED_ROW else int(x) for x in first[:nwit]]


def g1_scale(bases, k):
    """gs_g1_scale: out[i] = k * P[i] -> a base-array handle."""
    cell = HandleCell()
    call("gs_g1_scale", raw(bases), ptr64(ints_to_u64([int(k) % R])), cell.ref)
    return cell.result()


def _scale_powers(name, bases, off, n, c, t):
    cell = HandleCell()
    ct = ints_to_u64([int(c) % (1 << 256), int(t) % (1 << 256)])       # any 256-bit value: the library reduces mod r
    call(name, raw(bases), int(off), int(n), ptr64(ct[0]), ptr64(ct[1]), cell.ref)
    return cell.result()


def g1_scale_powers(bases, off, n, c, t):
    """gs_g1_scale_powers: out[i] = (c * t^i mod r) * P[off + i], i < n -> a base-array handle (t^0 = 1 also for t = 0)."""
    return _scale_powers("gs_g1_scale_powers", bases, off, n, c, t)


def g2_scale_powers(bases, off, n, c, t):
    return _scale_powers("gs_g2_scale_powers", bases, off, n, c, t)


def _check_report(rep, names):
    """gs_check_report -> [(name, ok, lhs, rhs)] with the points as affine int tuples (None = infinity); the coefs checks carry the number
    of differing rows in place of a left point."""
    out = []
    for i in range(rep.nchecks):
        r = rep.check[i]
        side = lambda w, inf, g2: _affine_result(np.array(w[:16 if g2 else 8], dtype=np.uint64), [inf], bool(g2))      # noqa: E731
        if names[i].startswith("coefs"):
            out.append((names[i], bool(r.ok), int(r.lhs[0]), None))
        else:
            out.append((names[i], bool(r.ok), side(r.lhs, r.lhs_inf, r.lhs_g2), side(r.rhs, r.rhs_inf, r.rhs_g2)))
    return out


def groth16_key_check(a, b1, b2, ic, c, h, key_system, circuit_system, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, delta2, log2_domain, npublic,
                      challenge):
    """gs_groth16_key_check: the key's resident arrays and section-4 system against the circuit's system and the transcript's arrays, for
    the challenge s -> [(check name, ok, lhs, rhs)] in the order of KEY_CHECKS.  delta2: a Jacobian int triple."""
    inp = KeyCheckInput(*[raw(x) for x in (a, b1, b2, ic, c, h, key_system, circuit_system, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1)])
    inp.delta2[:] = [int(v) for v in g2_points_to_u64([delta2]).reshape(-1)]
    inp.challenge[:] = [int(v) for v in ints_to_u64([int(challenge) % (1 << 256)]).reshape(-1)]
    inp.log2_domain, inp.npublic = int(log2_domain), int(npublic)
    rep = CheckReport()
    call("gs_groth16_key_check", ctypes.byref(inp), ctypes.byref(rep))
    return _check_report(rep, KEY_CHECKS)


def ptau_check(tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, log2_n, challenge):
    """gs_ptau_check: the first 2^log2_n powers of a resident transcript against themselves -> [(check name, ok, lhs, rhs)] in the order
    of PTAU_CHECKS.  beta_g2: a Jacobian int triple."""
    rep = CheckReport()
    call("gs_ptau_check", raw(tau_g1), raw(tau_g2), raw(alpha_tau_g1), raw(beta_tau_g1), ptr64(g2_points_to_u64([beta_g2]).reshape(-1)), int(log2_n),
         ptr64(ints_to_u64([int(challenge) % (1 << 256)]).reshape(-1)), ctypes.byref(rep))
    return _check_report(rep, PTAU_CHECKS)


def _lagrange_levels(name, powers, lo, hi):
    cell = HandleCell()
    call(name, raw(powers), int(lo), int(hi), cell.ref)
    return cell.result()


def g1_lagrange_levels(powers, lo, hi):
    """gs_g1_lagrange_levels: the Lagrange bases of the domains 2^lo .. 2^hi over the first points of `powers`, every level's stage of one
    span in one launch -> a base-array handle of 2^(hi+1) - 2^lo points, level p at index 2^p - 2^lo (an array of exactly 2^hi - 1
    points: the missing last point of level hi is the point at infinity)."""
    return _lagrange_levels("gs_g1_lagrange_levels", powers, lo, hi)


def g2_lagrange_levels(powers, lo, hi):
    return _lagrange_levels("gs_g2_lagrange_levels", powers, lo, hi)


def _lagrange_levels_check(name, check_name, powers, levels, hi, challenge):
    rep = CheckReport()
    rep.nchecks = 1
    call(name, raw(powers), raw(levels), int(hi), ptr64(ints_to_u64([int(challenge) % (1 << 256)]).reshape(-1)), ctypes.byref(rep.check[0]))
    return _check_report(rep, (check_name,))[0]


def g1_lagrange_levels_check(powers, levels, hi, challenge, name="levels"):
    """gs_g1_lagrange_levels_check: are the first 2^(hi+1) - 1 points of `levels` the levels 0 .. hi of `powers`?  Two sums and a scalar
    transform, for the challenge s -> (name, ok, lhs, rhs), the points as affine int tuples (None = infinity)."""
    return _lagrange_levels_check("gs_g1_lagrange_levels_check", name, powers, levels, hi, challenge)


def g2_lagrange_levels_check(powers, levels, hi, challenge, name="levels"):
    return _lagrange_levels_check("gs_g2_lagrange_levels_check", name, powers, levels, hi, challenge)


def g2_subgroup_check(bases, off=0, n=None):
    """gs_g2_subgroup_check: which of the points off .. off + n - 1 of a resident G2 array (default: all from off on) lie outside the
    order-r subgroup?  -> (how many, the smallest index of one counted from the start of the array, or None when there is none).  The
    uploads test the curve equation only; exact and per point, the point at infinity is a member."""
    off = int(off)
    n = max(len(bases) - off, 0) if n is None else int(n)
    nbad, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
    call("gs_g2_subgroup_check", raw(bases), off, n, ctypes.byref(nbad), ctypes.byref(first))
    return int(nbad.value), (None if first.value == (1 << 64) - 1 else int(first.value))


POINT_LARGEST_Y, POINT_INFINITY = 1, 2          # GS_POINT_LARGEST_Y, GS_POINT_INFINITY


def _decompress(name, x_u64, flags, words):
    init()
    x = np.ascontiguousarray(x_u64, dtype=np.uint64).reshape(-1, words)
    f = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    if f.shape[0] != x.shape[0]:
        raise ValueError("%s: %d x coordinates, %d flag bytes" % (name, x.shape[0], f.shape[0]))
    n = x.shape[0]
    ok = np.zeros(max(n, 1), dtype=np.uint8)
    nbad, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
    cell = HandleCell()
    one = np.zeros(max(words, 1), dtype=np.uint64)           # n = 0 still hands over readable memory
    call(name, ptr64(x) if n else ptr64(one), (f if n else ok).ctypes.data_as(u8p), n, cell.ref, ok.ctypes.data_as(u8p), ctypes.byref(nbad),
         ctypes.byref(first))
    return cell.result(), ok[:n] != 0


def g1_decompress(x_u64, flags):
    """gs_g1_decompress: x coordinates ([n, 4] uint64, standard form) and flag bytes (POINT_LARGEST_Y: y is the larger of {y, q - y};
    POINT_INFINITY) -> (a G1 base-array handle of n points, a bool array: which entries decoded).  An entry that does not decode -- x >= q,
    x^3 + 3 not a square, an inconsistent flag -- is the point at infinity in the array; nothing is raised for it."""
    return _decompress("gs_g1_decompress", x_u64, flags, 4)


def g2_decompress(x_u64, flags):
    """gs_g2_decompress: the same over the twist, x as [n, 8] uint64 (c0 | c1), "larger" decided by c1 and by c0 only when c1 = 0.  The
    points are on the twist, NOT tested for membership of the order-r subgroup: g2_subgroup_check on the handle does that."""
    return _decompress("gs_g2_decompress", x_u64, flags, 8)


def _compress(name, handle, off, n, words):
    off = int(off)
    n = max(len(handle) - off, 0) if n is None else int(n)
    x, f = np.zeros((max(n, 1), words), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.uint8)
    call(name, raw(handle), off, n, ptr64(x), f.ctypes.data_as(u8p))
    return x[:n], f[:n]


def g1_compress(handle, off=0, n=None):
    """gs_g1_compress: the points off .. off + n - 1 (default: all from off on) of a resident G1 array -> (x as [n, 4] uint64 in standard
    form, flag bytes); a point at infinity gives x = 0 and POINT_INFINITY."""
    return _compress("gs_g1_compress", handle, off, n, 4)


def g2_compress(handle, off=0, n=None):
    return _compress("gs_g2_compress", handle, off, n, 8)


def pairing_product(g1, poff, g2, qoff, n):
    """gs_pairing_product: prod_i e(P[poff + i], Q[qoff + i]) over a resident G1 and a resident G2 array -> (the value as the 48 words
    of gs_pairing's encoding, whether it is one).  The Q must be in G2: g2_subgroup_check on the same handle is the caller's job."""
    out, one = np.zeros(48, dtype=np.uint64), ctypes.c_int(0)
    call("gs_pairing_product", raw(g1), int(poff), raw(g2), int(qoff), int(n), ptr64(out), ctypes.byref(one))
    return out, bool(one.value)


def pairing_each(g1, poff, g2, qoff, n):
    """gs_pairing_each: e(P[poff + i], Q[qoff + i]) for every i < n over a resident G1 and a resident G2 array, final exponentiation
    on the device -> (the values as an (n, 48) array of gs_pairing's encoding, a bool array: which are one).  Every value equals
    gs_pairing's bit for bit.  The Q must be in G2: g2_subgroup_check on the same handle is the caller's job."""
    n = int(n)
    out, one = np.zeros((n, 48), dtype=np.uint64), np.zeros(max(n, 1), dtype=np.intc)
    call("gs_pairing_each", raw(g1), int(poff), raw(g2), int(qoff), n, ptr64(out) if n else ptr64(np.zeros(48, dtype=np.uint64)),
         one.ctypes.data_as(intp))
    return out, one[:n] != 0


def groth16_vk_create(alpha_u64, beta_u64, gamma_u64, delta_u64, ic_u64):
    """gs_groth16_vk_create: the key's points as Jacobian word arrays (alpha [12], beta / gamma / delta [24], IC [nic, 12]) -> the
    DeviceHandle of a prepared verification key.  A key that cannot verify anything is refused (GosnarkHipError, the point is named)."""
    init()
    ic = np.ascontiguousarray(ic_u64, dtype=np.uint64).reshape(-1, 12)
    cell = HandleCell()
    call("gs_groth16_vk_create", *[ptr64(np.ascontiguousarray(v, dtype=np.uint64).reshape(-1)) for v in (alpha_u64, beta_u64, gamma_u64, delta_u64)],
         ptr64(ic) if ic.shape[0] else None, ic.shape[0], cell.ref)
    return cell.result()


def groth16_verify_each_keys(keys, key_of_proof, pub_u64, a_u64, b_u64, c_u64):
    """gs_groth16_verify_each_keys: prepared keys (whatever raw() takes), the key index of every proof, the signals of all proofs
    concatenated in proof order ([total, 4] uint64) and the proofs' points as [n, 12], [n, 24], [n, 12] Jacobian words ->
    (a bool array of n verdicts, the count of zeros)."""
    kop = np.ascontiguousarray(key_of_proof, dtype=np.uint32).reshape(-1)
    n = kop.shape[0]
    pub = np.ascontiguousarray(pub_u64, dtype=np.uint64).reshape(-1, 4)
    if pub.shape[0] == 0:
        pub = np.zeros((1, 4), dtype=np.uint64)
    a, b, c = [np.ascontiguousarray(v, dtype=np.uint64).reshape(-1, w) if n else np.zeros((1, w), dtype=np.uint64)
               for v, w in zip((a_u64, b_u64, c_u64), (12, 24, 12))]
    if a.shape[0] != max(n, 1) or b.shape[0] != max(n, 1) or c.shape[0] != max(n, 1):
        raise ValueError("gs_groth16_verify_each_keys: %d key indices, %d / %d / %d points" % (n, a.shape[0], b.shape[0], c.shape[0]))
    ok, nbad = np.zeros(max(n, 1), dtype=np.intc), ctypes.c_uint64(0)
    call("gs_groth16_verify_each_keys", harr(keys) if len(keys) else None, len(keys), ptr32(kop) if n else None, ptr64(pub), ptr64(a), ptr64(b),
         ptr64(c), n, ok.ctypes.data_as(intp), ctypes.byref(nbad))
    return ok[:n] != 0, int(nbad.value)


def scalars_upload(s_u64):
    return _upload("gs_scalars_upload", s_u64, 4)


def g1_fixed_base(s_u64):
    return _upload("gs_g1_fixed_base", s_u64, 4)


def g2_fixed_base(s_u64):
    return _upload("gs_g2_fixed_base", s_u64, 4)


def _download(name, handle, words):
    n = len(handle)
    out = np.zeros((n, words), dtype=np.uint64)
    call(name, raw(handle), ptr64(out), n)
    return out


def g1_download(handle):
    return _download("gs_g1_download", handle, 12)


def g2_download(handle):
    return _download("gs_g2_download", handle, 24)


def scalars_download(handle):
    return _download("gs_scalars_download", handle, 4)


def _affine_result(out, inf, g2):
    if inf[0]:
        return None
    v = u64_to_ints(out)
    return ((v[0], v[1]), (v[2], v[3])) if g2 else (v[0], v[1])


def _point_call(name, g2, *args):
    """One of the g1 / g2 twins `name` ({g} = the group) whose arguments end in one affine point and its infinity flag."""
    out, inf = result(16 if g2 else 8)
    call(name.format(g="g2" if g2 else "g1"), *args, ptr64(out), inf)
    return _affine_result(out, inf, g2)


def msm(bases, scalars_u64, off=0, g2=False):
    """sum_i scalars[i] * bases[off+i] -> affine (x, y) / ((x0,x1),(y0,y1)) ints, None = infinity."""
    s = np.ascontiguousarray(scalars_u64, dtype=np.uint64).reshape(-1, 4)
    return _point_call("gs_msm_{g}", g2, raw(bases), ptr64(s), off, s.shape[0])


def msm_resident(bases, scalars, n, off=0, soff=0, g2=False):
    return _point_call("gs_msm_{g}_resident", g2, raw(bases), off, raw(scalars), soff, n)


def sum_affine(points, g2=False):
    """points: list of affine tuples or None (infinity) -> affine sum."""
    arr, ia = affine_words(points, [g2] * len(points))
    return _point_call("gs_{g}_sum_affine", g2, ptr64(arr), ia, len(points))


def _timing(name, *args):
    t = Timing()
    call(name, *args, ctypes.byref(t))
    return {n: getattr(t, n) for n, _ in Timing._fields_}


def last_timing():
    return _timing("gs_last_timing")


def memory_query():
    """gs_memory_query: what the current logical device's GPU and this library hold (bytes)."""
    init()
    m = Memory()
    call("gs_memory_query", ctypes.byref(m))
    return {n: int(getattr(m, n)) for n, _ in Memory._fields_ if n != "reserved"}


def _u64_pair(name, *args):
    a, b = ctypes.c_uint64(0), ctypes.c_uint64(0)
    call(name, *args, ctypes.byref(a), ctypes.byref(b))
    return int(a.value), int(b.value)


def handle_bytes(h):
    """gs_handle_bytes -> (object bytes, window-table bytes) of one handle."""
    return _u64_pair("gs_handle_bytes", raw(h))


def release_tables(h):
    """gs_release_tables: drop the window tables of a key / base array (rebuilt on its next use)."""
    call("gs_release_tables", raw(h))


TABLE_POLICY = {"auto": 0, "always": 1, "never": 2}


def set_table_policy(policy):
    """gs_set_table_policy: "auto" (table-free until a base array's second use, then a build in instalments paid by the calls
    that follow), "always" (build inside the first call), "never" (table-free only).  Results never depend on it."""
    init()
    call("gs_set_table_policy", TABLE_POLICY[policy] if isinstance(policy, str) else int(policy))


def build_tables(h, route=0):
    """gs_build_tables: build the window tables of a key / base array now (blocking).  route: 0 all, 1 px routes only, 2 witness
    routes only."""
    call("gs_build_tables", raw(h), int(route))


def set_memory_limit(nbytes):
    """gs_set_memory_limit (development / test hook): cap on the device bytes the library may hold, 0 = none."""
    call("gs_set_memory_limit", int(nbytes))


def alloc_counters():
    """gs_alloc_counters -> (hipMalloc calls, hipFree calls) the library has made so far."""
    return _u64_pair("gs_alloc_counters")


def scalars_update(handle, s_u64):
    """gs_scalars_update: overwrite a resident scalar vector in place (same length) -- no allocation, no device-wide sync."""
    a = np.ascontiguousarray(s_u64, dtype=np.uint64).reshape(-1, 4)
    call("gs_scalars_update", raw(handle), ptr64(a), a.shape[0])


def trim():
    """gs_trim: drop the cached workspaces of the current logical device."""
    call("gs_trim")


def set_eval_basis(on):
    init()
    call("gs_set_eval_basis", 1 if on else 0)


def set_window_bits(c):
    init()
    call("gs_set_window_bits", int(c))


def zpoly(deg):
    """Z(x) = prod_{i=1}^{deg} (x - i) as a [deg+1, 4] uint64 array (gs_zpoly)."""
    init()
    out = np.zeros((deg + 1, 4), dtype=np.uint64)
    call("gs_zpoly", deg, ptr64(out))
    return out


def msm_begin(bases, scalars, n, off=0, soff=0, g2=False):
    """Enqueue one resident MSM (gs_msm_g1_begin / gs_msm_g2_begin) -> ticket; at most three operations outstanding per logical device."""
    t = ticket_cell()
    call("gs_msm_g2_begin" if g2 else "gs_msm_g1_begin", raw(bases), off, raw(scalars), soff, n, ctypes.byref(t))
    return (t.value, g2)


def ticket_cancel(ticket):
    """gs_ticket_cancel: abandon a pipelined operation (proof ticket, or the integer of an MSM ticket) without its result."""
    call("gs_ticket_cancel", ticket[0] if isinstance(ticket, tuple) else ticket)


def msm_end(ticket):
    return _point_call("gs_msm_end", ticket[1], ticket[0])


# ---- several logical devices / communicator (multi.hip) -------------------------------------------------
def _clone(name, handle, target, off, n):
    cell = HandleCell()
    call(name, raw(handle), off, len(handle) - off if n is None else n, int(target), cell.ref)
    return cell.result()


def scalars_clone(handle, target, off=0, n=None):
    return _clone("gs_scalars_clone", handle, target, off, n)


def g1_clone(handle, target, off=0, n=None):
    return _clone("gs_g1_clone", handle, target, off, n)


def g2_clone(handle, target, off=0, n=None):
    return _clone("gs_g2_clone", handle, target, off, n)


def scalars_scatter(full_handle, total, root, slice_handle=None):
    """gs_scalars_scatter (one process per GPU, communicator of comm_init_rank): the root's `total` scalars -> every rank's slice of
    the contiguous split.  full_handle is ignored on the other ranks (pass None)."""
    cell = HandleCell(slice_handle)
    call("gs_scalars_scatter", raw(full_handle), int(total), int(root), cell.ref)
    return cell.result()


def comm_unique_id():
    buf = (ctypes.c_uint8 * 128)()
    call("gs_comm_unique_id", buf)
    return bytes(buf)


def comm_init_rank(uid, nranks, rank):
    call("gs_comm_init_rank", (ctypes.c_uint8 * 128).from_buffer_copy(uid), int(nranks), int(rank))


def comm_init_local():
    call("gs_comm_init_local")


def comm_destroy():
    load_library().gs_comm_destroy()


def comm_info():
    nr, rk, loc, cnt = ctypes.c_int(0), ctypes.c_int(0), ctypes.c_int(0), ctypes.c_uint64(0)
    call("gs_comm_info", ctypes.byref(nr), ctypes.byref(rk), ctypes.byref(loc), ctypes.byref(cnt))
    return {"nranks": nr.value, "rank": rk.value, "local": bool(loc.value), "collectives": cnt.value}


def comm_allgather(block, nblocks_out, local_blocks=1):
    """bytes `block` (local_blocks consecutive blocks in local mode) -> bytes of all ranks' blocks."""
    per = len(block) // local_blocks
    send = (ctypes.c_uint8 * len(block)).from_buffer_copy(block)
    recv = (ctypes.c_uint8 * (per * nblocks_out))()
    call("gs_comm_allgather", send, per, recv)
    return bytes(recv)


def msm_multi(bases, scalars, g2=False):
    """One MSM over len(bases) logical devices (gs_msm_g1_multi / gs_msm_g2_multi) -> (affine point, used_rccl)."""
    out, inf = result(16 if g2 else 8)
    used = ctypes.c_int(0)
    call("gs_msm_g2_multi" if g2 else "gs_msm_g1_multi", harr(bases), harr(scalars), len(bases), ptr64(out), inf, ctypes.byref(used))
    return _affine_result(out, inf, g2), bool(used.value)


def msm_sharded(bases, scalars, g2=False):
    return _point_call("gs_msm_{g}_sharded", g2, raw(bases), raw(scalars))


def device_timing(logical):
    return _timing("gs_device_timing", int(logical))
