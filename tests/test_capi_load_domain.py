"""CPU-side checks of the power-of-two domain entry points (snarkjs / circom keys): the library exports them, the ctypes binding
knows them, and without a device they say GS_ERR_NOT_INIT like every other compute call (nothing falls back to host code)."""
import ctypes

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi

NEW = ("gs_r1cs_upload_domain", "gs_groth16_pk_derive_eval_domain", "gs_groth16_pk_set_eval_domain")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_domain_entry_points_are_exported_and_bound():
    lib = capi.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.EXPORTS
    from gosnark_amd import circom
    assert gosnark_amd.circom is circom and callable(circom.UploadProvingKey) and callable(circom.GenerateProofs)


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_domain_entry_points_without_a_device():
    lib = capi.load_library()
    rp = np.zeros(3, dtype=np.uint32)
    cl = np.zeros(1, dtype=np.uint32)
    vl = np.zeros((1, 4), dtype=np.uint64)
    h = capi.Handle(0)
    st = lib.gs_r1cs_upload_domain(1, 2, 3, capi.ptr32(rp), capi.ptr32(cl), capi.ptr64(vl), capi.ptr32(rp), capi.ptr32(cl), capi.ptr64(vl),
                                   capi.ptr32(rp), capi.ptr32(cl), capi.ptr64(vl), ctypes.byref(h))
    assert st == -5 and h.value == 0                                        # GS_ERR_NOT_INIT
    assert lib.gs_groth16_pk_derive_eval_domain(capi.Handle(1), 2) == -5
    assert lib.gs_groth16_pk_set_eval_domain(capi.Handle(1), capi.Handle(2), 2) == -5
    assert b"gs_init" in lib.gs_last_error()
