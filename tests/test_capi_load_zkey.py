"""CPU-side checks of the .zkey entry points: the library exports them, the ctypes binding knows them, and without a device they say
GS_ERR_NOT_INIT like every other compute call (nothing falls back to host code)."""
import ctypes

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi

NEW = ("gs_g1_upload_affine_mont", "gs_g2_upload_affine_mont", "gs_r1cs_upload_zkey", "gs_groth16_pk_create_domain")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_zkey_entry_points_are_exported_and_bound():
    lib = capi.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.EXPORTS and name in capi._SIGS
        assert getattr(lib, name).argtypes == capi._SIGS[name]
    from gosnark_amd import circom
    for name in ("ReadZkey", "ReadWtns", "WriteZkey", "WriteWtns", "UploadZkey", "VerificationKeyFromZkey", "ConvertProvingKey"):
        assert callable(getattr(circom, name))


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_zkey_entry_points_without_a_device():
    lib = capi.load_library()
    buf = np.zeros(128, dtype=np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    pts = np.zeros(24, dtype=np.uint64)
    for call in (lambda h: lib.gs_g1_upload_affine_mont(p, 1, ctypes.byref(h)),
                 lambda h: lib.gs_g2_upload_affine_mont(p, 1, ctypes.byref(h)),
                 lambda h: lib.gs_r1cs_upload_zkey(1, 3, p, 1, ctypes.byref(h)),
                 lambda h: lib.gs_groth16_pk_create_domain(1, 2, 3, 4, 5, capi.ptr64(pts), capi.ptr64(pts), capi.ptr64(pts), capi.ptr64(pts),
                                                           capi.ptr64(pts), 1, 3, 1, ctypes.byref(h))):
        h = capi.Handle(0)
        assert call(h) == -5 and h.value == 0                               # GS_ERR_NOT_INIT
        assert b"gs_init" in lib.gs_last_error()
