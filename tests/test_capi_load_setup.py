"""CPU-side checks of the entry points of the setup from a transcript: the library exports them, the ctypes binding knows them, and
without a device they say GS_ERR_NOT_INIT like every other compute call (nothing falls back to host code)."""
import ctypes

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi

NEW = ("gs_g1_lagrange", "gs_g2_lagrange", "gs_r1cs_colsum_g1", "gs_r1cs_colsum_g2", "gs_g1_scale", "gs_g1_download_affine_mont",
       "gs_g2_download_affine_mont")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_setup_entry_points_are_exported_and_bound():
    lib = capi.load_library()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.EXPORTS and name in capi._SIGS
        assert getattr(lib, name).argtypes == capi._SIGS[name]
    for name in ("g1_lagrange", "g2_lagrange", "r1cs_colsum", "g1_scale", "g1_download_affine_mont", "g2_download_affine_mont"):
        assert callable(getattr(capi, name))
    from gosnark_amd import circom
    for name in ("ReadR1cs", "WriteR1cs", "ReadPtau", "WritePtau", "SetupFromPtau", "ContributeDelta"):
        assert callable(getattr(circom, name))


def test_header_declares_the_setup_entry_points():
    import os
    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gosnark_hip.h")).read()
    for name in NEW:
        assert "int %s(" % name in text


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_setup_entry_points_without_a_device():
    lib = capi.load_library()
    buf = np.zeros(128, dtype=np.uint8)
    p = ctypes.c_void_p(buf.ctypes.data)
    k = np.ones(4, dtype=np.uint64)
    for call in (lambda h: lib.gs_g1_lagrange(1, 0, 1, 0, ctypes.byref(h)),
                 lambda h: lib.gs_g1_lagrange(1, 0, 1, 1, ctypes.byref(h)),
                 lambda h: lib.gs_g2_lagrange(1, 0, 1, ctypes.byref(h)),
                 lambda h: lib.gs_r1cs_colsum_g1(1, 2, 0, 0, ctypes.byref(h)),
                 lambda h: lib.gs_r1cs_colsum_g2(1, 0, 2, 0, ctypes.byref(h)),
                 lambda h: lib.gs_g1_scale(1, capi.ptr64(k), ctypes.byref(h)),
                 lambda h: lib.gs_g1_download_affine_mont(1, p, 1),
                 lambda h: lib.gs_g2_download_affine_mont(1, p, 1)):
        h = capi.Handle(0)
        assert call(h) == -5 and h.value == 0                               # GS_ERR_NOT_INIT
        assert b"gs_init" in lib.gs_last_error()
    assert not buf.any()
