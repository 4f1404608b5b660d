"""CPU-side checks of the per-proof verifier: the library exports gs_groth16_verify_each and gs_pairing_each, the header declares them
with the agreed prototypes, the ctypes binding and the Go bindings know them, the C driver and its INTEGRATION.md row exist; without a
device both say GS_ERR_NOT_INIT and leave their output buffers untouched (nothing falls back to host code), an empty batch is accepted
without one; VerifyProofsEach has the agreed signature and VerifyProofs keeps its own."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EACH, PAIRS = "gs_groth16_verify_each", "gs_pairing_each"
S = ctypes.c_size_t


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _flat(text):
    return " ".join(re.sub(r"/\*.*?\*/", " ", text, flags=re.S).split())


def test_both_are_exported_declared_and_bound():
    lib = capi.load_library()
    header = _flat(open(os.path.join(ROOT, "include", "gosnark_hip.h")).read())
    go = open(os.path.join(ROOT, "go", "gosnarkhip", "pairing_device.go")).read()
    for name in (EACH, PAIRS):
        assert hasattr(lib, name) and name in capi.EXPORTS and name in capi._SIGS
        assert getattr(lib, name).argtypes == capi._SIGS[name]
        assert "C.%s(" % name in go
    assert capi._SIGS[EACH] == [capi.u64p] * 5 + [S, capi.u64p, S, capi.u64p, capi.u64p, capi.u64p, S, capi.intp, ctypes.POINTER(ctypes.c_uint64)]
    assert ("int gs_pairing_each(gs_handle g1, size_t poff, gs_handle g2, size_t qoff, size_t n, uint64_t* out_fq12 , int* is_one );" in header)
    assert ("int gs_groth16_verify_each(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24], "
            "const uint64_t vk_g2_delta[24], const uint64_t* vk_ic, size_t nic, const uint64_t* public_signals , size_t npublic, "
            "const uint64_t* pi_a, const uint64_t* pi_b, const uint64_t* pi_c, size_t nproofs, int* ok_each , uint64_t* nbad );" in header)
    assert "func PairingEach(" in go and "func Groth16VerifyEach(" in go
    assert "func VerifyProofsEach(" in open(os.path.join(ROOT, "go", "groth16hip", "groth16hip.go")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Groth16VerifyEach" in integration and "verify_each.c" in integration
    assert os.path.exists(os.path.join(ROOT, "tests", "c", "verify_each.c"))


def test_signatures():
    p = inspect.signature(groth16.VerifyProofsEach).parameters
    assert list(p) == ["vk", "proofs", "publicSignalsList"]
    assert "VerifyProofs" in groth16.VerifyProofsEach.__doc__ and "VerifyProofsEach" in groth16.VerifyProofs.__doc__
    assert list(inspect.signature(groth16.VerifyProofs).parameters) == ["vk", "proofs", "publicSignalsList", "seed"]


def _args(nproofs, nic=1, npublic=0):
    z = lambda n: np.zeros(max(n, 1), dtype=np.uint64)   # noqa: E731
    bufs = [z(12), z(24), z(24), z(24), z(12 * nic), z(4), z(12), z(24), z(12)]
    p = [capi.ptr64(b) for b in bufs]
    ok, nbad = np.full(max(nproofs, 1), 7, dtype=np.intc), ctypes.c_uint64(77)
    return bufs, (p[0], p[1], p[2], p[3], p[4], nic, p[5], npublic, p[6], p[7], p[8], nproofs, ok.ctypes.data_as(capi.intp), ctypes.byref(nbad)), ok, nbad


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_without_a_device_nothing_is_written():
    lib = capi.load_library()
    bufs, args, ok, nbad = _args(3)
    assert getattr(lib, EACH)(*args) == -5                               # GS_ERR_NOT_INIT
    assert b"gs_init" in lib.gs_last_error() and (ok == 7).all() and nbad.value == 77
    out, one = np.full((2, 48), 7, dtype=np.uint64), np.full(2, 7, dtype=np.intc)
    assert getattr(lib, PAIRS)(1, 0, 2, 0, 2, capi.ptr64(out), one.ctypes.data_as(capi.intp)) == -5
    assert (one == 7).all() and (out == 7).all()


def test_an_empty_batch_and_the_shape_errors_need_no_device():
    lib = capi.load_library()
    bufs, args, ok, nbad = _args(0)
    assert getattr(lib, EACH)(*args) == 0 and nbad.value == 0 and (ok == 7).all()
    bufs, args, ok, nbad = _args(2, nic=1, npublic=1)                    # nic < npublic + 1
    assert getattr(lib, EACH)(*args) == -4 and nbad.value == 77 and (ok == 7).all()
    bufs, args, ok, nbad = _args(2)
    assert getattr(lib, EACH)(*(args[:12] + (None, args[13]))) == -3 and nbad.value == 77      # a null verdict array
    try:
        assert lib.gs_verify_set_strict(1) == 0
        bufs, args, ok, nbad = _args(2, nic=3, npublic=1)                # strict: nic != npublic + 1
        assert getattr(lib, EACH)(*args) == -4 and nbad.value == 77 and (ok == 7).all()
    finally:
        lib.gs_verify_set_strict(0)
