"""CPU-side checks of the device pairing product and the batch verifier: the library exports gs_pairing_product and
gs_groth16_verify_batch, the header declares them with the agreed prototypes, the ctypes binding and the Go binding know them, the C
driver exists; without a device both say GS_ERR_NOT_INIT and write nothing (nothing falls back to host code), an empty batch is
accepted without one; VerifyProofs takes the seed keyword."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import bn128, capi, groth16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRODUCT, BATCH = "gs_pairing_product", "gs_groth16_verify_batch"
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
    for name in (PRODUCT, BATCH):
        assert hasattr(lib, name) and name in capi.EXPORTS and name in capi._SIGS
        assert getattr(lib, name).argtypes == capi._SIGS[name]
        assert "C.%s(" % name in go
    assert capi._SIGS[PRODUCT] == [capi.Handle, S, capi.Handle, S, S, capi.u64p, capi.intp]
    assert capi._SIGS[BATCH] == [capi.u64p] * 5 + [S, capi.u64p, S, capi.u64p, capi.u64p, capi.u64p, S, capi.u64p, capi.intp]
    assert ("int gs_pairing_product(gs_handle g1, size_t poff, gs_handle g2, size_t qoff, size_t n, uint64_t out_fq12[48] , int* is_one );"
            in header)
    assert ("int gs_groth16_verify_batch(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24], "
            "const uint64_t vk_g2_delta[24], const uint64_t* vk_ic, size_t nic, const uint64_t* public_signals , size_t npublic, "
            "const uint64_t* pi_a , const uint64_t* pi_b , const uint64_t* pi_c , size_t nproofs, const uint64_t challenge[4], int* ok);"
            in header)
    assert "func PairingProduct(" in go and "func Groth16VerifyBatch(" in go
    assert "func VerifyProofs(" in open(os.path.join(ROOT, "go", "groth16hip", "groth16hip.go")).read()
    assert callable(capi.pairing_product) and callable(bn128.PairingProduct)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "PairingProduct" in integration and "Groth16VerifyBatch" in integration and "verify_batch.c" in integration
    assert os.path.exists(os.path.join(ROOT, "tests", "c", "verify_batch.c"))


def test_the_header_states_the_precondition_and_the_soundness():
    text = " ".join(open(os.path.join(ROOT, "include", "gosnark_hip.h")).read().replace("\n * ", " ").split())
    assert "PRECONDITION: the Q are in G2" in text and "gs_g2_subgroup_check on the same handle" in text
    assert "(nproofs - 1) / r" in text and "does not say WHICH proof is bad" in text


def test_verify_proofs_takes_a_seed():
    p = inspect.signature(groth16.VerifyProofs).parameters
    assert list(p) == ["vk", "proofs", "publicSignalsList", "seed"] and p["seed"].default is None
    assert "VerifyProof" in groth16.VerifyProofs.__doc__


def _batch_args(nproofs, challenge=(5, 0, 0, 0)):
    z = lambda n: np.zeros(max(n, 1), dtype=np.uint64)   # noqa: E731
    bufs = [z(12), z(24), z(24), z(24), z(12), z(4), z(12), z(24), z(12), np.array(challenge, dtype=np.uint64)]
    p = [capi.ptr64(b) for b in bufs]
    ok = ctypes.c_int(7)
    return bufs, (p[0], p[1], p[2], p[3], p[4], 1, p[5], 0, p[6], p[7], p[8], nproofs, p[9], ctypes.byref(ok)), ok


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_both_without_a_device():
    lib = capi.load_library()
    out, one = np.full(48, 7, dtype=np.uint64), ctypes.c_int(7)
    assert getattr(lib, PRODUCT)(1, 0, 2, 0, 1, capi.ptr64(out), ctypes.byref(one)) == -5          # GS_ERR_NOT_INIT
    assert b"gs_init" in lib.gs_last_error() and one.value == 7 and (out == 7).all()
    with pytest.raises(capi.GosnarkHipError) as e:
        capi.pairing_product(capi.DeviceHandle(0), 0, capi.DeviceHandle(0), 0, 1)
    assert e.value.code == -5
    bufs, args, ok = _batch_args(1)
    assert getattr(lib, BATCH)(*args) == -5
    assert b"gs_init" in lib.gs_last_error()


def test_an_empty_batch_is_accepted_without_a_device():
    lib = capi.load_library()
    bufs, args, ok = _batch_args(0)
    assert getattr(lib, BATCH)(*args) == 0 and ok.value == 1
    for challenge in ((0, 0, 0, 0), (1, 0, 0, 0)):                      # ... but not with a constant for a challenge
        bufs, args, ok = _batch_args(0, challenge)
        assert getattr(lib, BATCH)(*args) == -3 and ok.value == 7
