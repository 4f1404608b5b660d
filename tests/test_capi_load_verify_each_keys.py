"""CPU-side checks of the multi-key per-proof verifier: the library exports gs_groth16_vk_create and gs_groth16_verify_each_keys, the
header declares them with the agreed prototypes, the ctypes binding and the Go bindings know them, the C driver and its INTEGRATION.md
row exist and the cgo layer agrees with the header; without a device both say GS_ERR_NOT_INIT and leave every out-argument untouched
(nothing falls back to host code); an empty batch is accepted without a device, keys or handles; the Python front ends have the
documented signatures."""
import ctypes
import inspect
import os
import re
import sys

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CREATE, KEYS = "gs_groth16_vk_create", "gs_groth16_verify_each_keys"
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
    for name in (CREATE, KEYS):
        assert hasattr(lib, name) and name in capi.EXPORTS and name in capi._SIGS
        assert getattr(lib, name).argtypes == capi._SIGS[name]
        assert "C.%s(" % name in go
    assert capi._SIGS[CREATE] == [capi.u64p] * 5 + [S, ctypes.POINTER(capi.Handle)]
    assert capi._SIGS[KEYS] == [ctypes.POINTER(capi.Handle), S, capi.u32p] + [capi.u64p] * 4 + [S, capi.intp, ctypes.POINTER(ctypes.c_uint64)]
    assert ("int gs_groth16_vk_create(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24], "
            "const uint64_t vk_g2_delta[24], const uint64_t* vk_ic , size_t nic, gs_handle* out);" in header)
    assert ("int gs_groth16_verify_each_keys(const gs_handle* keys, size_t nkeys, const uint32_t* key_of_proof , const uint64_t* public_signals , "
            "const uint64_t* pi_a, const uint64_t* pi_b, const uint64_t* pi_c, size_t nproofs, int* ok_each, uint64_t* nbad );" in header)
    assert "func Groth16VkCreate(" in go and "func Groth16VerifyEachKeys(" in go
    hip = open(os.path.join(ROOT, "go", "groth16hip", "groth16hip.go")).read()
    assert "func PrepareVerificationKey(" in hip and "func VerifyProofsEachKeys(" in hip
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "Groth16VkCreate" in integration and "Groth16VerifyEachKeys" in integration and "verify_each_keys.c" in integration
    driver = open(os.path.join(ROOT, "tests", "c", "verify_each_keys.c")).read()
    assert CREATE + "(" in driver and KEYS + "(" in driver
    plan = os.path.join(ROOT, "go-snark-study_amd", "csrc", "verify_plan.h")
    assert os.path.exists(plan)
    for unit in ("verify.hip", "pairing_device.hip"):
        assert '#include "verify_plan.h"' in open(os.path.join(ROOT, "go-snark-study_amd", "csrc", unit)).read()


def test_the_cgo_layer_agrees_with_the_header():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_go_abi
    finally:
        sys.path.pop(0)
    errors, stats = check_go_abi.check()
    assert errors == [] and stats["unresolved_arguments"] == 0, (errors, stats)


def test_python_signatures():
    assert list(inspect.signature(groth16.PrepareVerificationKey).parameters) == ["vk"]
    assert list(inspect.signature(groth16.VerifyProofsEachKeys).parameters) == ["keys", "key_of_proof", "proofs", "publicSignalsList"]
    assert list(inspect.signature(groth16.VerifyProofsEachKeysCompressed).parameters) == ["keys", "key_of_proof", "blobs", "publicSignalsList", "codec"]
    assert list(inspect.signature(groth16.DeviceVk.__init__).parameters) == ["self", "handle", "npublic"]
    assert callable(capi.groth16_vk_create) and callable(capi.groth16_verify_each_keys)
    key = groth16.DeviceVk(None, 2)                                      # a length mismatch is found before any call: no device needed
    with pytest.raises(ValueError, match="proof 1"):
        groth16.VerifyProofsEachKeys([key], [0, 0], [groth16.Proof((0, 0, 0), ((0, 0), (0, 0), (0, 0)), (0, 0, 0))] * 2, [[1, 2], [1]])
    with pytest.raises(ValueError):
        groth16.VerifyProofsEachKeys([key], [0], [groth16.Proof((0, 0, 0), ((0, 0), (0, 0), (0, 0)), (0, 0, 0))] * 2, [[1, 2], [1, 2]])


def _keys_args(nproofs, nkeys):
    z = lambda n: np.zeros(max(n, 1), dtype=np.uint64)   # noqa: E731
    bufs = [z(4 * nproofs), z(12 * nproofs), z(24 * nproofs), z(12 * nproofs), np.zeros(max(nproofs, 1), dtype=np.uint32)]
    handles = (capi.Handle * max(nkeys, 1))(*([12345] * max(nkeys, 1)))
    ok, nbad = np.full(max(nproofs, 1), 7, dtype=np.intc), ctypes.c_uint64(77)
    args = (handles, nkeys, capi.ptr32(bufs[4]), capi.ptr64(bufs[0]), capi.ptr64(bufs[1]), capi.ptr64(bufs[2]), capi.ptr64(bufs[3]), nproofs,
            ok.ctypes.data_as(capi.intp), ctypes.byref(nbad))
    return bufs, handles, args, ok, nbad


def test_an_empty_batch_and_the_argument_errors_need_no_device():
    lib = capi.load_library()
    bufs, handles, args, ok, nbad = _keys_args(0, 0)
    assert getattr(lib, KEYS)(*args) == 0 and nbad.value == 0 and (ok == 7).all()
    assert getattr(lib, KEYS)(None, 0, None, None, None, None, None, 0, None, None) == 0
    bufs, handles, args, ok, nbad = _keys_args(0, 3)                      # handles are not looked at
    assert getattr(lib, KEYS)(*args) == 0 and nbad.value == 0
    bufs, handles, args, ok, nbad = _keys_args(2, 1)
    assert getattr(lib, KEYS)(*(args[:8] + (None, args[9]))) == -3 and nbad.value == 77        # a null verdict array
    assert getattr(lib, KEYS)(*((None,) + args[1:])) == -3 and nbad.value == 77 and (ok == 7).all()   # a null key array
    bufs[4][1] = 1                                                       # key_of_proof[1] = nkeys
    assert getattr(lib, KEYS)(*args) == -3 and nbad.value == 77 and (ok == 7).all()
    assert b"key_of_proof[1]" in lib.gs_last_error()
    bufs, handles, args, ok, nbad = _keys_args(2, 0)                      # proofs but no keys
    assert getattr(lib, KEYS)(*args) == -3 and nbad.value == 77 and (ok == 7).all()
    z = np.zeros(24, dtype=np.uint64)
    out = capi.Handle(77)
    p = capi.ptr64(z)
    assert getattr(lib, CREATE)(p, p, p, p, p, 0, ctypes.byref(out)) == -4 and out.value == 77                 # nic = 0
    assert getattr(lib, CREATE)(p, p, p, p, p, 1, None) == -3
    assert getattr(lib, CREATE)(None, p, p, p, p, 1, ctypes.byref(out)) == -3 and out.value == 77


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_without_a_device_nothing_is_written():
    lib = capi.load_library()
    bufs, handles, args, ok, nbad = _keys_args(3, 1)
    assert getattr(lib, KEYS)(*args) == -5                               # GS_ERR_NOT_INIT
    assert b"gs_init" in lib.gs_last_error() and (ok == 7).all() and nbad.value == 77
    z = np.zeros(24, dtype=np.uint64)
    out = capi.Handle(77)
    p = capi.ptr64(z)
    assert getattr(lib, CREATE)(p, p, p, p, p, 2, ctypes.byref(out)) == -5
    assert b"gs_init" in lib.gs_last_error() and out.value == 77
