"""CPU-side checks of the per-proof Pinocchio verifier: the library exports gs_pinocchio_verify_each, the header declares it with the
agreed prototype, the ctypes binding and the Go bindings know it, the C driver and its INTEGRATION.md row exist; without a device it says
GS_ERR_NOT_INIT and leaves its output buffers untouched (nothing falls back to host code), an empty batch and the argument errors need
none; VerifyProofsEach and VerifyProofsEachChecks have the agreed signatures and name each other."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, snark

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EACH = "gs_pinocchio_verify_each"
S = ctypes.c_size_t


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _flat(text):
    return " ".join(re.sub(r"/\*.*?\*/", " ", text, flags=re.S).split())


def test_it_is_exported_declared_and_bound():
    lib = capi.load_library()
    header = _flat(open(os.path.join(ROOT, "include", "gosnark_hip.h")).read())
    go = open(os.path.join(ROOT, "go", "gosnarkhip", "pairing_device.go")).read()
    assert hasattr(lib, EACH) and EACH in capi.EXPORTS and EACH in capi._SIGS
    assert getattr(lib, EACH).argtypes == capi._SIGS[EACH]
    assert capi._SIGS[EACH] == [capi.u64p] * 8 + [S, capi.u64p, S, capi.u64p, S, capi.intp, capi.intp, ctypes.POINTER(ctypes.c_uint64)]
    assert ("int gs_pinocchio_verify_each(const uint64_t vka[24], const uint64_t vkb[12], const uint64_t vkc[24], const uint64_t g1kbg[12], "
            "const uint64_t g2kbg[24], const uint64_t g2kg[24], const uint64_t vkz[24], const uint64_t* vk_ic , size_t nic, "
            "const uint64_t* public_signals , size_t npublic, const uint64_t* proofs , size_t nproofs, "
            "int* ok_each , int* failed_each , uint64_t* nbad );" in header)
    assert "C.%s(" % EACH in go and "func PinocchioVerifyEach(" in go
    assert "func VerifyProofsEach(" in open(os.path.join(ROOT, "go", "snarkhip", "snarkhip.go")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "PinocchioVerifyEach" in integration and "pinocchio_verify_each.c" in integration
    assert os.path.exists(os.path.join(ROOT, "tests", "c", "pinocchio_verify_each.c"))
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "%d entry points" % len(capi.EXPORTS) in readme and EACH in readme           # the counts follow the header


def test_signatures():
    assert list(inspect.signature(snark.VerifyProofsEach).parameters) == ["vk", "proofs", "publicSignalsList", "debug"]
    assert inspect.signature(snark.VerifyProofsEach).parameters["debug"].default is False
    assert list(inspect.signature(snark.VerifyProofsEachChecks).parameters) == ["vk", "proofs", "publicSignalsList"]
    assert "VerifyProofsEachChecks" in snark.VerifyProofsEach.__doc__ and "VerifyProofsEach" in snark.VerifyProofsEachChecks.__doc__
    assert "VerifyProofsEach" in snark.VerifyProof.__doc__ and "VerifyProofsEachChecks" in snark.VerifyProof.__doc__
    assert list(inspect.signature(snark.VerifyProof).parameters) == ["vk", "proof", "publicSignals", "debug"]


def _args(nproofs, nic=1, npublic=0):
    z = lambda n: np.zeros(max(n, 1), dtype=np.uint64)   # noqa: E731
    bufs = [z(24), z(12), z(24), z(12), z(24), z(24), z(24), z(12 * nic), z(4 * max(nproofs, 1) * max(npublic, 1)), z(108 * max(nproofs, 1))]
    p = [capi.ptr64(b) for b in bufs]
    ok, failed, nbad = np.full(max(nproofs, 1), 7, dtype=np.intc), np.full(max(nproofs, 1), 7, dtype=np.intc), ctypes.c_uint64(77)
    args = tuple(p[:8]) + (nic, p[8], npublic, p[9], nproofs, ok.ctypes.data_as(capi.intp), failed.ctypes.data_as(capi.intp), ctypes.byref(nbad))
    return bufs, args, ok, failed, nbad


def untouched(ok, failed, nbad):
    return (ok == 7).all() and (failed == 7).all() and nbad.value == 77


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_without_a_device_nothing_is_written():
    lib = capi.load_library()
    bufs, args, ok, failed, nbad = _args(3)
    assert getattr(lib, EACH)(*args) == -5                               # GS_ERR_NOT_INIT
    assert b"gs_init" in lib.gs_last_error() and untouched(ok, failed, nbad)
    with pytest.raises(Exception):
        snark.VerifyProofsEach(snark.Vk(IC=[(0, 0, 0)], Vka=((0, 0),) * 3, Vkb=(0, 0, 0), Vkc=((0, 0),) * 3, G1Kbg=(0, 0, 0), G2Kbg=((0, 0),) * 3,
                                        G2Kg=((0, 0),) * 3, Vkz=((0, 0),) * 3),
                               [snark.Proof(**{f: (((0, 0),) * 3 if f == "PiB" else (0, 0, 0)) for f in snark.Proof.FIELDS})], [[]])


def test_an_empty_batch_and_the_argument_errors_need_no_device():
    lib = capi.load_library()
    bufs, args, ok, failed, nbad = _args(0)
    assert getattr(lib, EACH)(*args) == 0 and nbad.value == 0 and (ok == 7).all() and (failed == 7).all()
    assert getattr(lib, EACH)(*(args[:13] + (None, None, None))) == 0   # nothing to write to
    assert snark.VerifyProofsEach(snark.Vk(IC=[(0, 0, 0)], Vka=((0, 0),) * 3, Vkb=(0, 0, 0), Vkc=((0, 0),) * 3, G1Kbg=(0, 0, 0), G2Kbg=((0, 0),) * 3,
                                           G2Kg=((0, 0),) * 3, Vkz=((0, 0),) * 3), [], []) == []
    bufs, args, ok, failed, nbad = _args(2, nic=1, npublic=1)            # nic < npublic + 1
    assert getattr(lib, EACH)(*args) == -4 and untouched(ok, failed, nbad)
    bufs, args, ok, failed, nbad = _args(2)
    assert getattr(lib, EACH)(*(args[:13] + (None,) + args[14:])) == -3 and untouched(ok, failed, nbad)      # a null verdict array
    assert getattr(lib, EACH)(*((None,) + args[1:])) == -3 and untouched(ok, failed, nbad)                   # a null key point
    assert getattr(lib, EACH)(*(args[:11] + (None,) + args[12:])) == -3 and untouched(ok, failed, nbad)      # null proofs
    try:
        assert lib.gs_verify_set_strict(1) == 0
        bufs, args, ok, failed, nbad = _args(2, nic=3, npublic=1)        # strict: nic != npublic + 1
        assert getattr(lib, EACH)(*args) == -4 and untouched(ok, failed, nbad)
    finally:
        lib.gs_verify_set_strict(0)
