"""CPU-side checks of gs_pairing_each: the library exports it, the header declares it with the agreed prototype and states the
precondition, the ctypes binding and the Go binding know it, the C driver and its INTEGRATION.md row exist; without a device it says
GS_ERR_NOT_INIT and writes nothing (nothing falls back to host code)."""
import ctypes
import os
import re

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import bn128, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EACH = "gs_pairing_each"
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
    raw = open(os.path.join(ROOT, "include", "gosnark_hip.h")).read()
    go = open(os.path.join(ROOT, "go", "gosnarkhip", "pairing_device.go")).read()
    assert hasattr(lib, EACH) and EACH in capi.EXPORTS and EACH in capi._SIGS
    assert getattr(lib, EACH).argtypes == capi._SIGS[EACH]
    assert capi._SIGS[EACH] == [capi.Handle, S, capi.Handle, S, S, capi.u64p, capi.intp]
    assert ("int gs_pairing_each(gs_handle g1, size_t poff, gs_handle g2, size_t qoff, size_t n, uint64_t* out_fq12 , int* is_one );"
            in _flat(raw))
    assert "C.%s(" % EACH in go and "func PairingEach(" in go
    assert callable(capi.pairing_each) and callable(bn128.PairingEach)
    text = " ".join(raw.replace("\n * ", " ").split())
    assert "PRECONDITION (gs_pairing_product's): the Q are in G2" in text and "equal bit for bit to gs_pairing on that pair" in text
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "PairingEach" in integration and "pairing_each.c" in integration
    assert os.path.exists(os.path.join(ROOT, "tests", "c", "pairing_each.c"))


def test_the_final_exponentiation_is_device_source():
    """The kernel's tower is the header the host test instantiates, and the Frobenius constants come from the generator."""
    unit = open(os.path.join(ROOT, "go-snark-study_amd", "csrc", "pairing_device.hip")).read()
    assert '#include "finalexp.h"' in unit and "k_final_exp" in unit and "k_miller_each" in unit
    assert "frob(int row, int i)" in open(os.path.join(ROOT, "go-snark-study_amd", "csrc", "bn128_constants.h")).read()


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_without_a_device():
    lib = capi.load_library()
    out, one = np.full((2, 48), 7, dtype=np.uint64), np.full(2, 7, dtype=np.intc)
    assert getattr(lib, EACH)(1, 0, 2, 0, 2, capi.ptr64(out), one.ctypes.data_as(capi.intp)) == -5          # GS_ERR_NOT_INIT
    assert b"gs_init" in lib.gs_last_error() and (one == 7).all() and (out == 7).all()
    with pytest.raises(capi.GosnarkHipError) as e:
        capi.pairing_each(capi.DeviceHandle(0), 0, capi.DeviceHandle(0), 0, 1)
    assert e.value.code == -5
