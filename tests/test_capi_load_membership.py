"""CPU-side checks of the G2 membership test: the library exports gs_g2_subgroup_check, the header declares it, the ctypes binding and the
Go binding know it; without a device it says GS_ERR_NOT_INIT (nothing falls back to host code); the three verifiers take the keyword and
default it to False; and a report with appended membership checks names the failed one."""
import ctypes
import inspect
import os

import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gs_g2_subgroup_check"


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_subgroup_check_is_exported_declared_and_bound():
    lib = capi.load_library()
    text = open(os.path.join(ROOT, "include", "gosnark_hip.h")).read()
    go = open(os.path.join(ROOT, "go", "gosnarkhip", "g2_membership.go")).read()
    assert hasattr(lib, NAME) and NAME in capi.EXPORTS and NAME in capi._SIGS
    assert getattr(lib, NAME).argtypes == capi._SIGS[NAME]
    assert capi._SIGS[NAME] == [capi.Handle, ctypes.c_size_t, ctypes.c_size_t, capi.u64p, capi.u64p]
    assert "int %s(gs_handle points, size_t off, size_t n, uint64_t* nbad, uint64_t* first_bad);" % NAME in text
    assert "C.%s(" % NAME in go and "func G2SubgroupCheck(" in go
    assert callable(capi.g2_subgroup_check)
    assert "G2SubgroupCheck" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tests", "c", "g2_membership.c"))


def test_verifiers_take_membership_and_default_it_to_false():
    for f in (circom.VerifyPtau, circom.VerifyPtauPrepared, circom.VerifyZkey):
        p = inspect.signature(f).parameters
        assert "membership" in p and p["membership"].default is False
    assert capi.CHECK_MAX == 8 and len(capi.KEY_CHECKS) == 8 and len(capi.PTAU_CHECKS) == 8 and len(circom.PTAU_PREPARED_CHECKS) == 4


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_subgroup_check_without_a_device():
    lib = capi.load_library()
    nbad, first = ctypes.c_uint64(7), ctypes.c_uint64(7)
    assert getattr(lib, NAME)(1, 0, 1, ctypes.byref(nbad), ctypes.byref(first)) == -5      # GS_ERR_NOT_INIT
    assert b"gs_init" in lib.gs_last_error() and (nbad.value, first.value) == (7, 7)
    with pytest.raises(capi.GosnarkHipError) as e:
        capi.g2_subgroup_check(capi.DeviceHandle(0), 0, 1)
    assert e.value.code == -5


def test_report_with_appended_membership_checks():
    """Host logic: (name, ok, nbad, first_bad) rows behind the pinned ones."""
    base = [(n, True, (1, 2), (1, 2)) for n in capi.PTAU_CHECKS]
    good = circom.PtauReport(base + [("tauG2 membership", True, 0, None)], 5)
    assert good and good.failed == [] and repr(good) == "PtauReport(all 9 checks passed)"
    assert good.points["tauG2 membership"] == (0, None)
    bad = circom.PtauReport(base + [("tauG2 membership", False, 2, 17)], 5)
    assert not bad and bad.failed == ["tauG2 membership"] and repr(bad) == "PtauReport(FAILED: tauG2 membership)"
    assert bad.points["tauG2 membership"] == (2, 17)
    assert [c[0] for c in bad.checks[:8]] == list(capi.PTAU_CHECKS)
    key = circom.ZkeyReport([("header", True, None, None), ("delta", True, None, None)] + [(n, True, None, None) for n in capi.KEY_CHECKS]
                            + [("tauG2 membership", True, 0, None), ("B2 membership", False, 1, 3)], 5)
    assert not key and key.failed == ["B2 membership"] and repr(key) == "ZkeyReport(FAILED: B2 membership)"
