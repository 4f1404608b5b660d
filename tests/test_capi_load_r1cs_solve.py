"""CPU-side checks of the witness solver: the library exports the four entry points, the header declares them, the ctypes binding and
the Go binding know them, the structs have the sizes the library says; without a device every call says GS_ERR_NOT_INIT and writes
nothing (there is no host fallback); SolveReport is host logic."""
import ctypes
import os

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom, groth16, r1csqap, snark

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("gs_r1cs_solve_plan", "gs_r1cs_solve_unsolved", "gs_r1cs_solve", "gs_solve_abi_sizes")


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_the_entry_points_are_exported_declared_and_bound():
    lib = capi.load_library()
    text = open(os.path.join(ROOT, "include", "gosnark_hip.h")).read()
    go = open(os.path.join(ROOT, "go", "gosnarkhip", "r1cs_solve.go")).read()
    for name in NAMES:
        assert hasattr(lib, name) and name in capi.EXPORTS and name in capi._SIGS
        assert getattr(lib, name).argtypes == capi._SIGS[name]
        assert "int %s(" % name in text and "C.%s(" % name in go
    assert capi._SIGS["gs_r1cs_solve"] == [capi.Handle, ctypes.c_size_t, capi.u64p, ctypes.POINTER(capi.Handle), capi.u64p, capi.u32p]
    assert "int gs_r1cs_solve(gs_handle plan, size_t nwit, const uint64_t* inputs" in text and "No host fallback" in text
    assert all("func %s(" % f in go for f in ("R1csSolvePlan", "R1csSolveUnsolved", "R1csSolve"))
    assert callable(r1csqap.DeviceR1CS.PlanSolve) and callable(r1csqap.SolvePlan.Solve) and callable(r1csqap.SolvePlan.unsolved)
    assert issubclass(circom.DeviceDomainR1CS, r1csqap.DeviceR1CS) and "PlanSolve" not in vars(circom.DeviceDomainR1CS)
    assert callable(groth16.GenerateProofsFromInputs) and callable(snark.GenerateProofsFromInputs)
    assert issubclass(r1csqap.SolveError, ValueError)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "R1csSolve" in integration and "r1cs_solve.c" in integration
    assert os.path.exists(os.path.join(ROOT, "tests", "c", "r1cs_solve.c"))


def test_struct_sizes_match_the_library():
    lib = capi.load_library()
    ob, sb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.gs_solve_abi_sizes(ctypes.byref(ob), ctypes.byref(sb)) == 0
    assert (ob.value, sb.value) == (ctypes.sizeof(capi.SolveOpts), ctypes.sizeof(capi.SolveStats)) == (8, 64)
    assert lib.gs_solve_abi_sizes(None, None) == 0


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_without_a_device_every_call_says_not_init_and_writes_nothing():
    lib = capi.load_library()
    plan, stats = capi.Handle(77), capi.SolveStats()
    ctypes.memset(ctypes.byref(stats), 0xEE, ctypes.sizeof(stats))
    iv = np.array([1], dtype=np.uint32)
    assert lib.gs_r1cs_solve_plan(1, capi.ptr32(iv), 1, None, ctypes.byref(plan), ctypes.byref(stats)) == -5      # GS_ERR_NOT_INIT
    assert b"gs_init" in lib.gs_last_error() and plan.value == 77 and stats.solved == 0xEEEEEEEEEEEEEEEE
    count, vars_ = ctypes.c_uint64(7), np.full(4, 9, dtype=np.uint32)
    assert lib.gs_r1cs_solve_unsolved(1, 4, capi.ptr32(vars_), ctypes.byref(count)) == -5 and count.value == 7 and (vars_ == 9).all()
    hs, nfailed, first = (capi.Handle * 2)(0, 5), np.full(2, 9, dtype=np.uint64), np.full(2, 9, dtype=np.uint32)
    inputs = capi.ints_to_u64([3, 4])
    assert lib.gs_r1cs_solve(1, 2, capi.ptr64(inputs), hs, capi.ptr64(nfailed), capi.ptr32(first)) == -5
    assert list(hs) == [0, 5] and (nfailed == 9).all() and (first == 9).all()
    with pytest.raises(capi.GosnarkHipError) as e:
        capi.r1cs_solve_plan(capi.DeviceHandle(0), [1])
    assert e.value.code == -5


def test_solve_report_truthiness_and_repr():
    good = r1csqap.SolveReport([], [0, 0], [None, None])
    assert good and repr(good) == "SolveReport(2 witnesses solved)"
    partly = r1csqap.SolveReport([4, 9], [0], [None])
    assert not partly and "2 variables unsolved" in repr(partly)
    failed = r1csqap.SolveReport([], [0, 2], [None, 7])
    assert not failed and "witnesses [1]" in repr(failed)
    err = r1csqap.SolveError(failed)
    assert err.report is failed and isinstance(err, ValueError)
