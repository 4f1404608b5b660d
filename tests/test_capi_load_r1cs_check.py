"""CPU-side checks of the witness check: the library exports gs_r1cs_check, the header declares it, the ctypes binding and the Go binding
know it; without a device it says GS_ERR_NOT_INIT and writes nothing (there is no host fallback); WitnessReport and its explain are
host logic over a parsed circuit; CheckWtns refuses a witness of the wrong length before it touches the device."""
import ctypes
import os

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom, groth16, r1csqap, snark

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "gs_r1cs_check"
R = capi.R


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_r1cs_check_is_exported_declared_and_bound():
    lib = capi.load_library()
    text = open(os.path.join(ROOT, "include", "gosnark_hip.h")).read()
    read = lambda *p: open(os.path.join(ROOT, "go", *p)).read()              # noqa: E731
    assert hasattr(lib, NAME) and NAME in capi.EXPORTS and NAME in capi._SIGS
    assert getattr(lib, NAME).argtypes == capi._SIGS[NAME]
    assert capi._SIGS[NAME] == [capi.Handle, capi.Handle, ctypes.c_size_t, capi.u64p, capi.u32p, capi.u64p]
    assert "int %s(gs_handle r1cs, gs_handle w, size_t cap, uint64_t* nviolated, uint32_t* rows" % NAME in text
    assert "all n rows" in text and "roots of the KEY's Z" in text
    go = read("gosnarkhip", "r1cs.go")
    assert "C.%s(" % NAME in go and "func R1csCheck(" in go
    assert "func CheckWitness(" in read("r1csqaphip", "r1csqaphip.go")
    assert "func GenerateProofsChecked(" in read("groth16hip", "groth16hip.go") and "func GenerateProofsChecked(" in read("snarkhip", "snarkhip.go")
    assert callable(capi.r1cs_check) and callable(r1csqap.DeviceR1CS.CheckWitness) and callable(circom.CheckWtns)
    assert all(callable(mod.GenerateProofsChecked) for mod in (groth16, snark, circom))
    assert issubclass(circom.DeviceDomainR1CS, r1csqap.DeviceR1CS) and "CheckWitness" not in vars(circom.DeviceZkeyR1CS)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "R1csCheck" in integration and "r1cs_check.c" in integration
    assert os.path.exists(os.path.join(ROOT, "tests", "c", "r1cs_check.c"))


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_r1cs_check_without_a_device():
    lib = capi.load_library()
    count = ctypes.c_uint64(7)
    rows, values = np.full(4, 9, dtype=np.uint32), np.full((4, 3, 4), 9, dtype=np.uint64)
    assert getattr(lib, NAME)(1, 2, 4, ctypes.byref(count), capi.ptr32(rows), capi.ptr64(values)) == -5      # GS_ERR_NOT_INIT
    assert b"gs_init" in lib.gs_last_error() and count.value == 7 and (rows == 9).all() and (values == 9).all()
    with pytest.raises(capi.GosnarkHipError) as e:
        capi.r1cs_check(capi.DeviceHandle(0), capi.DeviceHandle(0), 4)
    assert e.value.code == -5


def hand_built():
    """Two constraints over wires [one, x, y, z]: (2 x + 3 one) * y = z and x * x = y, the first with x named twice in A (1 + 1)."""
    cons = [([(1, 1), (0, 3), (1, 1)], [(2, 1)], [(3, 1)]), ([(1, R + 1)], [(1, 1)], [(2, 1)])]
    csr = []
    for k in range(3):
        rp = np.cumsum([0] + [len(c[k]) for c in cons]).astype(np.uint32)
        col = np.array([s for c in cons for s, _ in c[k]], dtype=np.uint32)
        csr.append((rp, col, capi.ints_to_u64([v for c in cons for _, v in c[k]])))
    return circom.R1cs(4, 0, 1, 2, 4, 2, *csr), cons


def test_witness_report_truthiness_repr_and_explain():
    r1cs, cons = hand_built()
    good = r1csqap.WitnessReport(0, [], [])
    assert good and good.count == 0 and repr(good) == "WitnessReport(every constraint satisfied)"
    w = [1, 5, 25, 326]                                            # (2 * 5 + 3) * 25 = 325: the first constraint is broken
    bad = r1csqap.WitnessReport(1, np.array([0], dtype=np.uint32), [(13, 25, 326)], witness=w)
    assert not bad and bad.rows == [0] and bad.values == [(13, 25, 326)] and repr(bad) == "WitnessReport(1 violated: rows 0)"
    assert bad.explain(0, r1cs) == ([(1, 1, 5), (0, 3, 1), (1, 1, 5)], [(2, 1, 25)], [(3, 1, 326)])
    a, b, c = bad.explain(0, r1cs)
    assert tuple(sum(k * x for _, k, x in lc) % R for lc in (a, b, c)) == bad.values[0]
    many = r1csqap.WitnessReport(40, list(range(0, 32, 2)), [(0, 0, 1)] * 16)
    assert repr(many) == "WitnessReport(40 violated: rows 0, 2, 4, 6, 8, 10, 12, 14, ...)"
    # the witness as the limb array of a .wtns file, values and coefficients reduced mod r
    both = r1csqap.WitnessReport(2, [0, 1], [(13, 25, 326), (5, 5, 26)], witness=capi.ints_to_u64([1, 5 + R, 26, 326]))
    assert both.explain(1, r1cs) == ([(1, 1, 5)], [(1, 1, 5)], [(2, 1, 26)])
    resident = r1csqap.WitnessReport(1, [1], [(5, 5, 26)])
    with pytest.raises(ValueError):
        resident.explain(0, r1cs)
    assert resident.explain(0, r1cs, w=[1, 5, 26, 0])[2] == [(2, 1, 26)]
    err = r1csqap.WitnessError(bad)
    assert err.report is bad and "1 constraint" in str(err) and isinstance(err, ValueError)


def test_check_wtns_refuses_a_witness_of_another_length(tmp_path):
    _, cons = hand_built()
    r1cs_path, wtns_path = str(tmp_path / "c.r1cs"), str(tmp_path / "w.wtns")
    circom.WriteR1cs(r1cs_path, 4, 0, 1, 2, cons)
    circom.WriteWtns(wtns_path, [1, 5, 25, 325, 7])
    with pytest.raises(ValueError) as e:
        circom.CheckWtns(r1cs_path, wtns_path)
    assert "5" in str(e.value) and "nWires = 4" in str(e.value)
