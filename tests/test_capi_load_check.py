"""CPU-side checks of the key and transcript checks: the library exports the entry points, the header declares them, the ctypes binding
knows them and its structs have the library's sizes; without a device they say GS_ERR_NOT_INIT (nothing falls back to host code); and
the ValueErrors of circom.VerifyZkey / VerifyPtau -- files that do not fit each other -- are raised before the device is touched."""
import ctypes
import os
import struct

import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom, groth16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_groth16_key_check", "gs_ptau_check", "gs_check_abi_sizes")
G1, G2 = circom.G1_GEN, circom.G2_GEN


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_check_entry_points_are_exported_declared_and_bound():
    lib = capi.load_library()
    text = open(os.path.join(ROOT, "include", "gosnark_hip.h")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.EXPORTS and name in capi._SIGS
        assert getattr(lib, name).argtypes == capi._SIGS[name]
        assert "int %s(" % name in text
    go = open(os.path.join(ROOT, "go", "gosnarkhip", "zkey_check.go")).read()
    for name in NEW:
        assert "C.%s(" % name in go
    for name in ("groth16_key_check", "ptau_check"):
        assert callable(getattr(capi, name))
    for name in ("VerifyZkey", "VerifyPtau", "ZkeyReport", "PtauReport"):
        assert callable(getattr(circom, name))
    assert len(capi.KEY_CHECKS) == len(capi.PTAU_CHECKS) == capi.CHECK_MAX == 8


def test_the_structs_have_the_librarys_sizes():
    lib = capi.load_library()
    a, b = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert lib.gs_check_abi_sizes(ctypes.byref(a), ctypes.byref(b)) == 0
    assert (a.value, b.value) == (ctypes.sizeof(capi.KeyCheckInput), ctypes.sizeof(capi.CheckReport))
    assert ctypes.sizeof(capi.CheckResult) == 24 + 2 * 128 and b.value == 8 + 8 * ctypes.sizeof(capi.CheckResult)
    assert lib.gs_check_abi_sizes(None, None) == 0


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_check_entry_points_without_a_device():
    lib = capi.load_library()
    rep, inp = capi.CheckReport(), capi.KeyCheckInput()
    inp.a = 1
    words = capi.ints_to_u64([1] * 6).reshape(-1)
    s = capi.ints_to_u64([5]).reshape(-1)
    for status in (lib.gs_groth16_key_check(ctypes.byref(inp), ctypes.byref(rep)),
                   lib.gs_ptau_check(1, 2, 3, 4, capi.ptr64(words), 3, capi.ptr64(s), ctypes.byref(rep))):
        assert status == -5 and b"gs_init" in lib.gs_last_error()             # GS_ERR_NOT_INIT
    assert rep.nchecks == 0 and rep.failed == 0
    with pytest.raises(capi.GosnarkHipError) as e:
        capi.ptau_check(capi.DeviceHandle(0), 2, 3, 4, G2, 3, 5)
    assert e.value.code == -5
    with pytest.raises(capi.GosnarkHipError) as e:
        capi.groth16_key_check(*range(1, 13), G2, 3, 1, 5)
    assert e.value.code == -5


def test_reports_are_truthy_only_when_every_check_passed():
    good = circom.ZkeyReport([("header", True, None, None), ("A", True, (1, 2), (1, 2))], 7)
    bad = circom.PtauReport([("g1", True, (1, 2), (1, 2)), ("tauG1", False, (1, 2), None), ("betaG2", False, None, None)], 7)
    assert good and not bad and good.failed == [] and bad.failed == ["tauG1", "betaG2"]
    assert bad.points["tauG1"] == ((1, 2), None) and good.seed == 7
    assert "tauG1, betaG2" in repr(bad) and "all 2 checks passed" in repr(good)


# ---- files written without a device: a transcript of tau = alpha = beta = 1 (every point is the generator), a key of infinities ----
def _write_ptau(path, power):
    n = 1 << power
    g1, g2 = circom.G1ToZkey(G1), circom.G2ToZkey(G2)
    head = struct.pack("<I", 32) + circom.Q.to_bytes(32, "little") + struct.pack("<II", power, power)
    secs = [(1, head), (2, g1 * (2 * n - 1)), (3, g2 * n), (4, g1 * n), (5, g1 * n), (6, g2)]
    with open(path, "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, len(secs)))
        for sid, payload in secs:
            f.write(struct.pack("<IQ", sid, len(payload)) + payload)


def _write_zkey(path, nvars, npublic, k):
    inf1, inf2 = circom.G1_INF, circom.G2_INF
    rows = [dict() for _ in range(1 << k)]
    pkj = circom.ProvingKey(nvars, npublic, k, rows, rows, rows, [inf1] * nvars, [inf1] * nvars, [inf2] * nvars, [inf1] * nvars, [], G1, G1, G1, G2, G2)
    vk = groth16.Vk(IC=[inf1] * (npublic + 1), G1_Alpha=G1, G2_Beta=G2, G2_Gamma=G2, G2_Delta=G2)
    circom.WriteZkey(path, pkj, vk, [inf1] * (1 << k))


def _write_r1cs(path, nvars, npublic, ncons):
    circom.WriteR1cs(path, nvars, 0, npublic, nvars - npublic - 1, [([(0, 1)], [(1, 1)], [(2, 1)])] * ncons)


def test_files_that_do_not_fit_are_value_errors_before_the_device(tmp_path, monkeypatch):
    def no_device(device=None):
        raise AssertionError("the device was touched before the files were compared")
    monkeypatch.setattr(capi, "init", no_device)
    r1cs, ptau, zkey, x = (str(tmp_path / n) for n in ("c.r1cs", "t.ptau", "c.zkey", "x"))
    _write_r1cs(r1cs, 6, 2, 5)                                     # 5 constraints + 3 public rows: a domain of 8
    _write_ptau(ptau, 3)
    _write_zkey(zkey, 6, 2, 3)
    _write_zkey(x, 7, 2, 3)
    with pytest.raises(ValueError, match=r"x: section 2 \(header\): nVars = 7, but the circuit .*c.r1cs \(section 1 \(header\)\) needs 6"):
        circom.VerifyZkey(r1cs, ptau, x)
    _write_zkey(x, 6, 1, 3)
    with pytest.raises(ValueError, match=r"section 2 \(header\): nPublic = 1, .* needs 2"):
        circom.VerifyZkey(r1cs, ptau, x)
    _write_zkey(x, 6, 2, 4)
    with pytest.raises(ValueError, match=r"section 2 \(header\): domainSize = 16, .* needs 8"):
        circom.VerifyZkey(r1cs, ptau, x)
    _write_ptau(x, 2)
    with pytest.raises(ValueError, match=r"x: section 1 \(header\): power = 2, but the key's domain of 2\^3"):
        circom.VerifyZkey(r1cs, x, zkey)
    # malformed files keep the readers' own errors
    with open(x, "wb") as f:
        f.write(open(zkey, "rb").read()[:-1])
    with pytest.raises(ValueError, match=r"section 9 \(H\)"):
        circom.VerifyZkey(r1cs, ptau, x)
    for power in (0, 4):
        with pytest.raises(ValueError, match=r"t.ptau: section 1 \(header\): power = 3"):
            circom.VerifyPtau(ptau, power=power)
    # files that fit reach the device (here: the stub)
    with pytest.raises(AssertionError, match="the device was touched"):
        circom.VerifyZkey(r1cs, ptau, zkey, seed=1)
    with pytest.raises(AssertionError, match="the device was touched"):
        circom.VerifyPtau(ptau, seed=1)
