"""CPU-side checks of preparing a transcript for phase 2: the library exports gs_g*_lagrange_levels and gs_g*_lagrange_levels_check, the
header declares them, the ctypes binding and the Go binding know them; without a device they say GS_ERR_NOT_INIT and leave *out alone;
circom.ReadPtauPrepared reads the layout of sections 12 - 15 and names the section of every malformation while ReadPtau stays
indifferent to them; and every ValueError of circom.PreparePtau, SetupFromPtau(prepared=True) and VerifyPtauPrepared is raised before
the device is touched."""
import ctypes
import os
import struct

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = ("gs_g1_lagrange_levels", "gs_g2_lagrange_levels")
CHECKS = ("gs_g1_lagrange_levels_check", "gs_g2_lagrange_levels_check")
R = circom.R


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _no_device(device=None):
    raise AssertionError("the device was touched")


def test_entry_points_are_exported_declared_and_bound():
    lib = capi.load_library()
    text = open(os.path.join(ROOT, "include", "gosnark_hip.h")).read()
    go = open(os.path.join(ROOT, "go", "gosnarkhip", "ptau.go")).read()
    for name in LEVELS + CHECKS:
        assert hasattr(lib, name) and name in capi.EXPORTS and name in capi._SIGS
        assert getattr(lib, name).argtypes == capi._SIGS[name]
        assert "C.%s(" % name in go
    for name in LEVELS:
        assert capi._SIGS[name] == [capi.Handle, ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(capi.Handle)]
        assert "int %s(gs_handle powers, size_t lo, size_t hi, gs_handle* out);" % name in text
    for name in CHECKS:
        assert capi._SIGS[name] == [capi.Handle, capi.Handle, ctypes.c_size_t, capi.u64p, ctypes.POINTER(capi.CheckResult)]
        assert "int %s(gs_handle powers, gs_handle levels, size_t hi, const uint64_t challenge[4], gs_check_result* out);" % name in text
    for name in ("LagrangeLevelsG1", "LagrangeLevelsG2", "CheckLagrangeLevelsG1", "CheckLagrangeLevelsG2", "PreparePtauArrays"):
        assert "func %s(" % name in go
    for name in ("g1_lagrange_levels", "g2_lagrange_levels", "g1_lagrange_levels_check", "g2_lagrange_levels_check"):
        assert callable(getattr(capi, name))
    for name in ("ReadPtauPrepared", "PreparePtau", "VerifyPtauPrepared"):
        assert callable(getattr(circom, name))
    assert "tests/c/ptau_prepare.c" in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert os.path.exists(os.path.join(ROOT, "tests", "c", "ptau_prepare.c"))


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_without_a_device():
    lib = capi.load_library()
    s = capi.ints_to_u64([5])
    for name in LEVELS:
        h = capi.Handle(77)
        assert getattr(lib, name)(1, 0, 1, ctypes.byref(h)) == -5      # GS_ERR_NOT_INIT
        assert b"gs_init" in lib.gs_last_error() and h.value == 77
    for name in CHECKS:
        res = capi.CheckResult()
        res.ok, res.lhs[3] = 9, 1234
        assert getattr(lib, name)(1, 2, 1, capi.ptr64(s[0]), ctypes.byref(res)) == -5
        assert b"gs_init" in lib.gs_last_error() and (res.ok, res.lhs[3]) == (9, 1234)
    for f in (capi.g1_lagrange_levels, capi.g2_lagrange_levels):
        with pytest.raises(capi.GosnarkHipError) as e:
            f(capi.DeviceHandle(0), 0, 1)
        assert e.value.code == -5
    for f in (capi.g1_lagrange_levels_check, capi.g2_lagrange_levels_check):
        with pytest.raises(capi.GosnarkHipError) as e:
            f(capi.DeviceHandle(0), capi.DeviceHandle(0), 1, (1 << 256) - 1)
        assert e.value.code == -5


# ---- files ---------------------------------------------------------------------------------------------------------------------------
def _sections(path):
    data = open(path, "rb").read()
    nsec, pos, out = struct.unpack("<I", data[8:12])[0], 12, []
    for _ in range(nsec):
        sid, length = struct.unpack("<IQ", data[pos:pos + 12])
        out.append((sid, data[pos + 12:pos + 12 + length]))
        pos += 12 + length
    assert pos == len(data)
    return out


def _write(path, secs):
    with open(path, "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, len(secs)))
        for sid, payload in secs:
            f.write(struct.pack("<IQ", sid, len(payload)) + payload)


def _counts(power):
    n = 1 << power
    return {12: (4 * n - 1, 64), 13: (2 * n - 1, 128), 14: (2 * n - 1, 64), 15: (2 * n - 1, 64)}


def _fake_prepared(path, power, order=(12, 13, 14, 15), lengths=None, front=False):
    """NewPtau's sections plus prepared sections whose point i of section sid is the byte pattern (sid, i): host code only"""
    circom.NewPtau(path, power)
    extra = []
    for sid in order:
        count, size = _counts(power)[sid]
        count = (lengths or {}).get(sid, count)
        body = np.zeros((count, size), dtype=np.uint8)
        body[:, 0], body[:, 1], body[:, 2] = sid, np.arange(count) & 255, np.arange(count) >> 8
        extra.append((sid, body.tobytes()))
    secs = _sections(path)
    _write(path, extra + secs if front else secs + extra)


@pytest.mark.parametrize("power", [0, 1, 3])
def test_read_ptau_prepared_counts_and_levels(power, tmp_path):
    path = str(tmp_path / "p.ptau")
    _fake_prepared(path, power)
    p = circom.ReadPtauPrepared(path)
    assert isinstance(p, circom.Ptau) and (p.power, p.ceremonyPower) == (power, power)
    plain = circom.ReadPtau(path)
    for name in ("tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2"):
        assert np.array_equal(getattr(p, name), getattr(plain, name))
    for sid, (count, size) in _counts(power).items():
        assert p.lagrange[sid].size == count * size and not p.lagrange[sid].flags.writeable
        top = power + (1 if sid == 12 else 0)
        assert p.top_level(sid) == top
        at = 0
        for lv in range(top + 1):
            rows = np.asarray(p.level(sid, lv)).reshape(-1, size)
            assert rows.shape[0] == 1 << lv and at == (1 << lv) - 1
            assert all(tuple(r[:3]) == (sid, (at + i) & 255, (at + i) >> 8) for i, r in enumerate(rows))
            at += 1 << lv
        assert at == count
        for lv in (-1, top + 1):
            with pytest.raises(ValueError, match=r"section %d \(.* Lagrange\) holds the levels 0 \.\. %d" % (sid, top)):
                p.level(sid, lv)


def test_read_ptau_prepared_accepts_any_section_order(tmp_path):
    a, b = str(tmp_path / "a.ptau"), str(tmp_path / "b.ptau")
    _fake_prepared(a, 2)
    _fake_prepared(b, 2, order=(15, 12, 14, 13), front=True)
    pa, pb = circom.ReadPtauPrepared(a), circom.ReadPtauPrepared(b)
    for sid in (12, 13, 14, 15):
        assert np.array_equal(pa.lagrange[sid], pb.lagrange[sid])
    assert np.array_equal(pa.tauG1, pb.tauG1)


def test_read_ptau_prepared_names_the_section_of_every_malformation(tmp_path):
    path = str(tmp_path / "p.ptau")
    names = {12: "tauG1 Lagrange", 13: "tauG2 Lagrange", 14: "alphaTauG1 Lagrange", 15: "betaTauG1 Lagrange"}
    for sid, name in names.items():
        _fake_prepared(path, 2, order=[s for s in names if s != sid])
        with pytest.raises(ValueError, match=r"section %d \(%s\) is missing" % (sid, name)):
            circom.ReadPtauPrepared(path)
        count, size = _counts(2)[sid]
        for wrong in (count - 1, count + 1, 0):
            _fake_prepared(path, 2, lengths={sid: wrong})
            with pytest.raises(ValueError, match=r"section %d \(%s\) has %d bytes, its counts need %d" % (sid, name, wrong * size, count * size)):
                circom.ReadPtauPrepared(path)
    # levels 0 .. power of tauG1 only (the length of sections 14 / 15): section 12 runs to level power + 1
    _fake_prepared(path, 2, lengths={12: 7})
    with pytest.raises(ValueError, match=r"section 12 \(tauG1 Lagrange\) has 448 bytes, its counts need 960"):
        circom.ReadPtauPrepared(path)
    _fake_prepared(path, 2)
    secs = _sections(path)
    _write(path, secs + [secs[-1]])
    with pytest.raises(ValueError, match=r"section 15 \(betaTauG1 Lagrange\) appears twice"):
        circom.ReadPtauPrepared(path)
    _write(path, secs)
    with open(path, "r+b") as f:
        f.truncate(os.path.getsize(path) - 1)
    with pytest.raises(ValueError, match=r"section 15 \(\d+ bytes\) runs past the end"):      # ReadPtau's walk says it first, by number
        circom.ReadPtauPrepared(path)
    # what ReadPtau raises comes first
    _write(path, [s for s in secs if s[0] != 4])
    with pytest.raises(ValueError, match=r"section 4 \(alphaTauG1\) is missing"):
        circom.ReadPtauPrepared(path)


def test_read_ptau_stays_indifferent_to_the_prepared_sections(tmp_path):
    path = str(tmp_path / "p.ptau")
    _fake_prepared(path, 2, lengths={12: 3})
    assert circom.ReadPtau(path).power == 2
    secs = _sections(path)
    _write(path, secs + [secs[-1]])                     # even twice
    assert circom.ReadPtau(path).power == 2
    assert 12 not in circom._PTAU_NAMES and 12 in circom._PTAU_PREPARED_NAMES


# ---- ValueErrors before the device --------------------------------------------------------------------------------------------------
def test_prepare_ptau_value_errors_come_before_the_device(tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "init", _no_device)
    src, dst, bad = (str(tmp_path / n) for n in ("in.ptau", "out.ptau", "bad.ptau"))
    circom.NewPtau(src, 2)
    for b in (-1, 28):
        with pytest.raises(ValueError, match="batch_log2 = %d is not in 0 .. 27" % b):
            circom.PreparePtau(src, dst, batch_log2=b)
    with pytest.raises(ValueError, match="must not be the input file"):
        circom.PreparePtau(src, src)
    os.symlink(src, str(tmp_path / "link.ptau"))
    with pytest.raises(ValueError, match="must not be the input file"):
        circom.PreparePtau(src, str(tmp_path / "link.ptau"))
    with open(bad, "wb") as f:
        f.write(open(src, "rb").read()[:-1])
    with pytest.raises(ValueError, match=r"section 6 \(betaG2\)"):
        circom.PreparePtau(bad, dst)
    with open(bad, "wb") as f:
        f.write(b"zkey" + open(src, "rb").read()[4:])
    with pytest.raises(ValueError, match="not a .ptau file"):
        circom.PreparePtau(bad, dst)
    # powers 27 and 28: ReadPtau is given a Ptau of that power without a file of 2^27 points
    real = circom.ReadPtau
    for power in (27, 28):
        def huge(path, power=power):
            p = real(path)
            p.power = p.ceremonyPower = power
            return p
        monkeypatch.setattr(circom, "ReadPtau", huge)
        with pytest.raises(ValueError, match=r"section 1 \(header\): power = %d, preparing needs power <= 26" % power):
            circom.PreparePtau(src, dst)
    monkeypatch.setattr(circom, "ReadPtau", real)
    assert not os.path.exists(dst)
    # a valid call reaches the device (here: the stub)
    with pytest.raises(AssertionError, match="the device was touched"):
        circom.PreparePtau(src, dst, batch_log2=0)
    with pytest.raises(AssertionError, match="the device was touched"):
        circom.PreparePtau(src, dst, batch_log2=27)


def _tiny_r1cs(path):
    """one product w1 * w2 = w3 with w1 public: nConstraints + nPublic = 2, a domain of 2^2"""
    circom.WriteR1cs(path, 4, 0, 1, 2, [([(1, 1)], [(2, 1)], [(3, 1)])])


def test_setup_from_prepared_value_errors_come_before_the_device(tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "init", _no_device)
    r1cs, ptau, zkey = (str(tmp_path / n) for n in ("c.r1cs", "t.ptau", "c.zkey"))
    _tiny_r1cs(r1cs)
    circom.NewPtau(ptau, 2)                               # no prepared sections at all
    with pytest.raises(ValueError, match=r"section 12 \(tauG1 Lagrange\) is missing"):
        circom.SetupFromPtau(r1cs, ptau, zkey, prepared=True)
    _fake_prepared(ptau, 2, lengths={13: 6})              # one of the wrong length
    with pytest.raises(ValueError, match=r"section 13 \(tauG2 Lagrange\) has 768 bytes, its counts need 896"):
        circom.SetupFromPtau(r1cs, ptau, zkey, prepared=True)
    _fake_prepared(ptau, 1)                               # prepared, but too small for the circuit
    with pytest.raises(ValueError, match=r"power = 1, but 1 constraints and 1 public signals need a domain of 2\^2 points"):
        circom.SetupFromPtau(r1cs, ptau, zkey, prepared=True)
    assert not os.path.exists(zkey)
    _fake_prepared(ptau, 2)
    with pytest.raises(AssertionError, match="the device was touched"):
        circom.SetupFromPtau(r1cs, ptau, zkey, prepared=True)
    # the default path does not look at the prepared sections: a mis-sized one does not stop it before the device
    _fake_prepared(ptau, 2, lengths={13: 6})
    with pytest.raises(AssertionError, match="the device was touched"):
        circom.SetupFromPtau(r1cs, ptau, zkey)


def test_verify_ptau_prepared_value_errors_come_before_the_device(tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "init", _no_device)
    path = str(tmp_path / "t.ptau")
    circom.NewPtau(path, 2)
    with pytest.raises(ValueError, match=r"section 12 \(tauG1 Lagrange\) is missing"):
        circom.VerifyPtauPrepared(path)
    _fake_prepared(path, 2)
    for power in (-1, 3):
        with pytest.raises(ValueError, match=r"the levels 0 \.\. %d cannot be checked \(0 <= power <= 2" % power):
            circom.VerifyPtauPrepared(path, power=power)
    with pytest.raises(AssertionError, match="the device was touched"):
        circom.VerifyPtauPrepared(path, power=0, seed=1)
