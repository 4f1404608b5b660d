"""CPU-side checks of the phase-1 contribution: the library exports gs_g1_scale_powers / gs_g2_scale_powers, the header declares them, the
ctypes binding and the Go binding know them; without a device they say GS_ERR_NOT_INIT (nothing falls back to host code);
circom.NewPtau is host code and writes the transcript of tau = alpha = beta = 1; and every ValueError of circom.ContributePtau is
raised before the device is touched."""
import ctypes
import os
import struct

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gs_g1_scale_powers", "gs_g2_scale_powers")
R = circom.R


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def _no_device(device=None):
    raise AssertionError("the device was touched")


def test_scale_powers_entry_points_are_exported_declared_and_bound():
    lib = capi.load_library()
    text = open(os.path.join(ROOT, "include", "gosnark_hip.h")).read()
    go = open(os.path.join(ROOT, "go", "gosnarkhip", "ptau.go")).read()
    for name in NEW:
        assert hasattr(lib, name) and name in capi.EXPORTS and name in capi._SIGS
        assert getattr(lib, name).argtypes == capi._SIGS[name]
        assert capi._SIGS[name] == [capi.Handle, ctypes.c_size_t, ctypes.c_size_t, capi.u64p, capi.u64p, ctypes.POINTER(capi.Handle)]
        assert "int %s(gs_handle bases, size_t off, size_t n, const uint64_t c[4], const uint64_t t[4], gs_handle* out);" % name in text
        assert "C.%s(" % name in go
    for name in ("ScalePowersG1", "ScalePowersG2", "ContributePtauArrays"):
        assert "func %s(" % name in go
    for name in ("g1_scale_powers", "g2_scale_powers"):
        assert callable(getattr(capi, name))
    for name in ("NewPtau", "ContributePtau"):
        assert callable(getattr(circom, name))


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_scale_powers_without_a_device():
    lib = capi.load_library()
    s = capi.ints_to_u64([5, 7])
    for name in NEW:
        h = capi.Handle(0)
        assert getattr(lib, name)(1, 0, 1, capi.ptr64(s[0]), capi.ptr64(s[1]), ctypes.byref(h)) == -5      # GS_ERR_NOT_INIT
        assert b"gs_init" in lib.gs_last_error() and h.value == 0
    for f in (capi.g1_scale_powers, capi.g2_scale_powers):
        with pytest.raises(capi.GosnarkHipError) as e:
            f(capi.DeviceHandle(0), 0, 1, (1 << 256) - 1, R - 1)
        assert e.value.code == -5


def _sections(path):
    data = open(path, "rb").read()
    assert data[:4] == b"ptau" and struct.unpack("<I", data[4:8])[0] == 1
    nsec, pos, out = struct.unpack("<I", data[8:12])[0], 12, []
    for _ in range(nsec):
        sid, length = struct.unpack("<IQ", data[pos:pos + 12])
        out.append((sid, data[pos + 12:pos + 12 + length]))
        pos += 12 + length
    assert pos == len(data)
    return out


@pytest.mark.parametrize("power", [0, 3])
def test_new_ptau_is_the_transcript_of_ones_and_needs_no_device(power, tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "init", _no_device)
    path = str(tmp_path / "new.ptau")
    circom.NewPtau(path, power)
    n = 1 << power
    secs = _sections(path)
    assert [sid for sid, _ in secs] == [1, 2, 3, 4, 5, 6]
    assert [len(b) for _, b in secs] == [44, (2 * n - 1) * 64, n * 128, n * 64, n * 64, 128]
    p = circom.ReadPtau(path)
    assert (p.power, p.ceremonyPower) == (power, power)
    for sec, count in ((p.tauG1, 2 * n - 1), (p.alphaTauG1, n), (p.betaTauG1, n)):
        rows = np.asarray(sec).reshape(-1, 64)
        assert rows.shape[0] == count and all(circom.G1FromZkey(row) == circom.G1_GEN for row in rows)
    for sec, count in ((p.tauG2, n), (p.betaG2, 1)):
        rows = np.asarray(sec).reshape(-1, 128)
        assert rows.shape[0] == count and all(circom.G2FromZkey(row) == circom.G2_GEN for row in rows)


def test_new_ptau_writes_in_pieces_across_the_piece_size(tmp_path, monkeypatch):
    """2^17 - 1 tauG1 points: more than one write of 2^16 points and a ragged last one"""
    monkeypatch.setattr(capi, "init", _no_device)
    path = str(tmp_path / "new.ptau")
    circom.NewPtau(path, 16)
    p = circom.ReadPtau(path)
    g1 = np.frombuffer(circom.G1ToZkey(circom.G1_GEN), dtype=np.uint8)
    assert np.array_equal(np.asarray(p.tauG1).reshape(-1, 64), np.broadcast_to(g1, ((2 << 16) - 1, 64)))
    g2 = np.frombuffer(circom.G2ToZkey(circom.G2_GEN), dtype=np.uint8)
    assert np.array_equal(np.asarray(p.tauG2).reshape(-1, 128), np.broadcast_to(g2, (1 << 16, 128)))


@pytest.mark.parametrize("power", [-1, 29])
def test_new_ptau_refuses_a_power_outside_0_28(power, tmp_path):
    with pytest.raises(ValueError, match="power = %d" % power):
        circom.NewPtau(str(tmp_path / "x.ptau"), power)
    assert not os.path.exists(str(tmp_path / "x.ptau"))


def test_contribute_ptau_value_errors_come_before_the_device(tmp_path, monkeypatch):
    monkeypatch.setattr(capi, "init", _no_device)
    src, dst, bad = (str(tmp_path / n) for n in ("in.ptau", "out.ptau", "bad.ptau"))
    circom.NewPtau(src, 2)
    for tau, alpha, beta, name in ((0, 2, 3, "tau"), (R, 2, 3, "tau"), (2, 2 * R, 3, "alpha"), (2, 3, 0, "beta")):
        with pytest.raises(ValueError, match="%s must not be 0 mod r" % name):
            circom.ContributePtau(src, dst, tau, alpha, beta)
    with pytest.raises(ValueError, match="must not be the input file"):
        circom.ContributePtau(src, src, 2, 3, 4)
    os.symlink(src, str(tmp_path / "link.ptau"))
    with pytest.raises(ValueError, match="must not be the input file"):
        circom.ContributePtau(src, str(tmp_path / "link.ptau"), 2, 3, 4)
    for slab in (-1, 29):
        with pytest.raises(ValueError, match="slab_log2 = %d" % slab):
            circom.ContributePtau(src, dst, 2, 3, 4, slab_log2=slab)
    # what ReadPtau raises: a truncated file, a file that is no transcript
    with open(bad, "wb") as f:
        f.write(open(src, "rb").read()[:-1])
    with pytest.raises(ValueError, match=r"section 6 \(betaG2\)"):
        circom.ContributePtau(bad, dst, 2, 3, 4)
    with open(bad, "wb") as f:
        f.write(b"zkey" + open(src, "rb").read()[4:])
    with pytest.raises(ValueError, match="not a .ptau file"):
        circom.ContributePtau(bad, dst, 2, 3, 4)
    assert not os.path.exists(dst)
    assert open(src, "rb").read() == b"".join([b"ptau", struct.pack("<II", 1, 6)] + [struct.pack("<IQ", s, len(b)) + b for s, b in _sections(src)])
    # a valid call reaches the device (here: the stub)
    with pytest.raises(AssertionError, match="the device was touched"):
        circom.ContributePtau(src, dst, 2, 3, 4, slab_log2=0)
