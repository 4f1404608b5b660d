"""CPU-side checks of the compressed-point entry points: the library exports the four calls, the header declares them, the ctypes binding
and the Go binding know them and INTEGRATION.md names them; without a device they say GS_ERR_NOT_INIT and touch no out-argument (nothing
falls back to host code); the two verifier front ends have the signatures the callers are told."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import bn128, capi, compressed, groth16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DECOMPRESS = [capi.u64p, capi.u8p, ctypes.c_size_t, ctypes.POINTER(capi.Handle), capi.u8p, capi.u64p, capi.u64p]
COMPRESS = [capi.Handle, ctypes.c_size_t, ctypes.c_size_t, capi.u64p, capi.u8p]
NAMES = {"gs_g1_decompress": DECOMPRESS, "gs_g2_decompress": DECOMPRESS, "gs_g1_compress": COMPRESS, "gs_g2_compress": COMPRESS}


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def test_the_four_calls_are_exported_declared_and_bound():
    lib = capi.load_library()
    header = " ".join(open(os.path.join(ROOT, "include", "gosnark_hip.h")).read().split())
    go = open(os.path.join(ROOT, "go", "gosnarkhip", "point_codec.go")).read()
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name, sig in NAMES.items():
        assert hasattr(lib, name) and name in capi.EXPORTS and capi._SIGS[name] == sig
        assert getattr(lib, name).argtypes == sig
        assert "int %s(" % name in header
        assert "C.%s(" % name in go
        assert callable(getattr(capi, name[3:])) and callable(getattr(bn128, name[3:5].upper() + name[6:].capitalize()))
    assert ("int gs_g1_decompress(const uint64_t* x /* n x 4 */, const uint8_t* flags /* n */, size_t n, gs_handle* out, "
            "uint8_t* ok /* n, or NULL */, uint64_t* nbad, uint64_t* first_bad);") in header
    assert "int gs_g2_compress(gs_handle bases, size_t off, size_t n, uint64_t* x /* n x 8 */, uint8_t* flags);" in header
    assert "#define GS_POINT_LARGEST_Y 1u" in header and "#define GS_POINT_INFINITY 2u" in header
    assert (capi.POINT_LARGEST_Y, capi.POINT_INFINITY) == (1, 2)
    assert "gs_g2_subgroup_check" in header[header.index("compressed points"):header.index("#define GS_POINT_LARGEST_Y")]
    for fn in ("G1Decompress", "G2Decompress", "G1Compress", "G2Compress"):
        assert "func %s(" % fn in go and fn in integration
    assert "func VerifyProofsEachCompressed(" in open(os.path.join(ROOT, "go", "groth16hip", "groth16hip.go")).read()
    assert "point_codec.c" in integration and os.path.exists(os.path.join(ROOT, "tests", "c", "point_codec.c"))


def test_the_go_layer_still_resolves_every_argument():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import check_go_abi
    finally:
        sys.path.pop(0)
    errors, stats = check_go_abi.check()
    assert errors == [] and stats["unresolved_arguments"] == 0


def test_verifier_front_ends_have_the_documented_signatures():
    p = inspect.signature(groth16.VerifyProofsEachCompressed).parameters
    assert list(p) == ["vk", "blobs", "publicSignalsList", "codec"] and all(v.default is inspect.Parameter.empty for v in p.values())
    p = inspect.signature(groth16.VerifyProofsCompressed).parameters
    assert list(p) == ["vk", "blobs", "publicSignalsList", "codec", "seed"] and p["seed"].default is None
    assert list(inspect.signature(compressed.DecompressProofs).parameters) == ["blobs", "codec"]
    assert list(inspect.signature(compressed.CompressProof).parameters) == ["proof", "codec"]
    assert list(inspect.signature(capi.g1_compress).parameters) == ["handle", "off", "n"]
    assert list(inspect.signature(capi.g2_decompress).parameters) == ["x_u64", "flags"]


@pytest.mark.skipif(_has_gpu(), reason="checks the no-device behaviour")
def test_without_a_device_the_calls_say_not_init_and_touch_nothing():
    lib = capi.load_library()
    x, flags, ok = np.full(8, 7, dtype=np.uint64), np.full(1, 7, dtype=np.uint8), np.full(1, 7, dtype=np.uint8)
    u8 = lambda a: a.ctypes.data_as(capi.u8p)   # noqa: E731
    for name in ("gs_g1_decompress", "gs_g2_decompress"):
        h, nbad, first = capi.Handle(7), ctypes.c_uint64(7), ctypes.c_uint64(7)
        assert getattr(lib, name)(capi.ptr64(x), u8(flags), 1, ctypes.byref(h), u8(ok), ctypes.byref(nbad), ctypes.byref(first)) == -5
        assert b"gs_init" in lib.gs_last_error() and (h.value, nbad.value, first.value, int(ok[0])) == (7, 7, 7, 7)
        assert getattr(lib, name)(None, None, 1, None, None, None, None) == -5          # before an argument is looked at
    for name in ("gs_g1_compress", "gs_g2_compress"):
        assert getattr(lib, name)(1, 0, 1, capi.ptr64(x), u8(flags)) == -5
        assert b"gs_init" in lib.gs_last_error() and x.tolist() == [7] * 8 and int(flags[0]) == 7
        assert getattr(lib, name)(1, 0, 1, None, None) == -5
    with pytest.raises(capi.GosnarkHipError) as e:
        capi.g1_compress(capi.DeviceHandle(0), 0, 1)
    assert e.value.code == -5
