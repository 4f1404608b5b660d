"""-m gpu: tests/c/zkey_prove.c -- a process without Python walks the committed circuit.zkey and witness.wtns itself, hands their
sections to the four zkey entry points and takes a witness ticket: the C call sequence of go/gosnarkhip/zkey.go.  Its proof is the one
the Python route gives."""
import os

import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom
import c_util
import circom_util as CU

pytestmark = pytest.mark.gpu
ZFIX = os.path.join(CU.HERE, "golden", "zkey_multiplier")


def test_zkey_prove_c_sequence_gives_the_python_routes_proof(tmp_path):
    zpath, wpath = os.path.join(ZFIX, "circuit.zkey"), os.path.join(ZFIX, "witness.wtns")
    out = c_util.build_and_run("zkey_prove.c", [zpath, wpath], tmp_path)
    words = [int(x, 16) for x in out.split()]
    assert len(words) == 32, out
    v = [sum(words[4 * i + j] << (64 * j) for j in range(4)) for i in range(8)]
    r, s = 0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321fedcba0987654321
    capi.init()
    dev, r1cs = circom.UploadZkey(zpath)
    want = circom.GenerateProofs(dev, r1cs, circom.ReadWtns(wpath), r, s)
    assert (v[0], v[1]) == want.PiA[:2]
    assert ((v[2], v[3]), (v[4], v[5])) == want.PiB[:2]
    assert (v[6], v[7]) == want.PiC[:2]
    vk = circom.VerificationKeyFromZkey(zpath)
    assert circom.VerifyFromCircom(vk, want, [33]) is True
