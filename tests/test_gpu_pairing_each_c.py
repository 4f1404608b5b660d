"""-m gpu: tests/c/pairing_each.c -- a process without Python computes a pairing per pair with gs_pairing_each: the C call sequence of
gosnarkhip.PairingEach (go/gosnarkhip/pairing_device.go).  Every value must be the host's, and the flags must mark the pairs with an
infinite member."""
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi
import c_util
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
N = 65


def test_pairing_each_c_sequence_equals_the_host_pairing(tmp_path):
    capi.init()
    rng = random.Random(21)
    a = [rng.randrange(1, O.R) for _ in range(N)]
    b = [rng.randrange(1, O.R) for _ in range(N)]
    a[3] = b[40] = a[64] = 0
    p = capi.g1_download(capi.g1_fixed_base(capi.ints_to_u64(a)))
    q = capi.g2_download(capi.g2_fixed_base(capi.ints_to_u64(b)))
    path = c_util._blob(str(tmp_path / "pairs.bin"), [np.array([N], dtype=np.uint64), p, q])
    out = c_util.build_and_run("pairing_each.c", [path], tmp_path)
    flags = "".join("1" if i in (3, 40, 64) else "0" for i in range(N))
    assert out == "65 pairings, 65 equal to the host's\nis one: %s\n" % flags, out
