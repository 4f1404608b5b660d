"""-m gpu: tests/c/zkey_setup.c -- a process without Python walks a powers-of-tau file itself, uploads its sections and the circuit's
domain R1CS, and computes the arrays of a circuit.zkey with the Lagrange, column-sum, scale and download entry points: the C call sequence
of go/gosnarkhip/setup_ptau.go.  Its bytes are the sections circom.SetupFromPtau writes, and K / delta is what ContributeDelta's scale
gives (closed form)."""
import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom
import c_util
import circom_util as CU
from setup_util import Circuit

pytestmark = pytest.mark.gpu
R = CU.R


def _blob(path, c, k, scalar):
    parts = [np.array([c.nc + c.npub + 1, c.nvars, c.npub, 2], dtype=np.uint64)]
    for rows in c.system_rows():
        terms = [t for row in rows for t in row]
        rp = np.concatenate([[0], np.cumsum([len(row) for row in rows])])
        parts += [np.array([len(terms)], dtype=np.uint64), rp.astype(np.uint64), np.array([s for s, _ in terms], dtype=np.uint64),
                  capi.ints_to_u64([v for _, v in terms]) if terms else np.zeros((0, 4), dtype=np.uint64)]
    parts.append(capi.ints_to_u64([k, scalar]))
    return c_util._blob(path, parts)


@pytest.mark.parametrize("extra_power", [0, 1])
def test_zkey_setup_c_sequence_gives_the_python_routes_sections(tmp_path, extra_power):
    capi.init()
    k, npub, nc = 3, 1, 3
    c = Circuit(k, npub, nc, 77)
    delta = 0x1d2c3b4a59687786a5b4c3d2e1f00123456789abcdef
    paths = {n: str(tmp_path / n) for n in ("c.r1cs", "t.ptau", "c.zkey", "r1cs.bin", "out.bin")}
    c.write_r1cs(paths["c.r1cs"])
    circom.WritePtau(paths["t.ptau"], k + extra_power, c.tau, c.alpha, c.beta)
    _blob(paths["r1cs.bin"], c, k, pow(delta, -1, R))
    out = c_util.build_and_run("zkey_setup.c", [paths["r1cs.bin"], paths["t.ptau"], paths["out.bin"]], tmp_path)
    assert out.startswith("OK %d variables, domain 2^%d" % (c.nvars, k)), out
    got = np.fromfile(paths["out.bin"], dtype=np.uint8)
    circom.SetupFromPtau(paths["c.r1cs"], paths["t.ptau"], paths["c.zkey"])
    z = circom.ReadZkey(paths["c.zkey"])
    n, m = c.nvars * 64, c.m * 64
    assert np.array_equal(got[:n], z.A) and np.array_equal(got[n:2 * n], z.B1)
    assert np.array_equal(got[2 * n:3 * n], np.concatenate([z.IC, z.C]))
    assert np.array_equal(got[3 * n:3 * n + m], z.H)
    assert np.array_equal(got[4 * n + m:], z.B2)
    scaled = capi.g1_download(capi.g1_upload_affine_mont(got[3 * n + m:4 * n + m]))
    dinv = pow(delta, -1, R)
    assert np.array_equal(scaled, capi.g1_download(capi.g1_fixed_base(CU.u64([x * dinv % R for x in c.kk]))))
