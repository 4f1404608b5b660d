"""-m gpu: tests/c/zkey_check.c -- a process without Python walks a circuit.zkey and a powers-of-tau file itself, uploads their sections
and the circuit's domain R1CS, and runs gs_ptau_check and gs_groth16_key_check: the C call sequence of go/gosnarkhip/zkey_check.go.  It
accepts a good pair of files and names the failed check of a tampered one in its output."""
import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom
import c_util
from setup_util import Circuit

pytestmark = pytest.mark.gpu


def _blob(path, c, k, challenge):
    parts = [np.array([c.nc + c.npub + 1, c.nvars, c.npub, 2], dtype=np.uint64)]
    for rows in c.system_rows():
        terms = [t for row in rows for t in row]
        rp = np.concatenate([[0], np.cumsum([len(row) for row in rows])])
        parts += [np.array([len(terms)], dtype=np.uint64), rp.astype(np.uint64), np.array([s for s, _ in terms], dtype=np.uint64),
                  capi.ints_to_u64([v for _, v in terms]) if terms else np.zeros((0, 4), dtype=np.uint64)]
    parts.append(capi.ints_to_u64([k, challenge]))
    return c_util._blob(path, parts)


def test_zkey_check_c_accepts_a_good_key_and_names_the_failed_check_of_a_tampered_one(tmp_path):
    capi.init()
    k, npub, nc = 3, 1, 3
    c = Circuit(k, npub, nc, 77)
    paths = {n: str(tmp_path / n) for n in ("c.r1cs", "t.ptau", "c.zkey", "bad.zkey", "r1cs.bin")}
    c.write_r1cs(paths["c.r1cs"])
    circom.WritePtau(paths["t.ptau"], k + 1, c.tau, c.alpha, c.beta)
    circom.SetupFromPtau(paths["c.r1cs"], paths["t.ptau"], paths["c.zkey"])
    _blob(paths["r1cs.bin"], c, k, 0x1d2c3b4a59687786a5b4c3d2e1f00123456789abcdef)
    out = c_util.build_and_run("zkey_check.c", [paths["r1cs.bin"], paths["t.ptau"], paths["c.zkey"]], tmp_path)
    assert "ACCEPT transcript: 8 checks" in out and "ACCEPT key: 8 checks" in out, out
    # B1 of the last signal (the point at infinity: the wire stands in no B row) replaced by the generator
    data, sec = circom._read_sections(paths["c.zkey"], b"zkey", 1, circom._ZKEY_NAMES, (6,))
    bad = bytearray(bytes(data))
    last = sec[6][0] + (c.nvars - 1) * 64
    assert bytes(bad[last:last + 64]) != circom.G1ToZkey(circom.G1_GEN)
    bad[last:last + 64] = circom.G1ToZkey(circom.G1_GEN)
    with open(paths["bad.zkey"], "wb") as f:
        f.write(bytes(bad))
    out = c_util.build_and_run("zkey_check.c", [paths["r1cs.bin"], paths["t.ptau"], paths["bad.zkey"]], tmp_path)
    assert "ACCEPT transcript: 8 checks" in out and "REJECT key: [B1]\n" in out, out
