"""-m gpu: tests/c/r1cs_check.c -- a process without Python uploads a system and a witness, asks gs_r1cs_check for the violated rows and
their values, then for the count alone (the call sequence of go/gosnarkhip.R1csCheck).  Expectations are Python integers."""
import pytest

import gosnark_amd  # noqa: F401
import c_util
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = O.R


def instance(tmp_path, name, w):
    """x_j * x_j = y_j for j < 6 over [one, x_0 .. x_5, y_0 .. y_5]"""
    n, m = 6, 13
    a = [[1 if i == 1 + j else 0 for i in range(m)] for j in range(n)]
    c = [[1 if i == 7 + j else 0 for i in range(m)] for j in range(n)]
    return c_util.write_r1cs(tmp_path, (a, a, c), 0, w, name=name)


def test_r1cs_check_c_sequence_names_rows_and_values(tmp_path):
    xs = [3, R - 1, 0, 12345, 2, R - 2]
    good = [1] + xs + [x * x % R for x in xs]
    bad = list(good)
    for j in (1, 4, 5):
        bad[7 + j] = (bad[7 + j] + 1) % R
    out = c_util.build_and_run("r1cs_check.c", [instance(tmp_path, "good.bin", good), "4"], tmp_path).split("\n")
    assert out[:2] == ["violated 0", "PROVE"]
    limbs = lambda v: " ".join("%016x" % ((v >> (64 * i)) & (2 ** 64 - 1)) for i in range(4))              # noqa: E731
    line = lambda j: "row %d %s %s %s" % (j, limbs(xs[j]), limbs(xs[j]), limbs(bad[7 + j]))             # noqa: E731
    out = c_util.build_and_run("r1cs_check.c", [instance(tmp_path, "bad.bin", bad), "2"], tmp_path).split("\n")
    assert out[:4] == ["violated 3", line(1), line(4), "REFUSE"]
    out = c_util.build_and_run("r1cs_check.c", [instance(tmp_path, "bad.bin", bad), "8"], tmp_path).split("\n")
    assert out[:5] == ["violated 3", line(1), line(4), line(5), "REFUSE"]
