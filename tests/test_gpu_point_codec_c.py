"""-m gpu: tests/c/point_codec.c -- a process without Python uploads an array of G1 and an array of G2 points, compresses them, decompresses
the result and compares the downloads; then it plants an x without a root and asks how many entries are bad and where: the C call
sequence of go/gosnarkhip/point_codec.go."""
import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi
import c_util
import membership_util as M
from oracle import ref_py as O

pytestmark = pytest.mark.gpu


def test_point_codec_c_sequence_round_trips_and_locates_the_planted_x(tmp_path):
    n, at = 70, 66
    g1 = [O.G1.MulScalar(O.G1_GEN, 11 + i) for i in range(n)]
    g2 = M.subgroup_multiples(n, first=11)
    for i in range(n):
        if i % 3 == 2:
            g1[i], g2[i] = O.G1.Neg(g1[i]), O.G2.Neg(g2[i])
        if i % 5 == 4:
            g1[i], g2[i] = O.G1_ZERO, O.G2_ZERO
    path = c_util._blob(str(tmp_path / "points.bin"), [np.array([n], dtype=np.uint64), capi.g1_points_to_u64(g1), capi.g2_points_to_u64(g2)])
    out = c_util.build_and_run("point_codec.c", [path, str(at)], tmp_path)
    assert out == ("g1 round trip: 0 bad, first none, the rest equal\ng1 planted: 1 bad, first 66, the rest equal\n"
                   "g2 round trip: 0 bad, first none, the rest equal\ng2 planted: 1 bad, first 66, the rest equal\n"), out
