"""-m gpu: tests/c/g2_membership.c -- a process without Python uploads an array of G2 points and asks gs_g2_subgroup_check which of them lie
outside the order-r subgroup: the C call sequence of go/gosnarkhip/g2_membership.go.  It accepts an array of multiples of the generator and
counts and locates a planted point of the form G + S, ord(S) = 10069, in its output."""
import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi
import c_util
import membership_util as M

pytestmark = pytest.mark.gpu


def test_g2_membership_c_sequence_counts_and_locates_the_planted_point(tmp_path):
    n, at = 70, 66
    pts = M.subgroup_multiples(n, first=11)
    head = np.array([n], dtype=np.uint64)
    good = c_util._blob(str(tmp_path / "good.bin"), [head, capi.g2_points_to_u64(pts)])
    out = c_util.build_and_run("g2_membership.c", [good], tmp_path)
    assert out == "all [0, 70): 0 outside, first none\nACCEPT\n", out
    pts[at] = M.complete_add(pts[at], M.small_order_point())
    bad = c_util._blob(str(tmp_path / "bad.bin"), [head, capi.g2_points_to_u64(pts)])
    out = c_util.build_and_run("g2_membership.c", [bad], tmp_path)
    assert out == ("all [0, 70): 1 outside, first 66\nbefore [0, 66): 0 outside, first none\nat [66, 67): 1 outside, first 66\n"
                   "after [67, 70): 0 outside, first none\nREJECT\n"), out
