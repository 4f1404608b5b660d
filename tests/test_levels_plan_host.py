"""Host instantiation of the all-levels transform's index arithmetic (csrc/levels_plan.h), compiled for the CPU:
tests/host/levels_plan_host_test.hip walks every launch of every stage with the functions the kernels call."""
import subprocess

import hostbuild


def test_every_level_and_butterfly_is_visited_once_inside_its_slot():
    """All 0 <= lo <= hi <= 10 (66 pairs), every span: each (level, butterfly) with 2^p >= 2h exactly once, both operands inside their
    level's slot, twiddle index below 2^(hi-1); and the schedule run on integers mod 12289 equals every level's O(n^2) inverse transform,
    with the short last level when hi is odd."""
    exe = hostbuild.build("levels_plan_host_test")
    out = subprocess.run([exe], capture_output=True, text=True).stdout
    assert out.startswith("OK 66 pairs"), out
