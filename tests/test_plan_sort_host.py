"""Host instantiation of the sort plan's index arithmetic (msm_kernels.h: the XCD-coherent workgroup map of k_hist / k_scatter, the
slices of a padded digit row, the stored form of a digit), compiled for the CPU: tests/host/plan_sort_test.hip."""
import subprocess

import hostbuild


def test_sort_block_map_slices_and_digit_code():
    """For W in {8, 13, 15, 16, 17, 26} and S, R in {1, 2, 3, 8, 16}: every (window, slice, range) is produced exactly once, padded ids
    exit, id % 8 == window % 8; the slices of a row partition its 8-term groups; every digit of c = 8 .. 20 round-trips."""
    exe = hostbuild.build("plan_sort_test")
    out = subprocess.run([exe], capture_output=True, text=True).stdout
    assert out.startswith("OK 150 maps"), out
