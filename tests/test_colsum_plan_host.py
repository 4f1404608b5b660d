"""Host instantiation of the column sums' index arithmetic (csrc/colsum_plan.h: chunks, heads and tails of the segmented reduction, the
classes of a coefficient), compiled for the CPU: tests/host/colsum_plan_test.hip runs every level with the loop the kernels run."""
import subprocess

import hostbuild


def test_colsum_chunks_heads_tails_and_coefficient_classes():
    """Column-length profiles [0, 1, C-1, C, C+1, 3C+1] at every rotation (and twice over), one column holding every term (up to 2^16 + 1),
    all columns empty, one term per column: every entry of every level is added exactly once, every slot of the next level is written once
    and stays sorted, every non-empty column is handed out exactly once with all its terms; 0, +-1, +-2, +-65535, +-(2^32 - 1), 2^32, 2^128,
    r, r + 1 and 2^256 - 1 get their class, sign, bit length and magnitude."""
    exe = hostbuild.build("colsum_plan_test")
    out = subprocess.run([exe], capture_output=True, text=True).stdout
    assert out.startswith("OK 49 profiles"), out
