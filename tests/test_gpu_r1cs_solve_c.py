"""-m gpu: tests/c/r1cs_solve.c -- a process without Python uploads a system, plans its solve, solves three witnesses in one call (the
call sequence of go/gosnarkhip.R1csSolvePlan / R1csSolveUnsolved / R1csSolve) and prints counts and witnesses.  Expectations are
Python integers (tests/solve_util.py)."""
import pytest

import gosnark_amd  # noqa: F401
import c_util
import solve_util as SU

pytestmark = pytest.mark.gpu
R = SU.R


def test_r1cs_solve_c_sequence_prints_the_plan_and_the_witnesses(tmp_path):
    # one, x, y | p = x * y, q: q * x = y, s = p + q + 5, v: v * v = s (never solved), t = v * x (hangs on v)
    m = 8
    row = lambda *entries: [dict(entries).get(i, 0) for i in range(m)]                       # noqa: E731
    a = [row((1, 1)), row((4, 1)), row((3, 1), (4, 1), (0, 5)), row((6, 1)), row((6, 1))]
    b = [row((2, 1)), row((1, 1)), row((0, 1)), row((6, 1)), row((1, 1))]
    c = [row((3, 1)), row((2, 1)), row((5, 1)), row((5, 1)), row((7, 1))]
    values = [[3, 12], [0, 7], [R - 1, 5]]                                                  # witness 1 divides by zero in row 1
    path = c_util.write_r1cs(tmp_path, (a, b, c), 0, [v for pair in values for v in pair], name="solve.bin")
    out = c_util.build_and_run("r1cs_solve.c", [path, "1", "2"], tmp_path).split("\n")
    sparse = lambda M: [[(i, v) for i, v in enumerate(r) if v] for r in M]                   # noqa: E731
    A, B, C = sparse(a), sparse(b), sparse(c)
    plan = SU.plan(A, B, C, m, [1, 2])
    assert plan["unsolved"] == [6, 7] and len(plan["entries"]) == 3
    assert out[0] == "plan solved 3 unsolved 2 checks 0 stuck 2 levels 2" and out[1] == "unsolved 6 7"
    limbs = lambda v: " ".join("%016x" % ((v >> (64 * i)) & (2 ** 64 - 1)) for i in range(4))              # noqa: E731
    for k, pair in enumerate(values):
        w, nfailed, first = SU.solve(A, B, C, m, [1, 2], pair, plan)
        assert (nfailed, first) == ((1, 1) if k == 1 else (0, None))
        assert out[2 + k] == "witness %d failed %d first %d %s" % (k, nfailed, 0xFFFFFFFF if first is None else first, " ".join(limbs(v) for v in w))
    assert out[5] == "DONE"
