"""The level plan and the launch schedule of gs_r1cs_solve (csrc/solve_plan.h) compiled for the CPU (tests/host/solve_plan_host_test.hip)
against the plan restated the slow way in Python integers (tests/solve_util.py): levels, (form, row) order, lowest-row tie, checks, the
unsolved list, and the run cuts at `narrow` and `run_max_rows`.  No GPU."""
import subprocess

import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import synth
import hostbuild
import solve_util as SU
from oracle import ref_py as O

R = SU.R


def run_driver(A, B, C, m, inputs, narrow=0, run_max_rows=0):
    exe = hostbuild.build("solve_plan_host_test")
    lines = ["%d %d %d %d %d" % (len(A), m, len(inputs), narrow, run_max_rows), " ".join(str(v) for v in inputs)]
    for M in (A, B, C):
        for row in M:
            lines.append(" ".join([str(len(row))] + ["%d %x" % (v, c) for v, c in row]))
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True)
    out = p.stdout.split("\n")
    status = [int(x) for x in out[0].split()[1:]]
    if status[0]:
        return dict(status=status)
    k = int(out[1].split()[1])
    entries = []
    for line in out[2:2 + k]:
        row, target, form, elem = line.split()
        entries.append((int(row), int(target), int(form), int(elem, 16)))
    rest = out[2 + k:]
    nl = int(rest[3].split()[1])
    return dict(status=status, entries=entries, levels=[int(x) for x in rest[0].split()[1:]], unsolved=[int(x) for x in rest[1].split()[1:]],
                checks=int(rest[2].split()[1]), stuck=int(rest[2].split()[2]),
                launches=[(int(a), int(b), bool(int(c))) for a, b, c in (ln.split() for ln in rest[4:4 + nl])],
                defaults=tuple(int(x) for x in rest[4 + nl].split()[1:]))


def agree(system, narrow=4, run_max_rows=16):
    A, B, C, m, inputs = system
    got, want = run_driver(A, B, C, m, inputs, narrow, run_max_rows), SU.plan(A, B, C, m, inputs)
    assert got["status"][0] == 0
    for key in ("entries", "levels", "unsolved", "checks", "stuck"):
        assert got[key] == want[key], key
    assert got["launches"] == SU.launches(want["levels"], narrow, run_max_rows)
    assert len(got["entries"]) + got["checks"] + got["stuck"] == len(A)
    return got


def x3():
    dense = lambda M: [[(v, c) for v, c in enumerate(row) if c] for row in M]      # noqa: E731
    return dense(O.X3_R1CS_A), dense(O.X3_R1CS_B), dense(O.X3_R1CS_C), 8, [2]


def sqchain(n):
    a, b, c, _ = synth.sqchain_r1cs(n, 5)
    return SU.from_csr(a), SU.from_csr(b), SU.from_csr(c), n + 1, [1]


def gates(n, seed, mul_share=0.5):
    a, b, c, _, _ = synth.gates_r1cs(n, seed, mul_share)
    return SU.from_csr(a), SU.from_csr(b), SU.from_csr(c), n + 1, [1]


def test_x3_has_five_levels_a_check_and_nothing_unsolved():
    got = agree(x3())
    assert len(got["levels"]) - 1 == 5 and got["unsolved"] == [] and got["checks"] == 1 and got["stuck"] == 0
    assert 5 not in [e[0] for e in got["entries"]] and sorted(e[0] for e in got["entries"]) == [0, 1, 2, 3, 4, 6]
    assert [e for e in got["entries"] if e[0] == 4] == [(4, 1, SU.FORM_C, 1)]          # rows 4 and 5 both define `out`: the lowest wins


@pytest.mark.parametrize("n", [1, 2, 40])
def test_sqchain(n):
    got = agree(sqchain(n))
    assert len(got["entries"]) == n - 1 and got["checks"] == 1 and got["unsolved"] == []
    assert all(hi - lo == 1 for lo, hi in zip(got["levels"], got["levels"][1:]))
    # a chain is one run, cut every 16 rows
    assert got["launches"] == [(lo, min(lo + 16, n - 1), True) for lo in range(0, n - 1, 16)]


@pytest.mark.parametrize("seed,mul_share", [(1, 0.5), (2, 0.9), (3, 0.1)])
def test_gates_of_2_10_rows(seed, mul_share):
    got = agree(gates(1 << 10, seed, mul_share), narrow=8, run_max_rows=32)
    assert got["unsolved"] == [] and got["stuck"] == 0 and got["checks"] == 1 and len(got["entries"]) == (1 << 10) - 1
    assert any(run for _, _, run in got["launches"]) and any(not run for _, _, run in got["launches"])
    # the defaults (0, 0) give the schedule of knobs.h's values
    A, B, C, m, inputs = gates(1 << 10, seed, mul_share)
    dflt = run_driver(A, B, C, m, inputs)
    assert dflt["launches"] == SU.launches(dflt["levels"], *dflt["defaults"]) and dflt["entries"] == got["entries"]


def test_an_unknown_in_two_matrices_defines_nothing_and_holds_back_what_hangs_below():
    # variables: one, x, v, k, t, u.   row 0: x * x = k;  row 1: v * v = k (v in A and B: never solved);  row 2: v * x = t (hangs on v);
    # row 3: k * x = u (independent of v)
    A = [[(1, 1)], [(2, 1)], [(2, 1)], [(3, 1)]]
    B = [[(1, 1)], [(2, 1)], [(1, 1)], [(1, 1)]]
    C = [[(3, 1)], [(3, 1)], [(4, 1)], [(5, 1)]]
    got = agree((A, B, C, 6, [1]))
    assert got["unsolved"] == [2, 4] and got["stuck"] == 2 and got["checks"] == 0 and [e[:2] for e in got["entries"]] == [(0, 3), (3, 5)]


def test_duplicate_columns_are_summed_and_cancelling_ones_define_nothing():
    # row 0: (x + x + 3 one) * one = y with y named twice in C (2 + r - 1 = 1);  row 1: z named in C with coefficients 5 and r - 5 (cancel)
    # next to u: two unknowns, then one whose coefficient is zero;  row 2: y * x = u defines u;  row 3: (a - a) * one = ... a cancels in A,
    # sits in C: form C all the same, since A's sum is zero
    A = [[(1, 1), (0, 3), (1, 1)], [(1, 1)], [(2, 1)], [(5, 4), (5, R - 4), (1, 1)]]
    B = [[(0, 1)], [(0, 1)], [(1, 1)], [(0, 1)]]
    C = [[(2, 2), (2, R - 1)], [(3, 5), (4, 1), (3, R - 5)], [(4, 1)], [(5, 7)]]
    got = agree((A, B, C, 6, [1]))
    assert got["unsolved"] == [3] and got["stuck"] == 1
    assert (3, 5, SU.FORM_C, pow(7, R - 2, R)) in got["entries"] and (0, 2, SU.FORM_C, 1) in got["entries"]


def test_forms_a_and_b_and_the_order_inside_a_level():
    # out * v = u (form A), v * out = u (form B), and a product, all at level 1: ordered C, A, B whatever the rows' order
    A = [[(3, 2)], [(1, 1)], [(1, 1)]]
    B = [[(1, 1)], [(4, 3)], [(2, 1)]]
    C = [[(2, 1)], [(2, 1)], [(5, R - 1)]]
    got = agree((A, B, C, 6, [1, 2]))
    assert [e[:3] for e in got["entries"]] == [(2, 5, SU.FORM_C), (0, 3, SU.FORM_A), (1, 4, SU.FORM_B)]
    assert [e[3] for e in got["entries"]] == [pow(R - 1, R - 2, R), 2, 3]


def test_inputs_covering_every_variable_give_an_empty_plan():
    A, B, C, m, _ = x3()
    got = agree((A, B, C, m, list(range(1, m))))
    assert got["entries"] == [] and got["levels"] == [0] and got["launches"] == [] and got["checks"] == 7


def test_level_widths_and_seams():
    for ws in ([3, 4, 5, 1, 1, 1, 1, 6, 2], [1] * 16, [1] * 17, [1] * 33, [4], [3]):
        got = agree(SU.widths(ws))
        assert [hi - lo for lo, hi in zip(got["levels"], got["levels"][1:])] == ws
    assert SU.launches([0, 3, 7, 12, 13, 14], 4, 16) == [(0, 3, True), (3, 7, False), (7, 12, False), (12, 14, True)]


def test_bad_inputs_are_named():
    A, B, C, m, _ = x3()
    assert run_driver(A, B, C, m, [2, 8])["status"] == [1, 1]
    assert run_driver(A, B, C, m, [0])["status"] == [2, 0]
    assert run_driver(A, B, C, m, [2, 3, 2])["status"] == [3, 2]
