"""The index arithmetic of the evaluation-basis derivation (go-snark-study_amd/csrc/evaltree.h: real leaves below a node, a child's
window, the slot of a block), instantiated on the HOST: tests/host/evaltree_host_test.hip replays the push-down of csrc/ecntt.hip
over Fr scalars with the functions the kernels use.  Compared with the definition, computed here with Python integers:
E[j-1] = sum_i coeff_i(l_j) h[i], l_j the Lagrange basis over the nodes n+1 .. 2n -- the solution of the transposed Vandermonde system
sum_j E[j-1] (n+j)^i = h[i]."""
import random

import pytest

import hostbuild
from oracle import ref_py as O

R = O.R


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build("evaltree_host_test")


def lagrange_rows(n):
    """coefficients (lowest first) of l_j, j = 1..n, over the nodes n+1 .. 2n: schoolbook products, one inversion per row"""
    nodes = [n + j for j in range(1, n + 1)]
    rows = []
    for xj in nodes:
        num, den = [1], 1
        for xk in nodes:
            if xk == xj:
                continue
            nxt = [0] * (len(num) + 1)
            for i, c in enumerate(num):                     # num * (x - xk)
                nxt[i] = (nxt[i] - c * xk) % R
                nxt[i + 1] = (nxt[i + 1] + c) % R
            num, den = nxt, den * (xj - xk) % R
        inv = pow(den, R - 2, R)
        rows.append([c * inv % R for c in num])
    return rows


def brute_force(n, h):
    return [sum(c * x for c, x in zip(row, h)) % R for row in lagrange_rows(n)]


def test_push_down_with_the_kernels_index_functions_solves_the_transposed_system_for_every_n_up_to_70(exe):
    rng = random.Random(70)
    sizes = list(range(1, 71))
    hs = [[rng.randrange(R) for _ in range(n)] for n in sizes]
    lines = ["%d %s" % (n, " ".join("%x" % v for v in h)) for n, h in zip(sizes, hs)]
    out = hostbuild.run_lines(exe, lines)
    for n, h, line in zip(sizes, hs, out):
        got = [int(t, 16) for t in line.split()]
        want = brute_force(n, h)
        assert got == want, n
        assert all(sum(e * pow(n + j + 1, i, R) for j, e in enumerate(got)) % R == h[i] for i in range(n)), n


def test_sparse_and_extreme_inputs(exe):
    """zeros where the device has points at infinity, r - 1, and a single non-zero power sum"""
    cases = []
    for n in (2, 5, 17, 33, 64, 65):
        cases.append((n, [0] * n))
        cases.append((n, [R - 1] * n))
        cases.append((n, [0] * (n - 1) + [1]))
        cases.append((n, [1] + [0] * (n - 1)))
        cases.append((n, [(i % 3 == 0) * (R - 1 - i) for i in range(n)]))
    out = hostbuild.run_lines(exe, ["%d %s" % (n, " ".join("%x" % v for v in h)) for n, h in cases])
    for (n, h), line in zip(cases, out):
        assert [int(t, 16) for t in line.split()] == brute_force(n, h), (n, h[:3])
