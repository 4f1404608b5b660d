"""G2 subgroup membership (go-snark-study_amd/csrc/g2_subgroup.h) instantiated on the HOST: the verdict on every point against
the definition [r] Q = O from oracle/ref_py and against the independent 4 x 64-bit test of pairing.h; psi against the oracle-side
psi computed from the definition of its constants."""
import random

import pytest

import hostbuild
import membership_util as M
from oracle import ref_py as O


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build("g2_subgroup_host_test")


def fmt(p):
    a = M.affine(p)
    return "inf" if a is None else "%x %x %x %x" % (a[0] + a[1])


def parse(line):
    if line.strip() == "inf":
        return None
    v = [int(x, 16) for x in line.split()]
    return ((v[0], v[1]), (v[2], v[3]))


@pytest.fixture(scope="module")
def points():
    """(label, point) over every kind the membership test has to tell apart."""
    rng = random.Random(41)
    pts = [("infinity", O.G2_ZERO)]
    ks = [1, 2, 3, M.R - 1, M.R - 2, M.BN_X, M.BN_X + 1, 6 * M.BN_X ** 2] + [rng.randrange(1, M.R) for _ in range(26)]
    pts += [("%d G" % k, O.G2.MulScalar(O.G2_GEN, k)) for k in ks]
    twist = M.twist_points(4)
    pts += [("twist %d" % i, t) for i, t in enumerate(twist)]
    pts += [("cleared %d" % i, O.G2.MulScalar(t, M.COFACTOR)) for i, t in enumerate(twist)]
    for which in (0, 1):
        s = M.small_order_point(which)
        pts += [("S%d" % which, s), ("2 S%d" % which, O.G2.Double(s)), ("-S%d" % which, O.G2.Neg(s)),
                ("5034 S%d" % which, O.G2.MulScalar(s, 5034)), ("5035 S%d" % which, O.G2.MulScalar(s, 5035))]
        pts += [("%d G + S%d" % (k, which), M.complete_add(O.G2.MulScalar(O.G2_GEN, k), s)) for k in (1, 7, M.R - 1, rng.randrange(1, M.R))]
    return pts


def test_membership_equals_the_definition_and_the_host_verifier(exe, points):
    want = [M.in_subgroup(p) for _, p in points]
    assert sum(want) >= 33 + 4 and want.count(False) >= 4 + 10 + 8              # the set holds what it is meant to hold
    got = hostbuild.run_lines(exe, ["member " + fmt(p) for _, p in points])
    for (label, _), w, line in zip(points, want, got):
        assert line.split() == [str(int(w))] * 2, label


def test_psi_equals_its_definition(exe, points):
    some = [p for _, p in points]
    got = hostbuild.run_lines(exe, ["psi " + fmt(p) for p in some])
    for (label, p), line in zip(points, got):
        assert parse(line) == M.affine(M.psi(p)), label
    # the XYZZ overload, on a point whose denominators are not 1
    finite = [p for p in some if not O.G2.IsZero(p)][:12]
    got = hostbuild.run_lines(exe, ["psixyzz " + fmt(p) for p in finite])
    for p, line in zip(finite, got):
        assert parse(line) == M.affine(M.psi(O.G2.Double(p)))


def test_psi_acts_on_the_subgroup_as_q(exe):
    rng = random.Random(42)
    gs = [O.G2.MulScalar(O.G2_GEN, k) for k in (1, M.R - 1, rng.randrange(1, M.R), rng.randrange(1, M.R))]
    got = hostbuild.run_lines(exe, ["psi " + fmt(p) for p in gs])
    for p, line in zip(gs, got):
        assert parse(line) == M.affine(O.G2.MulScalar(p, M.Q % M.R))
    assert M.Q % M.R == 6 * M.BN_X ** 2
