"""The device code under gs_pinocchio_verify_each instantiated on the HOST (tests/host/pinocchio_miller_host_test.hip): miller.h's
miller_loop_prepared (equations 1 and 3: every line prepared, no G2 arithmetic) and miller_loop_groth16 (equations 2, 4 and 5: PiB is
the live pair) with lists from pairing.h's prepare_g2_lines and the final exponentiation of finalexp.h, against pairing.h's
final_exponentiation(multi_miller_loop(...)) over the same pairs, bit for bit; and pinocchio_sums, the points kernel's arithmetic,
against the oracle's G1.Add (its G1.Double where the two operands are equal: the reference's Add has no branch for that case and
answers infinity, which neither the host verifier nor the device follows)."""
import random

import pytest

import hostbuild
import pinocchio_each_util as P
from oracle import ref_py as O

Q, R = O.Q, O.R
ONE12 = [1] + [0] * 11
LIVE = (False, True, False, True, True)                                  # which equations run PiB as a live pair


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build("pinocchio_miller_host_test")


def ints(line):
    return [int(x, 16) for x in line.split()]


def g1(k):
    a = O.G1.Affine(P.g1(k))
    return "inf" if a is None else "%x %x" % (a[0], a[1])


def g2(k):
    a = O.G2.Affine(P.g2(k))
    return "inf" if a is None else "%x %x %x %x" % (a[0] + a[1])


def request(live, pairs):
    pairs = list(pairs) + [(0, 0)] * (3 - len(pairs))
    return ("live3 " if live else "prep3 ") + " ".join("%s %s" % (g1(p), g2(q)) for p, q in pairs)


def values(exe, requests):
    """Every answer is the device code's value and pairing.h's: equal bit for bit.  Returns the value per request."""
    out = []
    for req, line in zip(requests, hostbuild.run_lines(exe, requests)):
        v = ints(line)
        assert len(v) == 24 and v[:12] == v[12:], req
        out.append(v[:12])
    return out


def test_the_five_equation_values_equal_the_hosts_and_are_one_for_a_valid_proof(exe):
    rng = random.Random(41)
    key = P.dlog_key(3, rng)
    signals = [rng.randrange(R), 0, R - 1]
    proof = P.dlog_proof(key, signals, rng)
    good = values(exe, [request(LIVE[e], pairs) for e, pairs in enumerate(P.equations(key, proof, signals))])
    assert good == [ONE12] * 5
    for moved, fails in (("PiA", {0, 3, 4}), ("PiB", {1, 3, 4}), ("PiC", {2, 3, 4}), ("PiH", {3}), ("PiKp", {4})):
        bad = dict(proof)
        bad[moved] = (bad[moved] + 1) % R
        got = values(exe, [request(LIVE[e], pairs) for e, pairs in enumerate(P.equations(key, bad, signals))])
        assert {e for e in range(5) if got[e] != ONE12} == fails, moved


def test_infinite_members_and_skip_flags_contribute_one(exe):
    rng = random.Random(42)
    k = [rng.randrange(1, R) for _ in range(6)]
    full = [(k[0], k[1]), (k[2], k[3]), (k[4], k[5])]
    for live in (False, True):
        cases = [full,
                 [(0, k[1]), full[1], full[2]], [full[0], (0, k[3]), full[2]], [full[0], full[1], (0, k[5])],      # an infinite G1 member
                 [(k[0], 0), full[1], full[2]], [full[0], (k[2], 0), full[2]], [full[0], full[1], (k[4], 0)],      # a set skip flag
                 [full[1], full[2]], [full[0], full[2]], [full[0], full[1]],                                       # the pair left out
                 [(0, 0)] * 3, [(0, k[1]), (k[2], 0), (0, 0)]]                                                      # all pairs skipped
        v = values(exe, [request(live, c) for c in cases])
        assert v[0] != ONE12 and v[10] == ONE12 and v[11] == ONE12
        for i in range(3):
            assert v[1 + i] == v[4 + i] == v[7 + i] != v[0], (live, i)
        assert len({tuple(x) for x in v[:4]}) == 4
    # the two loops agree with each other on the same pairs
    assert values(exe, [request(False, full)]) == values(exe, [request(True, full)])


def test_the_points_kernels_sums_with_infinity_and_doubling(exe):
    rng = random.Random(43)
    v, a, c = (rng.randrange(1, R) for _ in range(3))
    cases = [(v, a, c), (v, R - v, c), (v, v, c), (v, R - v, 0), (v, a, R - v - a), (v, a, v + a), (v, 0, c), (v, 0, 0), (0, a, c), (0, 0, c),
             (0, 0, 0), (v, v, 2 * v), (v, v, R - 2 * v), (1, 1, 1), (1, R - 1, 1)]
    got = hostbuild.run_lines(exe, ["sums %s %s %s" % (g1(x), g1(y), g1(z)) for x, y, z in cases])

    def show(p):
        p = O.G1.Affine(p)
        return "inf" if p is None else "%064x %064x" % (p[0], p[1])

    def add(p, q):
        # the reference's Add (bn128/g1.go:32-89) has no branch for equal operands and answers infinity there; its own Double is the sum
        if not O.G1.IsZero(p) and O.G1.Affine(p) == O.G1.Affine(q):
            return O.G1.Double(p)
        return O.G1.Add(p, q)
    for (x, y, z), line in zip(cases, got):
        xa, xac = [t.strip() for t in line.split("|")]
        want_xa = add(P.g1(x), P.g1(y))
        assert xa == show(want_xa), (x, y, z)
        assert xac == show(add(want_xa, P.g1(z))), (x, y, z)
        assert (xa == "inf") == ((x + y) % R == 0) and (xac == "inf") == ((x + y + z) % R == 0)
