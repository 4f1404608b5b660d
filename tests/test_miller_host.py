"""The device tower and Miller loop (go-snark-study_amd/csrc/fq12.h, miller.h) instantiated on the HOST against the 4 x 64-bit
tower and pairing of pairing.h: Fq12 product, square and sparse line product on random and extremal operands, and
final_exponentiation(miller_loop(P, Q)) against the host pairing, bit for bit (the Miller values themselves differ by factors in
Fq2, which the final exponentiation removes)."""
import random

import pytest

import hostbuild
from oracle import ref_py as O

Q, R = O.Q, O.R
ONE12 = [1] + [0] * 11


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build("miller_host_test")


def hexes(vals):
    return " ".join("%x" % v for v in vals)


def ints(line):
    return [int(x, 16) for x in line.split()]


def operands():
    """Fq12 operands: random ones, and every coordinate 0, 1 or q - 1 in patterns that reach each Karatsuba sum."""
    rng = random.Random(2024)
    out = [[rng.randrange(Q) for _ in range(12)] for _ in range(6)]
    out += [[0] * 12, ONE12, [1] * 12, [Q - 1] * 12]
    out += [[(0, 1, Q - 1)[(i + k) % 3] for i in range(12)] for k in range(3)]
    out += [[Q - 1 if i == k else 0 for i in range(12)] for k in (0, 5, 6, 11)]
    out += [[rng.choice((0, 1, Q - 1)) for _ in range(12)] for _ in range(6)]
    return out


def test_product_and_square_equal_the_host_tower(exe):
    ops = operands()
    rng = random.Random(7)
    pairs = [(a, b) for a in ops[:10] for b in ops[:10]] + [(rng.choice(ops), rng.choice(ops)) for _ in range(40)]
    got = hostbuild.run_lines(exe, ["mul " + hexes(a) + " " + hexes(b) for a, b in pairs])
    for (a, b), line in zip(pairs, got):
        v = ints(line)
        assert len(v) == 24 and v[:12] == v[12:], (a, b)
    assert ints(got[pairs.index((ONE12, ops[0]))])[:12] == ops[0]            # the encoding is the one the test thinks it is
    got = hostbuild.run_lines(exe, ["sqr " + hexes(a) for a in ops])
    for a, line in zip(ops, got):
        v = ints(line)
        assert len(v) == 24 and v[:12] == v[12:], a


def test_line_product_equals_the_host_tower(exe):
    ops = operands()
    rng = random.Random(8)
    lines = [[rng.randrange(Q) for _ in range(6)] for _ in range(6)]
    lines += [[rng.randrange(Q), 0] + [rng.randrange(Q) for _ in range(4)] for _ in range(4)]      # l0 in Fq: the host's own shape
    lines += [[0] * 6, [1, 0, 0, 0, 0, 0], [Q - 1] * 6, [1] * 6, [Q - 1, 0, 1, Q - 1, 0, 1], [0, 0, Q - 1, Q - 1, 0, 0], [0, 0, 0, 0, 1, Q - 1]]
    cases = [(a, l) for a in ops[:12] for l in lines] + [(rng.choice(ops), rng.choice(lines)) for _ in range(30)]
    got = hostbuild.run_lines(exe, ["line " + hexes(a) + " " + hexes(l) for a, l in cases])
    in_fq = 0
    for (a, l), line in zip(cases, got):
        v = ints(line)
        assert len(v) == 36 and v[:12] == v[12:24], (a, l)
        if l[1] == 0:
            in_fq += 1
            assert v[:12] == v[24:], (a, l)
    assert in_fq >= 40


def g1(k):
    a = O.G1.Affine(O.G1.MulScalar(O.G1_GEN, k % R))
    return "inf" if a is None else "%x %x" % (a[0], a[1])


def g2(k):
    a = O.G2.Affine(O.G2.MulScalar(O.G2_GEN, k % R))
    return "inf" if a is None else "%x %x %x %x" % (a[0] + a[1])


def pair_values(exe, ab):
    got = hostbuild.run_lines(exe, ["pair %s %s" % (g1(a), g2(b)) for a, b in ab])
    out = []
    for (a, b), line in zip(ab, got):
        v = ints(line)
        assert len(v) == 24 and v[:12] == v[12:], (a, b)               # miller.h + final exponentiation == the host pairing
        out.append(v[:12])
    return out


def test_pairing_equals_the_host_pairing_bit_for_bit(exe):
    rng = random.Random(9)
    scalars = [1, 2, R - 1, rng.randrange(1, R)]
    vals = pair_values(exe, [(a, b) for a in scalars for b in scalars])
    assert vals[0] != ONE12                                              # the generators do not pair to one
    assert vals[scalars.index(R - 1) * 4 + scalars.index(R - 1)] == vals[0]     # e(-G1, -G2) = e(G1, G2)


def test_bilinearity(exe):
    rng = random.Random(10)
    for _ in range(2):
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        v = pair_values(exe, [(a, b), (a * b % R, 1), (1, a * b % R), (b, a)])
        assert v[0] == v[1] == v[2] == v[3]


def test_an_infinite_member_gives_one(exe):
    got = hostbuild.run_lines(exe, ["pair inf " + g2(5), "pair " + g1(5) + " inf", "pair inf inf"])
    for line in got:
        assert ints(line) == ONE12 + ONE12
