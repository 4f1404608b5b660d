"""The rest of the device tower and the final exponentiation (go-snark-study_amd/csrc/finalexp.h) instantiated on the HOST against
the 4 x 64-bit tower of pairing.h, every result bit for bit: conjugate, inverse, Frobenius maps, cyclotomic square and x-th power
on unitary elements, the final exponentiation on arbitrary elements and on Miller values of miller.h, and the Frobenius constants
of bn128_constants.h against the ones pairing.h computes at run time."""
import random

import pytest

import hostbuild
from oracle import ref_py as O

Q, R = O.Q, O.R
ONE12 = [1] + [0] * 11


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build("finalexp_host_test")


def hexes(vals):
    return " ".join("%x" % v for v in vals)


def ints(line):
    return [int(x, 16) for x in line.split()]


def operands():
    """The operands of test_miller_host.operands(): random ones, and every coordinate 0, 1 or q - 1 in patterns."""
    rng = random.Random(2024)
    out = [[rng.randrange(Q) for _ in range(12)] for _ in range(6)]
    out += [[0] * 12, ONE12, [1] * 12, [Q - 1] * 12]
    out += [[(0, 1, Q - 1)[(i + k) % 3] for i in range(12)] for k in range(3)]
    out += [[Q - 1 if i == k else 0 for i in range(12)] for k in (0, 5, 6, 11)]
    out += [[rng.choice((0, 1, Q - 1)) for _ in range(12)] for _ in range(6)]
    return out


def both(exe, requests, parts=2):
    """Runs the requests; every answer is `parts` Fq12 values that must all be equal.  Returns that value per request."""
    got = hostbuild.run_lines(exe, requests)
    out = []
    for req, line in zip(requests, got):
        v = ints(line)
        assert len(v) == 12 * parts, req
        for k in range(1, parts):
            assert v[:12] == v[12 * k:12 * k + 12], (req, k)
        out.append(v[:12])
    return out


def test_conjugate_and_frobenius_equal_the_host_tower(exe):
    ops = operands()
    vals = both(exe, ["conj " + hexes(a) for a in ops])
    assert vals[ops.index(ONE12)] == ONE12
    assert vals[0][:6] == ops[0][:6] and vals[0][6:] == [Q - c for c in ops[0][6:]]    # the encoding is the one the test thinks it is
    for k in (1, 2, 3):
        vals = both(exe, ["frob %d " % k + hexes(a) for a in ops])
        assert vals[ops.index(ONE12)] == ONE12
        assert vals[0] != ops[0]


def test_inverse_equals_the_host_tower_and_zero_terminates(exe):
    ops = operands()
    got = hostbuild.run_lines(exe, ["inv " + hexes(a) for a in ops])
    units = 0
    for a, line in zip(ops, got):
        v = ints(line)
        assert len(v) == 36 and v[:12] == v[24:], a                      # finalexp.h == pairing.h
        if v[12:24] == ONE12:
            units += 1
        else:                                                            # a zero divisor of the norm chain: both towers answer 0
            assert v[:12] == [0] * 12, a
    assert ints(got[ops.index([0] * 12)])[:12] == [0] * 12               # inv(0) = 0, and it came back
    assert units >= 12


def unitary_sources():
    rng = random.Random(11)
    return [[rng.randrange(Q) for _ in range(12)] for _ in range(5)] + [ONE12, [1] * 12, [Q - 1] * 12]


def test_easy_part_equals_the_host_tower(exe):
    vals = both(exe, ["easy " + hexes(a) for a in unitary_sources()])
    assert vals[5] == ONE12


def test_cyclotomic_square_on_unitary_elements(exe):
    # the header's cyclotomic square, fq12.h's ordinary square, pairing.h's cyclotomic square: all three equal
    src = unitary_sources()
    vals = both(exe, ["cyc " + hexes(a) for a in src], parts=3)
    assert vals[5] == ONE12 and vals[0] != ONE12


def test_pow_x_on_unitary_elements(exe):
    src = unitary_sources()
    vals = both(exe, ["powx " + hexes(a) for a in src])
    assert vals[5] == ONE12 and vals[0] != ONE12


def test_final_exponentiation_equals_the_host_bit_for_bit(exe):
    rng = random.Random(12)
    src = [[rng.randrange(Q) for _ in range(12)] for _ in range(6)] + [ONE12] + operands()[6:14]
    vals = both(exe, ["fe " + hexes(a) for a in src])
    assert vals[6] == ONE12
    assert vals[0] != ONE12


def g1(k):
    a = O.G1.Affine(O.G1.MulScalar(O.G1_GEN, k % R))
    return "inf" if a is None else "%x %x" % (a[0], a[1])


def g2(k):
    a = O.G2.Affine(O.G2.MulScalar(O.G2_GEN, k % R))
    return "inf" if a is None else "%x %x %x %x" % (a[0] + a[1])


def pairings(exe, ab):
    got = hostbuild.run_lines(exe, ["pairfe %s %s" % (g1(a), g2(b)) for a, b in ab])
    out = []
    for (a, b), line in zip(ab, got):
        v = ints(line)
        assert len(v) == 25 and v[:12] == v[13:], (a, b)                 # miller.h + finalexp.h == the host pairing
        assert v[12] == (1 if v[:12] == ONE12 else 0), (a, b)            # f12_is_one
        out.append(v[:12])
    return out


def test_final_exponentiation_of_miller_values(exe):
    rng = random.Random(13)
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    v = pairings(exe, [(1, 1), (a, b), (a * b % R, 1), (R - 1, R - 1), (0, 5), (5, 0), (0, 0)])
    assert v[0] != ONE12 and v[1] == v[2] and v[3] == v[0]
    assert v[4] == v[5] == v[6] == ONE12                                 # an infinite member gives one


def test_frobenius_constants_equal_the_host_ones(exe):
    v = ints(hostbuild.run_lines(exe, ["consts"])[0])
    assert len(v) == 60 and v[:30] == v[30:]
    assert v[0:2] != [1, 0] and all(v[10 + 2 * i + 1] == 0 for i in range(5))        # gamma_2 is in Fq


def test_three_pairs_in_one_accumulator_with_prepared_lines(exe):
    """miller.h's miller_loop_groth16 -- (P1, Q1) on projective steps, (P2, gamma) and (P3, delta) on prepared lines, one accumulator --
    exponentiated, against pairing.h's multi_miller_loop + final_exponentiation of the same three pairs."""
    rng = random.Random(14)
    k = [rng.randrange(1, R) for _ in range(6)]
    cases = [k, [1, 1, 1, 1, 1, 1], [R - 1, k[1], k[2], k[3], 2, R - 1],
             [0, k[1], k[2], k[3], k[4], k[5]], [k[0], 0, k[2], k[3], k[4], k[5]],       # an infinite P1, an infinite Q1
             [k[0], k[1], 0, k[3], k[4], k[5]], [k[0], k[1], k[2], k[3], 0, k[5]],       # an infinite P2, an infinite P3
             [k[0], k[1], k[2], 0, k[4], k[5]], [k[0], k[1], k[2], k[3], k[4], 0],       # an infinite gamma, an infinite delta
             [0, 0, 0, 0, 0, 0]]
    a, b = rng.randrange(1, R), rng.randrange(1, R)
    cases.append([R - a, b, a * b % R, 1, 5, 0])                         # e(-aG, bH) e(abG, H) = 1
    got = hostbuild.run_lines(exe, ["groth3 %s %s %s %s %s %s" % (g1(c[0]), g2(c[1]), g1(c[2]), g2(c[3]), g1(c[4]), g2(c[5])) for c in cases])
    vals = []
    for c, line in zip(cases, got):
        v = ints(line)
        assert len(v) == 24 and v[:12] == v[12:], c
        vals.append(v[:12])
    assert vals[0] != ONE12 and vals[9] == ONE12 and vals[10] == ONE12
    assert vals[3] == vals[4] and vals[5] == vals[7] and vals[6] == vals[8]          # the same pair dropped, by its P or by its Q
    assert len({tuple(v) for v in (vals[0], vals[1], vals[2], vals[3], vals[5], vals[6])}) == 6


def vkx_line(ic, scalars):
    return "vkx %d %s %s" % (len(scalars), " ".join(g1(k) for k in ic), hexes(scalars))


def test_vkx_equals_accumulate_ic(exe):
    """miller.h's groth16_vkx (joint double-and-add, complete formulas) against verify.hip's accumulate_ic restated on pairing.h."""
    rng = random.Random(15)
    special = [0, 1, R - 1, R, 2 ** 256 - 1, rng.randrange(R), rng.randrange(2 ** 256)]
    lines, want = [], []
    for npublic in (0, 1, 3):
        for _ in range(3 if npublic == 0 else 10):
            ic = [rng.randrange(1, R) for _ in range(npublic + 1)]
            sc = [rng.choice(special) for _ in range(npublic)]
            lines.append(vkx_line(ic, sc))
            want.append((ic[0] + sum(s * k for s, k in zip(sc, ic[1:]))) % R)
        for s in special:
            ic = [rng.randrange(1, R) for _ in range(npublic + 1)]
            sc = [s] * npublic
            lines.append(vkx_line(ic, sc))
            want.append((ic[0] + sum(x * k for x, k in zip(sc, ic[1:]))) % R)
    # two signals on the same IC point value: the second addition meets the doubling; the same with opposite points; sums that vanish
    p = rng.randrange(1, R)
    for ic, sc in (([7, p, p, 9], [5, 5, 1]), ([7, p, R - p, 9], [5, 5, 0]), ([p, p, p, p], [1, 1, 1]), ([p, R - p], [1]), ([0, p, p, 0], [3, R - 3, 8]),
                   ([p, 1], [R - p]), ([0, 0], [5])):
        lines.append(vkx_line(ic, sc))
        want.append((ic[0] + sum(x * k for x, k in zip(sc, ic[1:]))) % R)
    got = hostbuild.run_lines(exe, lines)
    for line, text, k in zip(lines, got, want):
        mine, host = [t.strip() for t in text.split("|")]
        assert mine == host, line
        assert (mine == "inf") == (k == 0), line
        if k:
            x, y = O.G1.Affine(O.G1.MulScalar(O.G1_GEN, k))[:2]
            assert ints(mine) == [x, y], line
