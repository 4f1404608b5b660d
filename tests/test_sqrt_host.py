"""Square roots in Fq and Fq2 and the sign rule of compressed points (go-snark-study_amd/csrc/sqrt.h) instantiated on the HOST.  The
expected value is never the code's own: whether an element has a root is Euler's criterion with Python's pow, a returned root is checked
by squaring it, and the "largest" predicate against the comparison of integers."""
import random

import pytest

import hostbuild
from oracle import ref_py as O

Q = O.Q
TWIST_B = O.FQ2.Mul(O.FQ2.Inverse((9, 1)), (3, 0))


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build("sqrt_host_test")


def f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_mul(a, a)
        e >>= 1
    return r


def fq_has_root(a):
    return a % Q == 0 or pow(a, (Q - 1) // 2, Q) == 1


def fq2_has_root(a):
    """Euler's criterion in Fq2: a^((q^2 - 1)/2) = 1."""
    return a == (0, 0) or f2_pow(a, (Q * Q - 1) // 2) == (1, 0)


def fq_largest(y):
    return y > Q - y if y else False


def fq2_largest(y):
    return fq_largest(y[1]) if y[1] else fq_largest(y[0])


def twist_rhs(x):
    return O.FQ2.Add(f2_mul(f2_mul(x, x), x), TWIST_B)


def run_fq(exe, vals):
    out = []
    for line in hostbuild.run_lines(exe, ["fq %x" % a for a in vals]):
        ok, y, big = line.split()
        out.append((ok == "1", int(y, 16), big == "1"))
    return out


def run_fq2(exe, vals):
    out = []
    for line in hostbuild.run_lines(exe, ["fq2 %x %x" % a for a in vals]):
        ok, y0, y1, big = line.split()
        out.append((ok == "1", (int(y0, 16), int(y1, 16)), big == "1"))
    return out


def check_fq(exe, vals):
    count = [0, 0]
    for a, (ok, y, big) in zip(vals, run_fq(exe, vals)):
        want = fq_has_root(a)
        count[want] += 1
        assert ok == want, hex(a)
        assert y < Q
        if want:
            assert y * y % Q == a % Q, hex(a)
            assert big == fq_largest(y), hex(a)
    return count


def check_fq2(exe, vals):
    count = [0, 0]
    for a, (ok, y, big) in zip(vals, run_fq2(exe, vals)):
        want = fq2_has_root(a)
        count[want] += 1
        assert ok == want, a
        assert y[0] < Q and y[1] < Q
        if want:
            assert f2_mul(y, y) == a, a
            assert big == fq2_largest(y), a
    return count


def test_fq_random_values_have_a_root_exactly_when_euler_says_so(exe):
    rng = random.Random(7)
    none, some = check_fq(exe, [rng.randrange(Q) for _ in range(200)])
    assert some >= 60 and none >= 60


def test_fq_special_values(exe):
    assert check_fq(exe, [0, 1, Q - 1, 4]) == [1, 3]                 # -1 is the non-residue
    assert check_fq(exe, [(0 ** 3 + 3) % Q]) == [1, 0]               # the right-hand side of E at x = 0
    got = run_fq(exe, [0, 1, 4])
    assert got[0][1] == 0 and got[1][1] in (1, Q - 1) and got[2][1] in (2, Q - 2)


def test_fq2_random_twist_right_hand_sides(exe):
    rng = random.Random(7)
    vals = [twist_rhs((rng.randrange(Q), rng.randrange(Q))) for _ in range(200)]
    none, some = check_fq2(exe, vals)
    assert some >= 60 and none >= 60


def test_fq2_squares_of_random_elements_have_roots(exe):
    rng = random.Random(8)
    xs = [(rng.randrange(Q), rng.randrange(Q)) for _ in range(200)]
    vals = [f2_mul(x, x) for x in xs]
    assert check_fq2(exe, vals) == [0, 200]
    for x, (_, y, _) in zip(xs, run_fq2(exe, vals)):
        assert y == x or y == ((-x[0]) % Q, (-x[1]) % Q)


def test_fq2_special_cases_all_have_roots(exe):
    vals = [(5, 0), (Q - 5, 0), (0, 7), (0, Q - 7), (0, 0), (1, 0), (Q - 1, 0)]
    assert check_fq2(exe, vals) == [0, len(vals)]
    assert run_fq2(exe, [(0, 0)])[0][1] == (0, 0)
    assert run_fq2(exe, [(Q - 1, 0)])[0][1] in ((0, 1), (0, Q - 1))


def test_fq2_twist_right_hand_side_at_zero_has_no_root(exe):
    assert not fq2_has_root(twist_rhs((0, 0)))
    assert check_fq2(exe, [twist_rhs((0, 0))]) == [1, 0]


def test_largest_is_the_integer_comparison(exe):
    rng = random.Random(9)
    half = (Q - 1) // 2
    ys = [0, 1, half - 1, half, half + 1, half + 2, Q - 1, Q - 2] + [rng.randrange(Q) for _ in range(40)]
    got = hostbuild.run_lines(exe, ["big %x" % y for y in ys])
    assert [g == "1" for g in got] == [fq_largest(y) for y in ys]
    pairs = [(a, b) for a in (0, 1, half, half + 1, Q - 1) for b in (0, 1, half, half + 1, Q - 1)] + [(rng.randrange(Q), rng.randrange(Q)) for _ in range(20)]
    got = hostbuild.run_lines(exe, ["big2 %x %x" % p for p in pairs])
    assert [g == "1" for g in got] == [fq2_largest(p) for p in pairs]
    for y in ys[1:]:
        assert fq_largest(y) != fq_largest(Q - y)                    # exactly one of {y, -y} is the largest (q is odd)
