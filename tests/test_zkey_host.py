"""The two number conversions of a .zkey (csrc/zkey_convert.h), instantiated on the HOST (tests/host/zkey_host_test.hip) and compared
with Python integers: a coordinate value * 2^256 mod q becomes the engine's element of that value, a coefficient v * 2^512 mod r becomes
v, and the range test says whether a word is below the modulus.  No GPU."""
import random

import pytest

import hostbuild
import circom_util as CU
from gosnark_amd import circom

R, Q = CU.R, circom.Q


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build("zkey_host_test")


def cases(p):
    rng = random.Random(2024 + p % 1000)
    return [0, 1, p - 1, (1 << 256) % p] + [rng.randrange(p) for _ in range(20)]


def ask(exe, which, words):
    return [line.split() for line in hostbuild.run_lines(exe, ["%s %064x" % (which, w) for w in words])]


def test_coordinate_conversion_matches_python(exe):
    vals = cases(Q)
    words = [v * (1 << 256) % Q for v in vals]                       # what the file holds for the value v
    for v, (below, got) in zip(vals, ask(exe, "q", words)):
        assert below == "1" and int(got, 16) == v
    # the bytes themselves as values: 0, 1, q - 1, 2^256 mod q and the seeded ones, read as Montgomery words
    inv = pow(1 << 256, -1, Q)
    for wd, (below, got) in zip(vals, ask(exe, "q", vals)):
        assert below == "1" and int(got, 16) == wd * inv % Q


def test_coefficient_conversion_matches_python(exe):
    vals = cases(R)
    words = [v * pow(2, 512, R) % R for v in vals]
    for v, (_, got) in zip(vals, ask(exe, "r", words)):
        assert int(got, 16) == v
    inv = pow(pow(2, 512, R), -1, R)
    for wd, (_, got) in zip(vals, ask(exe, "r", vals)):
        assert int(got, 16) == wd * inv % R


def test_range_test_and_words_at_or_above_the_modulus(exe):
    top = (1 << 256) - 1
    for which, p, shift in (("q", Q, 256), ("r", R, 512)):
        words = [p - 1, p, p + 1, 2 * p, top]
        inv = pow(pow(2, shift, p), -1, p)
        for wd, (below, got) in zip(words, ask(exe, which, words)):
            assert below == ("1" if wd < p else "0")
            assert int(got, 16) == wd * inv % p                       # any 256-bit word converts as its residue
