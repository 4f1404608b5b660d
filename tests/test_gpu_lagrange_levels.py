"""-m gpu: gs_g1_lagrange_levels / gs_g2_lagrange_levels -- the Lagrange bases of every domain 2^lo .. 2^hi in shared launches -- and
gs_g*_lagrange_levels_check, the two sums that check such an array without a transform in the group.

As in test_gpu_lagrange.py every input point is a known multiple of the generator (gs_g*_fixed_base), the expected output is the O(n^2)
definition of every level evaluated on the SCALARS in Python integers, times the generator, and the comparison is bit for bit on the
downloaded affine points.  Nothing is compared against gs_g*_lagrange alone."""
import ctypes
import functools
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi
import circom_util as CU

pytestmark = pytest.mark.gpu
R = CU.R
GS_ERR_ARG, GS_ERR_SHAPE = -3, -4
# hi = 7 / 8: 127 / 255 butterflies of mixed levels in two / four 64-thread blocks; (3, 7), (2, 4): lo > 0 moves the first butterfly's
# number; (5, 5), (0, 0): one level
G1_CASES = [(0, 0), (0, 1), (0, 7), (3, 7), (5, 5), (0, 8)]
G2_CASES = [(0, 0), (0, 5), (2, 4), (0, 7)]


@pytest.fixture(autouse=True)
def _init():
    capi.init()


def fixed(scalars, g2=False):
    return (capi.g2_fixed_base if g2 else capi.g1_fixed_base)(CU.u64(scalars))


def rows(handle, g2=False):
    return (capi.g2_download if g2 else capi.g1_download)(handle)


def assert_points(handle, scalars, g2=False):
    assert len(handle) == len(scalars)
    assert np.array_equal(rows(handle, g2), rows(fixed(scalars, g2), g2))


@functools.lru_cache(maxsize=None)
def transform(s, k):
    """out[j] = (1/n) sum_{i<n} w^(-ij) s_i over the first n = 2^k of s (a tuple; a missing s[n-1] is 0)"""
    n = 1 << k
    s = tuple(s[:n]) + (0,) * (n - len(s[:n]))
    wi = pow(CU.omega(k), -1, R)
    pw = [pow(wi, e, R) for e in range(n)]
    ninv = pow(n, -1, R)
    return tuple(sum(s[i] * pw[i * j % n] for i in range(n)) * ninv % R for j in range(n))


def levels(s, lo, hi):
    out = []
    for p in range(lo, hi + 1):
        out += transform(tuple(s), p)
    return out


def tau_powers(count, seed):
    tau = random.Random(seed).randrange(2, R)
    out = [1]
    for _ in range(count - 1):
        out.append(out[-1] * tau % R)
    return out


def planted(count, n, seed):
    """random multiples with infinities, equal pairs and opposite pairs at the partners of a butterfly of the smallest span (i / i + 1)
    and of the largest (i / i + n/2)"""
    rng = random.Random(seed)
    s = [rng.randrange(1, R) for _ in range(count)]
    at = 0
    for d in [d for d in (1, n // 2) if 0 < d < count]:
        for kind in ("equal", "opposite", "inf-lo", "inf-hi", "inf-both"):
            i = at % max(count - d, 1)
            at += 3
            if kind == "equal":
                s[i + d] = s[i]
            elif kind == "opposite":
                s[i + d] = (R - s[i]) % R
            elif kind == "inf-lo":
                s[i] = 0
            elif kind == "inf-hi":
                s[i + d] = 0
            else:
                s[i] = s[i + d] = 0
    return s


@pytest.mark.parametrize("lo,hi", G1_CASES)
def test_g1_lagrange_levels(lo, hi):
    n = 1 << hi
    for s in (tau_powers(n, 100 + 10 * hi + lo), planted(n, n, 200 + 10 * hi + lo)):
        out = capi.g1_lagrange_levels(fixed(s), lo, hi)
        assert len(out) == (2 << hi) - (1 << lo)
        assert_points(out, levels(s, lo, hi))
    assert capi.last_timing()["total_ms"] > 0


@pytest.mark.parametrize("lo,hi", G2_CASES)
def test_g2_lagrange_levels(lo, hi):
    n = 1 << hi
    for s in (tau_powers(n, 300 + 10 * hi + lo), planted(n, n, 400 + 10 * hi + lo)):
        assert_points(capi.g2_lagrange_levels(fixed(s, True), lo, hi), levels(s, lo, hi), True)


def test_a_longer_array_counts_only_its_first_points():
    s = planted(37, 16, 500)
    assert_points(capi.g1_lagrange_levels(fixed(s), 1, 4), levels(s[:16], 1, 4))
    assert_points(capi.g2_lagrange_levels(fixed(s, True), 1, 4), levels(s[:16], 1, 4), True)


@pytest.mark.parametrize("hi", [1, 4])
def test_short_last_level(hi):
    """exactly 2^hi - 1 points: the missing last point of level hi is the point at infinity, the lower levels are untouched"""
    n = 1 << hi
    s = planted(n, n, 600 + hi)
    s[n - 1] = 98765                                   # the full array differs from the short one in level hi
    for g2 in (False, True):
        f = capi.g2_lagrange_levels if g2 else capi.g1_lagrange_levels
        short, full = f(fixed(s[:n - 1], g2), 0, hi), f(fixed(s, g2), 0, hi)
        assert_points(short, levels(s[:n - 1] + [0], 0, hi), g2)
        assert_points(full, levels(s, 0, hi), g2)
        a, b = rows(short, g2), rows(full, g2)
        assert np.array_equal(a[:n - 1], b[:n - 1]) and not np.array_equal(a[n - 1:], b[n - 1:])


def refused(code, what, fn, *args, **kw):
    with pytest.raises(capi.GosnarkHipError, match=what) as e:
        fn(*args, **kw)
    assert e.value.code == code


def test_refusals():
    p1, p2 = fixed([1, 2, 3, 4]), fixed([1, 2, 3, 4], True)
    refused(GS_ERR_ARG, "gs_g1_lagrange_levels: bad base-array handle", capi.g1_lagrange_levels, p2, 0, 1)
    refused(GS_ERR_ARG, "gs_g2_lagrange_levels: bad base-array handle", capi.g2_lagrange_levels, p1, 0, 1)
    refused(GS_ERR_ARG, "bad base-array handle", capi.g1_lagrange_levels, 987654321, 0, 1)
    refused(GS_ERR_ARG, r"levels 2 \.\. 1, must be 0 <= lo <= hi <= 27", capi.g1_lagrange_levels, p1, 2, 1)
    refused(GS_ERR_ARG, r"levels 0 \.\. 28, must be 0 <= lo <= hi <= 27", capi.g1_lagrange_levels, p1, 0, 28)
    refused(GS_ERR_ARG, r"levels 28 \.\. 28, must be 0 <= lo <= hi <= 27", capi.g2_lagrange_levels, p2, 28, 28)
    refused(GS_ERR_SHAPE, r"the array has 4 points, level 3 needs 8 \(or 7 and a last point at infinity\)", capi.g1_lagrange_levels, p1, 0, 3)
    refused(GS_ERR_SHAPE, r"the array has 4 points, level 3 needs 8 \(or 7 and a last point at infinity\)", capi.g2_lagrange_levels, p2, 3, 3)
    lib = capi.load_library()
    for name, p in (("gs_g1_lagrange_levels", p1), ("gs_g2_lagrange_levels", p2)):
        assert getattr(lib, name)(capi.raw(p), 0, 1, None) == GS_ERR_ARG and b"bad base-array handle" in lib.gs_last_error()
    assert len(capi.g1_lagrange_levels(fixed([1, 2, 3]), 0, 2)) == 7          # 3 = 2^hi - 1 points: accepted


# ---- the check ----------------------------------------------------------------------------------------------------------------------
def point_of(scalar, g2=False):
    """scalar * generator as the affine int tuple a check result carries (None = infinity)"""
    if scalar % R == 0:
        return None
    return capi.msm(fixed([1], g2), CU.u64([scalar % R]), 0, g2)


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("hi", [0, 1, 5])
def test_levels_check_accepts_the_levels_and_names_both_sums(hi, g2):
    n = 1 << hi
    s = planted(n, n, 700 + hi)
    lv = levels(s, 0, hi)
    check = capi.g2_lagrange_levels_check if g2 else capi.g1_lagrange_levels_check
    ch = random.Random(710 + hi).randrange(1, R)
    name, ok, lhs, rhs = check(fixed(s, g2), fixed(lv, g2), hi, ch, name="mine")
    assert (name, ok) == ("mine", True) and lhs == rhs
    # both sides are sum_i ch^(i+1) lv[i] times the generator
    want = sum(pow(ch, i + 1, R) * v for i, v in enumerate(lv)) % R
    assert lhs == point_of(want, g2)
    # the levels of the computed array pass, a longer levels array counts only its prefix, a shorter hi checks a prefix
    f = capi.g2_lagrange_levels if g2 else capi.g1_lagrange_levels
    assert check(fixed(s, g2), f(fixed(s, g2), 0, hi), hi, ch)[1]
    assert check(fixed(s, g2), fixed(lv + [5, 6], g2), hi, ch)[1]
    if hi:
        assert check(fixed(s, g2), fixed(lv, g2), hi - 1, ch)[1]


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_levels_check_refuses_one_wrong_point_anywhere(g2):
    hi, n = 4, 16
    s = tau_powers(n, 720)
    lv = levels(s, 0, hi)
    check = capi.g2_lagrange_levels_check if g2 else capi.g1_lagrange_levels_check
    pw = fixed(s, g2)
    for at in (0, 5, len(lv) - 1):
        for wrong in ((lv[at] + 1) % R, 0):
            bad = list(lv)
            bad[at] = wrong
            name, ok, lhs, rhs = check(pw, fixed(bad, g2), hi, 12345)
            assert not ok and lhs != rhs
    other = list(s)
    other[n - 1] = (other[n - 1] + 1) % R               # a wrong POWER shows in the top level only
    assert not check(fixed(other, g2), fixed(lv, g2), hi, 12345)[1]
    assert check(fixed(other, g2), fixed(lv, g2), hi - 1, 12345)[1]


def test_levels_check_short_powers():
    """2^hi - 1 powers: the levels must be those of the array with a last point at infinity"""
    hi, n = 3, 8
    s = tau_powers(n, 730)
    short, full = levels(s[:n - 1] + [0], 0, hi), levels(s, 0, hi)
    assert capi.g1_lagrange_levels_check(fixed(s[:n - 1]), fixed(short), hi, 777)[1]
    assert not capi.g1_lagrange_levels_check(fixed(s[:n - 1]), fixed(full), hi, 777)[1]
    assert capi.g1_lagrange_levels_check(fixed(s), fixed(full), hi, 777)[1]


def test_levels_check_refusals():
    p1, p2 = fixed([1, 2, 3, 4]), fixed([1, 2, 3, 4], True)
    l1 = fixed(list(range(1, 8)))
    c1, c2 = capi.g1_lagrange_levels_check, capi.g2_lagrange_levels_check
    refused(GS_ERR_ARG, "gs_g1_lagrange_levels_check: bad base-array handle", c1, p2, l1, 2, 5)
    refused(GS_ERR_ARG, "gs_g2_lagrange_levels_check: bad base-array handle", c2, p2, l1, 2, 5)
    refused(GS_ERR_ARG, "the challenge is 0 mod r", c1, p1, l1, 2, 0)
    refused(GS_ERR_ARG, "the challenge is 0 mod r", c1, p1, l1, 2, R)
    refused(GS_ERR_ARG, r"hi = 26, must be 0 \.\. 25 \(a sum takes at most 2\^26 - 1 terms", c1, p1, l1, 26, 5)
    refused(GS_ERR_SHAPE, r"levels holds 7 points, the levels 0 \.\. 3 are 15", c1, p1, l1, 3, 5)
    refused(GS_ERR_SHAPE, r"powers holds 4 points, level 3 needs 8 \(or 7 and a last point at infinity\)", c1, p1, fixed(list(range(1, 16))), 3, 5)
    lib = capi.load_library()
    ch = capi.ints_to_u64([5])
    assert lib.gs_g1_lagrange_levels_check(capi.raw(p1), capi.raw(l1), 2, capi.ptr64(ch.reshape(-1)), None) == GS_ERR_ARG
    assert b"null argument" in lib.gs_last_error()
    res = capi.CheckResult()
    assert lib.gs_g1_lagrange_levels_check(capi.raw(p1), capi.raw(l1), 2, None, ctypes.byref(res)) == GS_ERR_ARG
