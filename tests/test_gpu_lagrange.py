"""-m gpu: gs_g1_lagrange / gs_g2_lagrange -- the inverse transform of a point sequence carried out in the group.

Every input point is a known multiple of the generator (gs_g*_fixed_base: infinity = 0, equal points = equal scalars, opposite points =
negated scalars), so the expected output is the O(n^2) definition evaluated on the SCALARS in Python integers, times the generator;
the comparison is bit for bit on the downloaded affine points."""
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi
import circom_util as CU

pytestmark = pytest.mark.gpu
R = CU.R
GS_ERR_ARG, GS_ERR_SHAPE = -3, -4
LOGS = [1, 2, 7, 8]          # one butterfly; two stages; exactly one 64-thread block of butterflies; two blocks


@pytest.fixture(autouse=True)
def _init():
    capi.init()


def fixed(scalars, g2=False):
    return (capi.g2_fixed_base if g2 else capi.g1_fixed_base)(CU.u64(scalars))


def rows(handle, g2=False):
    return (capi.g2_download if g2 else capi.g1_download)(handle)


def assert_points(handle, scalars, g2=False):
    """handle's points == scalars * generator, bit for bit (both through the same download of canonical affine points)"""
    assert len(handle) == len(scalars)
    assert np.array_equal(rows(handle, g2), rows(fixed(scalars, g2), g2))


def transform(s, k):
    """out[j] = (1/n) sum_{i<n} w^(-ij) s_i"""
    n = 1 << k
    wi = pow(CU.omega(k), -1, R)
    pw = [pow(wi, e, R) for e in range(n)]
    ninv = pow(n, -1, R)
    return [sum(s[i] * pw[i * j % n] for i in range(n)) * ninv % R for j in range(n)]


def odd_half(s, k):
    """out[j] = (1/2n) sum_{i<2n} v^(-(2j+1)i) s_i, v = 5^((r-1)/(2n)); a missing s[2n-1] is 0"""
    n = 1 << k
    s = list(s) + [0] * (2 * n - len(s))
    vi = pow(CU.omega(k + 1), -1, R)
    pw = [pow(vi, e, R) for e in range(2 * n)]
    inv = pow(2 * n, -1, R)
    return [sum(s[i] * pw[(2 * j + 1) * i % (2 * n)] for i in range(2 * n)) * inv % R for j in range(n)]


def tau_powers(count, seed):
    tau = random.Random(seed).randrange(2, R)
    out = [1]
    for _ in range(count - 1):
        out.append(out[-1] * tau % R)
    return out


def planted(count, n, seed):
    """random multiples with infinities, equal pairs and opposite pairs at the partners of a butterfly: i / i + n/2 (the last stage),
    i / i + 1 (the first), and i / i + n (the difference the odd half starts with)"""
    rng = random.Random(seed)
    s = [rng.randrange(1, R) for _ in range(count)]
    spans = [d for d in (1, n // 2, n) if 0 < d < count]
    at = 0
    for d in spans:
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


@pytest.mark.parametrize("k", LOGS)
def test_g1_lagrange(k):
    n = 1 << k
    for s in (tau_powers(n, 10 + k), planted(n, n, 20 + k)):
        assert_points(capi.g1_lagrange(fixed(s), k), transform(s, k))


@pytest.mark.parametrize("k", LOGS)
def test_g2_lagrange(k):
    n = 1 << k
    for s in (tau_powers(n, 30 + k), planted(n, n, 40 + k)):
        assert_points(capi.g2_lagrange(fixed(s, True), k), transform(s, k), True)


@pytest.mark.parametrize("k", LOGS)
def test_g1_lagrange_odd_half_with_and_without_the_last_point(k):
    n = 1 << k
    for s in (tau_powers(2 * n, 50 + k), planted(2 * n, n, 60 + k)):
        if s[2 * n - 1] == 0:
            s[2 * n - 1] = 12345
        short = capi.g1_lagrange(fixed(s[:2 * n - 1]), k, odd_half=True)
        full = capi.g1_lagrange(fixed(s), k, odd_half=True)
        assert_points(short, odd_half(s[:2 * n - 1], k))
        assert_points(full, odd_half(s, k))
        # the two differ by the last point's term alone: (1/2n) v^(-(2j+1)(2n-1)) s[2n-1] = (1/2n) v^(2j+1) s[2n-1]
        v, inv = CU.omega(k + 1), pow(2 * n, -1, R)
        a, b = odd_half(s[:2 * n - 1], k), odd_half(s, k)
        assert all((b[j] - a[j]) % R == inv * pow(v, 2 * j + 1, R) % R * s[2 * n - 1] % R for j in range(n))
        assert not np.array_equal(rows(short), rows(full))


def test_size_one_is_the_identity():
    s = [random.Random(70).randrange(1, R), 0]
    for g2 in (False, True):
        pts = fixed(s, g2)
        for off in (0, 1):
            out = capi.g2_lagrange(pts, 0, off=off) if g2 else capi.g1_lagrange(pts, 0, off=off)
            assert_points(out, [s[off]], g2)


def test_offsets_and_longer_arrays():
    """The transform reads n (2n - 1, 2n) points from `off` of an array that holds more: what lies before and behind does not count."""
    k, n, off = 3, 8, 5
    s = planted(off + 2 * n + 4, n, 80)
    p1, p2 = fixed(s), fixed(s, True)
    assert_points(capi.g1_lagrange(p1, k, off=off), transform(s[off:off + n], k))
    assert_points(capi.g2_lagrange(p2, k, off=off), transform(s[off:off + n], k), True)
    assert_points(capi.g1_lagrange(p1, k, off=off, odd_half=True), odd_half(s[off:off + 2 * n], k))
    tail = fixed(s[:off + 2 * n - 1])
    assert_points(capi.g1_lagrange(tail, k, off=off, odd_half=True), odd_half(s[off:off + 2 * n - 1], k))


def test_refusals():
    p1, p2 = fixed([1, 2, 3, 4]), fixed([1, 2, 3, 4], True)

    def refused(code, what, fn, *args, **kw):
        with pytest.raises(capi.GosnarkHipError, match=what) as e:
            fn(*args, **kw)
        assert e.value.code == code

    refused(GS_ERR_ARG, "bad base-array handle", capi.g1_lagrange, p2, 1)
    refused(GS_ERR_ARG, "bad base-array handle", capi.g2_lagrange, p1, 1)
    refused(GS_ERR_ARG, "bad base-array handle", capi.g1_lagrange, 987654321, 1)
    refused(GS_ERR_ARG, "log2_n = 28, must be 0 .. 27", capi.g1_lagrange, p1, 28)
    refused(GS_ERR_ARG, "log2_n = 28, must be 0 .. 27", capi.g2_lagrange, p2, 28)
    refused(GS_ERR_ARG, "log2_n = 0, must be 1 .. 27", capi.g1_lagrange, p1, 0, odd_half=True)
    refused(GS_ERR_ARG, "log2_n = 28, must be 1 .. 27", capi.g1_lagrange, p1, 28, odd_half=True)
    refused(GS_ERR_SHAPE, "the array has 4 points, the transform needs 8 from index 0", capi.g1_lagrange, p1, 3)
    refused(GS_ERR_SHAPE, "the array has 4 points, the transform needs 4 from index 1", capi.g1_lagrange, p1, 2, off=1)
    refused(GS_ERR_SHAPE, "the array has 4 points, the transform needs 7 from index 0", capi.g1_lagrange, p1, 2, odd_half=True)
    refused(GS_ERR_SHAPE, "the array has 4 points, the transform needs 4 from index 9", capi.g2_lagrange, p2, 2, off=9)
    assert len(capi.g1_lagrange(p1, 1, off=1, odd_half=True)) == 2          # 3 = 2n - 1 points from index 1: accepted
