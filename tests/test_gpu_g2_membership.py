"""-m gpu: gs_g2_subgroup_check -- which points of a resident G2 array lie outside the order-r subgroup?

Arrays of multiples of the generator (repeated addition, oracle/ref_py) with points of three bad kinds planted in them: a random twist
point, a point S of order 10069 (the smallest prime factor of the twist's cofactor) and G + S for the subgroup point G it replaces.  The
sizes put one wave, both sides of the 64-thread workgroup seam and a tail under the kernel."""
import ctypes

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi
import membership_util as M
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
NMAX = 200
SIZES = [1, 63, 64, 65, 129, 200]


@pytest.fixture(autouse=True)
def _init():
    capi.init()


@pytest.fixture(scope="module")
def good():
    """(the points, their upload words): 3 G2, 4 G2, ..."""
    pts = M.subgroup_multiples(NMAX, first=3)
    return pts, capi.g2_points_to_u64(pts)


@pytest.fixture(scope="module")
def bad_kinds():
    """name -> f(the subgroup point it replaces) -> a point outside the subgroup"""
    twist, s = M.twist_points(1)[0], M.small_order_point()
    return {"twist": lambda g: twist, "S": lambda g: s, "G+S": lambda g: M.complete_add(g, s)}


def upload(good, n, planted=()):
    """The first n good points with planted = [(index, point)] written over them."""
    words = good[1][:n].copy()
    for i, p in planted:
        words[i] = capi.g2_points_to_u64([p])[0]
    return capi.g2_upload(words)


@pytest.mark.parametrize("n", SIZES)
def test_subgroup_points_and_infinities_are_members(good, n):
    assert capi.g2_subgroup_check(upload(good, n)) == (0, None)
    third = [(i, O.G2_ZERO) for i in range(0, n, 3)]
    assert capi.g2_subgroup_check(upload(good, n, third)) == (0, None)
    assert capi.g2_subgroup_check(upload(good, n, [(i, O.G2_ZERO) for i in range(n)])) == (0, None)


@pytest.mark.parametrize("kind", ["twist", "S", "G+S"])
def test_one_planted_point_is_counted_and_located(good, bad_kinds, kind):
    n = 129
    for i in (0, 63, 64, n - 1, 37):
        h = upload(good, n, [(i, bad_kinds[kind](good[0][i]))])
        assert capi.g2_subgroup_check(h) == (1, i), (kind, i)


def test_several_planted_points_windows_and_the_oracles_verdict_per_index(good, bad_kinds):
    n = 129
    planted = [(5, bad_kinds["twist"](None)), (64, bad_kinds["S"](None)), (128, bad_kinds["G+S"](good[0][128]))]
    h = upload(good, n, planted)
    assert capi.g2_subgroup_check(h) == (3, 5)
    assert capi.g2_subgroup_check(h, 6, 58) == (0, None)
    assert capi.g2_subgroup_check(h, 6, 59) == (1, 64)
    assert capi.g2_subgroup_check(h, 6) == (2, 64)
    assert capi.g2_subgroup_check(h, 65, 0) == (0, None)
    assert capi.g2_subgroup_check(h, n, 0) == (0, None)
    pts = list(good[0][:n])
    for i, p in planted:
        pts[i] = p
    for i in (0, 1, 4, 5, 6, 31, 62, 63, 64, 65, 66, 100, 126, 127, 128, 77):
        want = M.in_subgroup(pts[i])
        assert want == (i not in (5, 64, 128))
        assert capi.g2_subgroup_check(h, i, 1) == ((0, None) if want else (1, i)), i


def test_errors_leave_the_array_usable(good):
    n = 65
    h = upload(good, n)
    g1 = capi.g1_fixed_base(capi.ints_to_u64([1, 2, 3]))
    sc = capi.scalars_upload(capi.ints_to_u64([1, 2, 3]))
    lib = capi.load_library()
    nbad, first = ctypes.c_uint64(0), ctypes.c_uint64(0)
    for args, code in (((capi.raw(g1), 0, 1, ctypes.byref(nbad), ctypes.byref(first)), -3), ((capi.raw(sc), 0, 1, ctypes.byref(nbad), ctypes.byref(first)), -3),
                       ((0, 0, 1, ctypes.byref(nbad), ctypes.byref(first)), -3),
                       ((capi.raw(h), 0, n, None, ctypes.byref(first)), -3), ((capi.raw(h), 0, n, ctypes.byref(nbad), None), -3),
                       ((capi.raw(h), 1, n, ctypes.byref(nbad), ctypes.byref(first)), -4), ((capi.raw(h), n + 1, 0, ctypes.byref(nbad), ctypes.byref(first)), -4),
                       ((capi.raw(h), 0, n + 1, ctypes.byref(nbad), ctypes.byref(first)), -4)):
        assert lib.gs_g2_subgroup_check(*args) == code, args
        assert b"gs_g2_subgroup_check" in lib.gs_last_error()
    with pytest.raises(capi.GosnarkHipError) as e:
        capi.g2_subgroup_check(h, 1, n)
    assert e.value.code == -4
    assert capi.g2_subgroup_check(h) == (0, None)
    assert capi.handle_bytes(h)[1] == 0                      # no window table was built
    assert np.array_equal(capi.g2_download(h), capi.g2_download(upload(good, n)))
    assert capi.last_timing()["total_ms"] >= 0.0
