"""-m gpu: gs_pairing_product -- prod_i e(P_i, Q_i) over two resident arrays, a Miller loop per pair on the device.

Pairs (a_i G1, b_i G2) from gs_g1_fixed_base / gs_g2_fixed_base, so nothing large is uploaded; by bilinearity the product is
e((sum a_i b_i mod r) G1, G2), ONE host pairing (gs_pairing), and the device's value must equal it bit for bit.  The sizes put one
lane, both sides of the 64-lane workgroup seam, both sides of the seam where a second pass over the partials starts (more than 4
partials: n = 257) and two such passes (n = 16449) under the kernels."""
import ctypes
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import bn128, capi
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = O.R
SIZES = [1, 2, 3, 4, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 16449]
ONE = [1] + [0] * 47


@pytest.fixture(autouse=True)
def _init():
    capi.init()


_host = {}


def host_pairing_of_multiple(k):
    """gs_pairing(k G1, G2) as 48 words, one host pairing per distinct k."""
    k %= R
    if k not in _host:
        out = np.zeros(48, dtype=np.uint64)
        a = capi.g1_points_to_u64([O.G1.MulScalar(O.G1_GEN, k) if k else O.G1_ZERO])
        b = capi.g2_points_to_u64([O.G2_GEN])
        capi.call("gs_pairing", capi.ptr64(a), capi.ptr64(b), capi.ptr64(out))
        _host[k] = [int(x) for x in out]
    return _host[k]


def arrays(a, b):
    return capi.g1_fixed_base(capi.ints_to_u64(a)), capi.g2_fixed_base(capi.ints_to_u64(b))


def product(a, b):
    g1, g2 = arrays(a, b)
    out, one = capi.pairing_product(g1, 0, g2, 0, len(a))
    return [int(x) for x in out], one


def scalars(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, 1 << 64) for _ in range(n)], [rng.randrange(1, 1 << 64) for _ in range(n)]


def test_the_generators_give_the_host_pairing_bit_for_bit():
    got, one = product([1], [1])
    assert got == host_pairing_of_multiple(1) and not one and got != ONE


@pytest.mark.parametrize("n", SIZES)
def test_product_equals_one_host_pairing_of_the_combined_scalar(n):
    a, b = scalars(n, 100 + n)
    got, one = product(a, b)
    assert got == host_pairing_of_multiple(sum(x * y for x, y in zip(a, b))), n
    assert not one


@pytest.mark.parametrize("n", [2, 65, 129, 257, 1000])
def test_a_vanishing_sum_gives_one_and_off_by_one_does_not(n):
    a, b = scalars(n, 200 + n)
    rest = sum(x * y for x, y in zip(a[:-1], b[:-1])) % R
    a[-1] = (-rest * pow(b[-1], R - 2, R)) % R
    got, one = product(a, b)
    assert one and got == ONE, n
    a[-1] = (a[-1] + 1) % R
    got, one = product(a, b)
    assert not one and got == host_pairing_of_multiple(b[-1]), n


def test_a_point_and_its_negative_against_the_same_q():
    rng = random.Random(5)
    k, m = rng.randrange(1, R), rng.randrange(1, R)
    assert product([k, R - k], [m, m]) == (ONE, True)
    assert product([R - 1, 1, 7], [m, m, 1]) == (host_pairing_of_multiple(7), False)


def test_infinite_members_contribute_one():
    a, b = scalars(70, 6)
    want = lambda keep: host_pairing_of_multiple(sum(a[i] * b[i] for i in keep))   # noqa: E731
    alive = set(range(70))
    pa, pb = list(a), list(b)
    for i in (0, 5, 63, 64):
        pa[i] = 0                                                       # infinite P only
    for i in (1, 6, 62, 69):
        pb[i] = 0                                                       # infinite Q only
    for i in (2, 65):
        pa[i] = pb[i] = 0                                               # both
    alive -= {0, 5, 63, 64, 1, 6, 62, 69, 2, 65}
    assert product(pa, pb) == (want(alive), False)
    assert product([0] * 70, b) == (ONE, True)
    assert product(a, [0] * 70) == (ONE, True)
    assert product([0] * 3, [0] * 3) == (ONE, True)
    assert product([0, 9], [4, 0]) == (ONE, True)


def test_a_q_outside_the_subgroup_still_returns():
    """The precondition is the caller's; the value means nothing, but the call runs the same instructions and returns, and the pairs
    in other calls are not disturbed."""
    import membership_util as M
    twist = M.twist_points(2)
    assert not any(M.in_subgroup(t) for t in twist)
    g2 = capi.g2_upload(capi.g2_points_to_u64(twist + [O.G2_GEN]))
    g1 = capi.g1_fixed_base(capi.ints_to_u64([3, 4, 5]))
    assert capi.g2_subgroup_check(g2) == (2, 0)
    out, one = capi.pairing_product(g1, 0, g2, 0, 2)
    assert len(out) == 48
    out, one = capi.pairing_product(g1, 2, g2, 2, 1)
    assert [int(x) for x in out] == host_pairing_of_multiple(5) and not one


def test_offsets_windows_and_the_empty_product():
    a, b = scalars(150, 7)
    g1, g2 = arrays(a, b)
    for poff, qoff, n in ((0, 0, 150), (3, 3, 64), (10, 70, 65), (149, 0, 1), (0, 149, 1), (86, 21, 64)):
        out, one = capi.pairing_product(g1, poff, g2, qoff, n)
        assert [int(x) for x in out] == host_pairing_of_multiple(sum(a[poff + i] * b[qoff + i] for i in range(n))), (poff, qoff, n)
    for poff, qoff in ((0, 0), (150, 150), (7, 150)):
        out, one = capi.pairing_product(g1, poff, g2, qoff, 0)
        assert [int(x) for x in out] == ONE and one
    value, one = bn128.PairingProduct(g1, g2, 148, 100)                 # as many pairs as both arrays hold: 2
    want = capi.u64_to_ints(np.array(host_pairing_of_multiple(a[148] * b[100] + a[149] * b[101]), dtype=np.uint64))
    assert not one and [c for half in value for pair in half for c in pair] == want
    lib = capi.load_library()
    flag, words = ctypes.c_int(7), np.zeros(48, dtype=np.uint64)
    assert lib.gs_pairing_product(capi.raw(g1), 0, capi.raw(g2), 0, 2, None, ctypes.byref(flag)) == 0 and flag.value == 0
    assert lib.gs_pairing_product(capi.raw(g1), 0, capi.raw(g2), 0, 2, capi.ptr64(words), None) == 0
    assert [int(x) for x in words] == host_pairing_of_multiple(a[0] * b[0] + a[1] * b[1])
    assert capi.last_timing()["total_ms"] > 0.0


def test_errors_and_balanced_allocations():
    a, b = scalars(65, 8)
    g1, g2 = arrays(a, b)
    sc = capi.scalars_upload(capi.ints_to_u64([1, 2, 3]))
    capi.pairing_product(g1, 0, g2, 0, 65)
    before = capi.alloc_counters()
    lib = capi.load_library()
    flag, words = ctypes.c_int(7), np.full(48, 7, dtype=np.uint64)
    out = (capi.ptr64(words), ctypes.byref(flag))
    h1, h2 = capi.raw(g1), capi.raw(g2)
    for args, code in (((h1, 1, h2, 0, 65) + out, -4), ((h1, 0, h2, 1, 65) + out, -4), ((h1, 66, h2, 0, 0) + out, -4), ((h1, 0, h2, 66, 0) + out, -4),
                       ((h1, 0, h2, 0, 66) + out, -4), ((h1, 0, h2, 0, (1 << 64) - 1) + out, -4),
                       ((h2, 0, h2, 0, 1) + out, -3), ((h1, 0, h1, 0, 1) + out, -3), ((h2, 0, h1, 0, 1) + out, -3), ((capi.raw(sc), 0, h2, 0, 1) + out, -3),
                       ((h1, 0, capi.raw(sc), 0, 1) + out, -3), ((0, 0, h2, 0, 1) + out, -3), ((h1, 0, 0, 0, 1) + out, -3),
                       ((h1, 0, h2, 0, 1, None, None), -3)):
        assert lib.gs_pairing_product(*args) == code, args
        assert b"gs_pairing_product" in lib.gs_last_error()
    assert flag.value == 7 and (words == 7).all()
    for n in (0, 1, 64, 65):
        capi.pairing_product(g1, 0, g2, 0, n)
    after = capi.alloc_counters()
    assert after[0] - before[0] == after[1] - before[1]                 # every workspace of a call is gone when it returns
    assert capi.handle_bytes(g1)[1] == 0 and capi.handle_bytes(g2)[1] == 0      # and no window table was built
