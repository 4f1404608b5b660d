"""-m gpu: gs_pairing_each -- e(P_i, Q_i) for every i over two resident arrays, Miller loop AND final exponentiation on the device.

Pairs (a_i G1, b_i G2) from gs_g1_fixed_base / gs_g2_fixed_base.  Every value must equal the host's gs_pairing of the same pair word
for word.  The sizes are one lane, two, and both sides of the one-wave workgroup seam with one and two full workgroups in front."""
import ctypes
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import bn128, capi
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
Q, R = O.Q, O.R
SIZES = [1, 2, 65, 130]
ONE = [1] + [0] * 47


@pytest.fixture(autouse=True)
def _init():
    capi.init()


def scalars(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(n)], [rng.randrange(1, R) for _ in range(n)]


def arrays(a, b):
    return capi.g1_fixed_base(capi.ints_to_u64(a)), capi.g2_fixed_base(capi.ints_to_u64(b))


def host_pairings(g1, g2, poff, qoff, n):
    """gs_pairing of pair i, read back from the resident arrays: n x 48 words."""
    p, q = capi.g1_download(g1), capi.g2_download(g2)
    out = np.zeros((n, 48), dtype=np.uint64)
    for i in range(n):
        capi.call("gs_pairing", capi.ptr64(np.ascontiguousarray(p[poff + i])), capi.ptr64(np.ascontiguousarray(q[qoff + i])), capi.ptr64(out[i]))
    return out


# Fq12 product on the 12 coordinates of gs_pairing's encoding: (a0.c0, a0.c1, a0.c2, a1.c0, a1.c1, a1.c2), each an (c0, c1) of Fq2
def _f2mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def _f2add(a, b):
    return ((a[0] + b[0]) % Q, (a[1] + b[1]) % Q)


def _xi(a):
    return _f2mul(a, (9, 1))


def _f6mul(a, b):
    z = (0, 0)
    c = [z] * 5
    for i in range(3):
        for j in range(3):
            c[i + j] = _f2add(c[i + j], _f2mul(a[i], b[j]))
    return [_f2add(c[0], _xi(c[3])), _f2add(c[1], _xi(c[4])), c[2]]


def f12_mul(x, y):
    a = [[(x[6 * h + 2 * i], x[6 * h + 2 * i + 1]) for i in range(3)] for h in range(2)]
    b = [[(y[6 * h + 2 * i], y[6 * h + 2 * i + 1]) for i in range(3)] for h in range(2)]
    t0, t1 = _f6mul(a[0], b[0]), _f6mul(a[1], b[1])
    vt1 = [_xi(t1[2]), t1[0], t1[1]]                                    # v (c0 + c1 v + c2 v^2)
    c0 = [_f2add(t0[i], vt1[i]) for i in range(3)]
    m0, m1 = _f6mul(a[0], b[1]), _f6mul(a[1], b[0])
    c1 = [_f2add(m0[i], m1[i]) for i in range(3)]
    return [c for half in (c0, c1) for pair in half for c in pair]


@pytest.mark.parametrize("n", SIZES)
def test_every_value_equals_the_host_pairing_and_the_product_the_device_product(n):
    a, b = scalars(n, 300 + n)
    g1, g2 = arrays(a, b)
    got, one = capi.pairing_each(g1, 0, g2, 0, n)
    want = host_pairings(g1, g2, 0, 0, n)
    assert got.shape == (n, 48) and (got == want).all(), [i for i in range(n) if (got[i] != want[i]).any()]
    assert not one.any()
    prod = [1] + [0] * 11
    for row in got:
        prod = f12_mul(prod, capi.u64_to_ints(row))
    whole, _ = capi.pairing_product(g1, 0, g2, 0, n)
    assert prod == capi.u64_to_ints(whole)


def test_infinite_members_give_one_in_their_lane_only():
    n = 130
    a, b = scalars(n, 17)
    for i in (0, 63, 64, 129):
        a[i] = 0                                                        # infinite P
    for i in (1, 62, 65, 128):
        b[i] = 0                                                        # infinite Q
    a[2] = b[2] = a[66] = b[66] = 0                                     # both
    dead = {0, 63, 64, 129, 1, 62, 65, 128, 2, 66}
    g1, g2 = arrays(a, b)
    got, one = capi.pairing_each(g1, 0, g2, 0, n)
    want = host_pairings(g1, g2, 0, 0, n)
    assert (got == want).all()
    for i in range(n):
        assert bool(one[i]) == (i in dead), i
        assert ([int(x) for x in got[i]] == ONE) == (i in dead), i


def test_inverse_pairs_and_ones_are_flagged():
    # e(kG1, mG2) e(-kG1, mG2) = 1, and e(kG1, rG2) cannot be built; e(P, Q)^r = 1 is implicit.  Here: value i times value i + 1 is one.
    rng = random.Random(18)
    k, m = rng.randrange(1, R), rng.randrange(1, R)
    g1, g2 = arrays([k, R - k], [m, m])
    got, one = capi.pairing_each(g1, 0, g2, 0, 2)
    assert not one.any()
    assert f12_mul(capi.u64_to_ints(got[0]), capi.u64_to_ints(got[1])) == [1] + [0] * 11


def test_offsets_null_outputs_and_the_python_wrapper():
    a, b = scalars(150, 19)
    g1, g2 = arrays(a, b)
    for poff, qoff, n in ((3, 3, 64), (10, 70, 65), (149, 0, 1), (0, 149, 1), (20, 0, 130)):
        got, one = capi.pairing_each(g1, poff, g2, qoff, n)
        assert (got == host_pairings(g1, g2, poff, qoff, n)).all(), (poff, qoff, n)
    assert capi.last_timing()["total_ms"] > 0.0
    vals, ones = bn128.PairingEach(g1, g2, 148, 100)                     # as many pairs as both arrays hold: 2
    want = host_pairings(g1, g2, 148, 100, 2)
    assert ones == [False, False] and len(vals) == 2
    for v, w in zip(vals, want):
        assert [c for half in v for pair in half for c in pair] == capi.u64_to_ints(w)
    assert vals[0] == bn128.Pairing(O.G1.MulScalar(O.G1_GEN, a[148]), O.G2.MulScalar(O.G2_GEN, b[100]))
    lib = capi.load_library()
    flags, words = np.full(2, 7, dtype=np.intc), np.zeros((2, 48), dtype=np.uint64)
    assert lib.gs_pairing_each(capi.raw(g1), 0, capi.raw(g2), 0, 2, None, flags.ctypes.data_as(capi.intp)) == 0 and (flags == 0).all()
    assert lib.gs_pairing_each(capi.raw(g1), 0, capi.raw(g2), 0, 2, capi.ptr64(words), None) == 0
    assert (words == host_pairings(g1, g2, 0, 0, 2)).all()
    got, one = capi.pairing_each(g1, 0, g2, 0, 0)
    assert got.shape == (0, 48) and len(one) == 0


def test_errors_and_balanced_allocations():
    a, b = scalars(65, 20)
    g1, g2 = arrays(a, b)
    sc = capi.scalars_upload(capi.ints_to_u64([1, 2, 3]))
    capi.pairing_each(g1, 0, g2, 0, 65)
    before = capi.alloc_counters()
    lib = capi.load_library()
    flags, words = np.full(66, 7, dtype=np.intc), np.full((66, 48), 7, dtype=np.uint64)
    out = (capi.ptr64(words), flags.ctypes.data_as(capi.intp))
    h1, h2 = capi.raw(g1), capi.raw(g2)
    for args, code in (((h1, 1, h2, 0, 65) + out, -4), ((h1, 0, h2, 1, 65) + out, -4), ((h1, 66, h2, 0, 0) + out, -4), ((h1, 0, h2, 66, 0) + out, -4),
                       ((h1, 0, h2, 0, 66) + out, -4), ((h1, 0, h2, 0, (1 << 64) - 1) + out, -4),
                       ((h2, 0, h2, 0, 1) + out, -3), ((h1, 0, h1, 0, 1) + out, -3), ((capi.raw(sc), 0, h2, 0, 1) + out, -3),
                       ((h1, 0, capi.raw(sc), 0, 1) + out, -3), ((0, 0, h2, 0, 1) + out, -3), ((h1, 0, 0, 0, 1) + out, -3),
                       ((h1, 0, h2, 0, 1, None, None), -3)):
        assert lib.gs_pairing_each(*args) == code, args
        assert b"gs_pairing_each" in lib.gs_last_error()
    assert (flags == 7).all() and (words == 7).all()
    for n in (0, 1, 64, 65):
        capi.pairing_each(g1, 0, g2, 0, n)
    after = capi.alloc_counters()
    assert after[0] - before[0] == after[1] - before[1]                 # every workspace of a call is gone when it returns
