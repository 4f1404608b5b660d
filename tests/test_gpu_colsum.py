"""-m gpu: gs_r1cs_colsum_g1 / _g2 -- out[s] = sum_j a_js Ba[j] + b_js Bb[j] + c_js Bc[j], the column sums of a resident R1CS over points.

The basis points are known multiples of the generator (gs_g*_fixed_base; 0 = infinity, equal and opposite scalars = equal and opposite
points), so the expected sum of a column is computed on the scalars in Python integers and multiplied onto the generator; every comparison
is bit for bit on the downloaded affine points."""
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom, r1csqap
import circom_util as CU

pytestmark = pytest.mark.gpu
R = CU.R
GS_ERR_ARG, GS_ERR_SHAPE = -3, -4
FULL = 0x2f3a9c0b5d7e1f4a6b8c9d0e1f2a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c % R
COEFS = [1, R - 1, 2, R - 2, 65535, R - 65535, 1 << 128, FULL, R + 1, (1 << 256) - 1]


@pytest.fixture(autouse=True)
def _init():
    capi.init()


def fixed(scalars, g2=False):
    return (capi.g2_fixed_base if g2 else capi.g1_fixed_base)(CU.u64(scalars))


def rows_of(handle, g2=False):
    return (capi.g2_download if g2 else capi.g1_download)(handle)


def assert_points(handle, scalars, g2=False):
    assert len(handle) == len(scalars)
    assert np.array_equal(rows_of(handle, g2), rows_of(fixed(scalars, g2), g2))


def csr(rows):
    """rows: one list of (column, value) per row, as they come (unsorted, repeats allowed, any value below 2^256)"""
    rp = np.zeros(len(rows) + 1, dtype=np.uint32)
    rp[1:] = np.cumsum([len(r) for r in rows])
    terms = [t for r in rows for t in r]
    col = np.array([c for c, _ in terms], dtype=np.uint32)
    val = capi.ints_to_u64([v for _, v in terms]) if terms else np.zeros((0, 4), dtype=np.uint64)
    return rp, col, val


class System:
    """n rows x nvars columns, three matrices.  Column 0 sits in every row of A; columns nvars - 3 .. nvars - 1 stay empty; column 1 of A
    cancels to infinity (v P and (r - v) P in one row, 1 P and (r - 1) P in another); column 2 of B has one term; (row 0, column 3) of C is
    repeated.  Coefficients are drawn from COEFS."""

    def __init__(self, n, nvars, seed, fan=2):
        rng = random.Random(seed)
        self.n, self.nvars = n, nvars
        free = list(range(4, nvars - 3))
        self.mats = []
        for k in range(3):
            rows = []
            for j in range(n):
                row = [(rng.choice(free), rng.choice(COEFS)) for _ in range(fan)] if free else []
                if k == 0:
                    row.append((0, COEFS[j % len(COEFS)]))
                rng.shuffle(row)
                rows.append(row)
            self.mats.append(rows)
        a, b, c = self.mats
        a[0] += [(1, FULL), (1, R - FULL)]
        a[n - 1] += [(1, 1), (1, R - 1)]
        b[n // 2].append((2, 65535))
        c[0] += [(3, 7), (3, R - 2), (3, 7)]

    def expected(self, bases):
        """bases: three scalar lists or None"""
        out = [0] * self.nvars
        for rows, basis in zip(self.mats, bases):
            if basis is None:
                continue
            for j, row in enumerate(rows):
                for s, v in row:
                    out[s] = (out[s] + v * basis[j]) % R
        return out

    def upload(self, k=None):
        a, b, c = (csr(rows) for rows in self.mats)
        return circom.DeviceDomainR1CS(k, a, b, c, self.nvars) if k else r1csqap.DeviceR1CS(a, b, c, self.nvars)


def basis_scalars(count, seed):
    """random multiples with infinities, an equal pair and an opposite pair"""
    rng = random.Random(seed)
    s = [rng.randrange(1, R) for _ in range(count)]
    s[count // 3] = 0
    if count >= 2:
        s[1] = s[0]
        s[count - 1] = (R - s[count - 2]) % R
    if count >= 8:
        s[5] = 0
    return s


SHAPES = [(1, 2, 9), (3, 8, 13), (3, 6, 77), (10, 1024, 1024 + 37), (None, 5, 11)]       # (log2 domain or nodes, rows, nvars)


@pytest.mark.parametrize("k,n,nvars", SHAPES)
def test_colsum_g1(k, n, nvars):
    system = System(n, nvars, 100 + n)
    dev = system.upload(k)
    points = (1 << k) if k else n
    scal = [basis_scalars(points + extra, 7 * n + extra) for extra in (0, 1, 3)]              # a basis may be longer than the rows
    bases = [fixed(s) for s in scal]
    ex = system.expected(scal)
    assert ex[1] == 0 and not any(ex[nvars - 3:])                                            # the cancelling and the empty columns
    assert_points(capi.r1cs_colsum(dev, *bases), ex)
    for which in range(3):                                                                   # each matrix alone
        only = [b if i == which else None for i, b in enumerate(bases)]
        assert_points(capi.r1cs_colsum(dev, *only), system.expected([s if i == which else None for i, s in enumerate(scal)]))
    assert_points(capi.r1cs_colsum(dev, bases[0], bases[0], None), system.expected([scal[0], scal[0], None]))
    assert_points(capi.r1cs_colsum(dev, None, None, None), [0] * nvars)


@pytest.mark.parametrize("k,n,nvars", [s for s in SHAPES if s[0] in (1, 3)])
def test_colsum_g2(k, n, nvars):
    system = System(n, nvars, 200 + n)
    dev = system.upload(k)
    scal = [basis_scalars(1 << k, 11 * n + i) for i in range(3)]
    bases = [fixed(s, True) for s in scal]
    assert_points(capi.r1cs_colsum(dev, *bases, g2=True), system.expected(scal), True)
    for which in range(3):
        only = [b if i == which else None for i, b in enumerate(bases)]
        assert_points(capi.r1cs_colsum(dev, *only, g2=True), system.expected([s if i == which else None for i, s in enumerate(scal)]), True)


def test_heavy_column_of_units_and_of_general_terms():
    """One column in every row of a 2^10 domain, once with +-1 coefficients only and once with full-width ones: 1024 terms of one class,
    several chunks and levels deep; every other column is empty."""
    k, n, nvars = 10, 1024, 70
    scal = basis_scalars(n, 5)
    basis = fixed(scal)
    for coefs in ([1, R - 1, 1], [FULL, R - 2, 3, (1 << 200) + 5]):
        rows = [[(69, coefs[j % len(coefs)])] for j in range(n)]
        empty = [[] for _ in range(n)]
        dev = circom.DeviceDomainR1CS(k, csr(empty), csr(rows), csr(empty), nvars)
        want = [0] * nvars
        want[69] = sum(coefs[j % len(coefs)] * scal[j] for j in range(n)) % R
        assert_points(capi.r1cs_colsum(dev, None, basis, None), want)


def test_product_system_and_refusals():
    k, n, nvars = 3, 8, 13
    system = System(n, nvars, 300)
    rows_a, rows_b = ([dict((s, v % R) for s, v in row if s >= 4) for row in rows] for rows in system.mats[:2])
    rec = np.frombuffer(b"".join(circom.CoefRecords(rows_a, rows_b)), dtype=np.uint8)
    prod = circom.DeviceZkeyR1CS(k, nvars, rec)
    scal = [basis_scalars(n, 31), basis_scalars(n, 32)]
    b1, b2 = fixed(scal[0]), fixed(scal[1])
    want = [0] * nvars
    for rows, basis in zip((rows_a, rows_b), scal):
        for j, row in enumerate(rows):
            for s, v in row.items():
                want[s] = (want[s] + v * basis[j]) % R
    assert_points(capi.r1cs_colsum(prod, b1, b2, None), want)

    def refused(code, what, *args, **kw):
        with pytest.raises(capi.GosnarkHipError, match=what) as e:
            capi.r1cs_colsum(*args, **kw)
        assert e.value.code == code

    refused(GS_ERR_SHAPE, "product system", prod, b1, b2, b1)
    dev = system.upload(k)
    short = fixed(scal[0][:n - 1])
    refused(GS_ERR_SHAPE, "the basis of matrix B has 7 points, the system 8 rows", dev, b1, short, None)
    refused(GS_ERR_SHAPE, "the basis of matrix C has 7 points", dev, None, None, short)
    refused(GS_ERR_ARG, "bad base-array handle for matrix A", dev, fixed(scal[0], True), None, None)
    refused(GS_ERR_ARG, "bad base-array handle for matrix B", dev, None, b1, None, g2=True)
    refused(GS_ERR_ARG, "bad R1CS handle", b1, b1, None, None)
