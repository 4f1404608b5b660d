"""-m gpu: gs_g1_decompress / gs_g2_decompress / gs_g1_compress / gs_g2_compress against Python integers (point_codec_util).

Arrays of multiples of the generators (oracle/ref_py) with every third point negated and every fifth replaced by infinity -- for G2 also
twist points outside the subgroup -- at sizes that put one wave, both sides of the 64-thread workgroup seam and a tail under the kernels;
hand-built x coordinates with and without a root, out of range, and every inconsistent flag."""
import ctypes
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi
import membership_util as M
import point_codec_util as P
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
Q = O.Q
NMAX = 200
SIZES = [1, 63, 64, 65, 129, 200]
LARGEST, INF = capi.POINT_LARGEST_Y, capi.POINT_INFINITY
NONE = (1 << 64) - 1


@pytest.fixture(autouse=True)
def _init():
    capi.init()


class Group:
    """One of the two groups: its oracle, word widths and the functions of point_codec_util."""

    def __init__(self, g2):
        self.g2 = g2
        self.G = O.G2 if g2 else O.G1
        self.zero = O.G2_ZERO if g2 else O.G1_ZERO
        self.cw, self.jw = (8, 24) if g2 else (4, 12)
        self.to_u64 = capi.g2_points_to_u64 if g2 else capi.g1_points_to_u64
        self.upload = capi.g2_upload if g2 else capi.g1_upload
        self.download = capi.g2_download if g2 else capi.g1_download
        self.compress = capi.g2_compress if g2 else capi.g1_compress
        self.decompress = capi.g2_decompress if g2 else capi.g1_decompress
        self.encoding = P.g2_encoding if g2 else P.g1_encoding
        self.point = P.g2_point if g2 else P.g1_point
        self.lib_decompress = "gs_g2_decompress" if g2 else "gs_g1_decompress"
        self.lib_compress = "gs_g2_compress" if g2 else "gs_g1_compress"

    def x_words(self, xs):
        """x coordinates (ints, or pairs of ints) of any size below 2^256 -> [n, cw] uint64"""
        flat = [c for x in xs for c in x] if self.g2 else list(xs)
        return capi.ints_to_u64(flat).reshape(len(xs), self.cw)

    def rows(self, affine):
        """affine points or None -> the [n, jw] words a download gives"""
        one = (1, 0) if self.g2 else 1
        return self.to_u64([self.zero if a is None else (a[0], a[1], one) for a in affine])

    def neg_y(self, y):
        return ((-y[0]) % Q, (-y[1]) % Q) if self.g2 else (-y) % Q

    def rand_x(self, rng):
        return (rng.randrange(Q), rng.randrange(Q)) if self.g2 else rng.randrange(Q)


def _g1_multiples(n, first):
    p, out = O.G1.MulScalar(O.G1_GEN, first), []
    for _ in range(n):
        a = O.G1.Affine(p)
        out.append((a[0], a[1], 1))
        p = O.G1.Add(p, O.G1_GEN)
    return out


@pytest.fixture(scope="module", params=[False, True], ids=["g1", "g2"])
def grp(request):
    """(the group, NMAX points of the oracle, their upload words): generator multiples, every third negated, every fifth infinity, and for
    G2 every seventh a twist point outside the subgroup."""
    g = Group(request.param)
    pts = M.subgroup_multiples(NMAX, first=3) if g.g2 else _g1_multiples(NMAX, 3)
    twist = iter(M.twist_points(NMAX // 7 + 1)) if g.g2 else None
    for i in range(NMAX):
        if g.g2 and i % 7 == 6:
            pts[i] = next(twist)
        if i % 3 == 2:
            pts[i] = g.G.Neg(pts[i])
        if i % 5 == 4:
            pts[i] = g.zero
    return g, pts, g.to_u64(pts)


@pytest.mark.parametrize("n", SIZES)
def test_compress_equals_the_integer_encoding_and_decompress_gives_the_array_back(grp, n):
    g, pts, words = grp
    h = g.upload(words[:n])
    x, flags = g.compress(h)
    enc = [g.encoding(p) for p in pts[:n]]
    assert np.array_equal(x, g.x_words([e[0] for e in enc]))
    assert flags.tolist() == [e[1] for e in enc]
    back, ok = g.decompress(x, flags)
    assert ok.tolist() == [True] * n and len(back) == n
    assert np.array_equal(g.download(back), g.download(h))
    assert capi.handle_bytes(back)[1] == 0                       # no window table was built
    if n > 2:                                                    # a window of the array
        x2, f2 = g.compress(h, 1, n - 2)
        assert np.array_equal(x2, x[1:n - 1]) and np.array_equal(f2, flags[1:n - 1])
        assert g.compress(h, n, 0)[0].shape == (0, g.cw)


def _decompress_raw(g, x, flags, want_ok=True):
    """The library call itself -> (handle, ok or None, nbad, first_bad)."""
    lib = capi.load_library()
    n = len(flags)
    ok = np.full(max(n, 1), 9, dtype=np.uint8) if want_ok else None
    h, nbad, first = capi.Handle(0), ctypes.c_uint64(5), ctypes.c_uint64(5)
    f = np.ascontiguousarray(flags, dtype=np.uint8)
    capi.check(getattr(lib, g.lib_decompress)(capi.ptr64(np.ascontiguousarray(x, dtype=np.uint64)) if n else None, f.ctypes.data_as(capi.u8p) if n else None, n,
                                              ctypes.byref(h), ok.ctypes.data_as(capi.u8p) if want_ok else None, ctypes.byref(nbad), ctypes.byref(first)))
    return capi.DeviceHandle(h.value), (ok[:n] if want_ok else None), nbad.value, first.value


def test_random_x_with_and_without_a_root(grp):
    g = grp[0]
    rng = random.Random(7)
    xs = [g.rand_x(rng) for _ in range(100)]
    flags = [rng.randrange(2) for _ in xs]
    want = [g.point(x, f) for x, f in zip(xs, flags)]
    bad = [i for i, w in enumerate(want) if w is None]
    assert len(bad) >= 30 and len(xs) - len(bad) >= 30
    h, ok, nbad, first = _decompress_raw(g, g.x_words(xs), flags)
    assert ok.tolist() == [int(w is not None) for w in want]
    assert (nbad, first) == (len(bad), bad[0])
    assert np.array_equal(g.download(h), g.rows(want))          # the root the sign rule picks; infinity where there is none
    # the same x with the other flag: the other root
    h2, ok2 = g.decompress(g.x_words(xs), [1 - f for f in flags])
    other = [None if w is None else (w[0], g.neg_y(w[1])) for w in want]
    assert ok2.tolist() == [w is not None for w in want] and np.array_equal(g.download(h2), g.rows(other))


def test_out_of_range_coordinates_and_inconsistent_flags(grp):
    g, pts, _ = grp
    good_x, good_f = g.encoding(pts[0])
    big = [Q, Q + 1, (1 << 256) - 1]
    if g.g2:
        cases = [((b, good_x[1]), 0) for b in big] + [((good_x[0], b), 0) for b in big] + [((good_x[0], b), LARGEST) for b in big]
        zero = (0, 0)
    else:
        cases = [(b, 0) for b in big] + [(b, LARGEST) for b in big]
        zero = 0
    cases += [(good_x, INF), (good_x, INF | LARGEST), (zero, INF | LARGEST), (good_x, 4), (good_x, good_f | 4), (good_x, 0x80), (good_x, good_f | 0x80),
              (zero, INF | 4), (zero, 0), (zero, LARGEST)]           # x = 0 is on neither curve
    xs, flags = [], []
    for x, f in cases:                                              # every case between two good entries
        xs += [good_x, x]
        flags += [good_f, f]
    xs += [good_x, zero]
    flags += [good_f, INF]                                          # ... and a well-formed infinity at the end
    h, ok, nbad, first = _decompress_raw(g, g.x_words(xs), flags)
    want_ok = [1, 0] * len(cases) + [1, 1]
    assert ok.tolist() == want_ok and (nbad, first) == (len(cases), 1)
    a = g.G.Affine(pts[0])
    assert np.array_equal(g.download(h), g.rows([a, None] * len(cases) + [a, None]))


def test_a_bad_entry_leaves_its_neighbours_alone(grp):
    g, pts, words = grp
    n = 129
    h = g.upload(words[:n])
    x, flags = g.compress(h)
    clean = g.download(h)
    no_root = next(v for v in range(1, 50) if g.point((v, 0) if g.g2 else v, 0) is None)
    for at in (0, 63, 64, n - 1):
        bx, bf = x.copy(), flags.copy()
        bx[at] = g.x_words([(no_root, 0) if g.g2 else no_root])[0]
        bf[at] = 0
        hb, ok, nbad, first = _decompress_raw(g, bx, bf)
        want = clean.copy()
        want[at] = 0
        assert (nbad, first) == (1, at) and ok.tolist() == [int(i != at) for i in range(n)]
        assert np.array_equal(g.download(hb), want)
    bf = flags.copy()
    bf[[0, 63, 64, n - 1]] = 8
    assert _decompress_raw(g, x, bf)[2:] == (4, 0)


def test_ok_may_be_null_and_n_may_be_zero(grp):
    g, pts, words = grp
    h = g.upload(words[:65])
    x, flags = g.compress(h)
    flags[64] = 4
    hb, ok, nbad, first = _decompress_raw(g, x, flags, want_ok=False)
    assert ok is None and (nbad, first) == (1, 64) and len(hb) == 65
    assert capi.last_timing()["total_ms"] > 0.0
    he, ok, nbad, first = _decompress_raw(g, np.zeros((0, g.cw), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    assert len(he) == 0 and ok.shape == (0,) and (nbad, first) == (0, NONE)
    he2, ok2 = g.decompress(np.zeros((0, g.cw), dtype=np.uint64), np.zeros(0, dtype=np.uint8))
    assert len(he2) == 0 and ok2.shape == (0,)
    assert g.compress(he2)[0].shape == (0, g.cw)


def test_errors_leave_the_array_usable(grp):
    g, pts, words = grp
    n = 65
    h = g.upload(words[:n])
    other = (capi.g1_upload if g.g2 else capi.g2_upload)((capi.g1_points_to_u64 if g.g2 else capi.g2_points_to_u64)([O.G1_GEN if g.g2 else O.G2_GEN]))
    sc = capi.scalars_upload(capi.ints_to_u64([1, 2, 3]))
    lib = capi.load_library()
    x, f = np.zeros((n, g.cw), dtype=np.uint64), np.zeros(n, dtype=np.uint8)
    px, pf = capi.ptr64(x), f.ctypes.data_as(capi.u8p)
    compress = getattr(lib, g.lib_compress)
    for args, code in (((capi.raw(other), 0, 1, px, pf), -3), ((capi.raw(sc), 0, 1, px, pf), -3), ((0, 0, 1, px, pf), -3),
                       ((capi.raw(h), 0, n, None, pf), -3), ((capi.raw(h), 0, n, px, None), -3),
                       ((capi.raw(h), 1, n, px, pf), -4), ((capi.raw(h), n + 1, 0, px, pf), -4), ((capi.raw(h), 0, n + 1, px, pf), -4)):
        assert compress(*args) == code, args
        assert g.lib_compress.encode() in lib.gs_last_error()
    decompress = getattr(lib, g.lib_decompress)
    out, nbad, first = capi.Handle(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
    full = (px, pf, n, ctypes.byref(out), None, ctypes.byref(nbad), ctypes.byref(first))
    for i in (0, 1, 3, 5, 6):                                       # x, flags, out, nbad, first_bad
        args = list(full)
        args[i] = None
        assert decompress(*args) == -3, i
        assert g.lib_decompress.encode() in lib.gs_last_error()
    with pytest.raises(capi.GosnarkHipError) as e:
        g.compress(h, 1, n)
    assert e.value.code == -4
    assert np.array_equal(g.download(h), g.download(g.upload(words[:n])))
    x2, f2 = g.compress(h)
    assert f2.tolist() == [g.encoding(p)[1] for p in pts[:n]]


def test_decompressed_arrays_are_ordinary_arrays(grp):
    g, pts, words = grp
    n = 129
    h = g.upload(words[:n])
    back, ok = g.decompress(*g.compress(h))
    assert ok.all()
    one = capi.scalars_upload(capi.ints_to_u64([1]))
    if g.g2:
        want = capi.g2_subgroup_check(h)
        assert want[0] == len(range(6, n, 7)) - len([i for i in range(6, n, 7) if i % 5 == 4]) and want[1] == 6
        assert capi.g2_subgroup_check(back) == want
        for i in (0, 6, 64, 128):
            assert capi.g2_subgroup_check(back, i, 1) == capi.g2_subgroup_check(h, i, 1)
    for i in (0, 2, 63, 64, 128):
        assert capi.msm_resident(back, one, 1, off=i, g2=g.g2) == g.G.Affine(pts[i])
