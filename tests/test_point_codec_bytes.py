"""The byte codecs of compressed points (go-snark-study_amd/compressed.py) alone, no device: byte-level vectors of the three presets,
Decode(Encode(.)) over random inputs, and what an invalid tag decodes to."""
import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, compressed as Z
from oracle import ref_py as O

Q = O.Q
G2X, G2Y = O.G2.Affine(O.G2_GEN)
LARGEST, INF = capi.POINT_LARGEST_Y, capi.POINT_INFINITY
#               tag of: smaller, larger, infinity, the invalid one
TAGS = {"GNARK": (0b10, 0b11, 0b01, 0b00), "BN256_PAIRING": (0b00, 0b10, 0b01, 0b11), "ARKWORKS": (0b00, 0b10, 0b01, 0b11)}


def larger(y):
    return y > Q - y


def larger2(y):
    return larger(y[1]) if y[1] else larger(y[0])


def want_bytes(codec, halves, tag):
    """The encoding from Python integers: halves = (c0,) or (c0, c1)."""
    order = list(halves[::-1]) if (len(halves) == 2 and codec.c1_first) else list(halves)
    b = bytearray(b"".join(h.to_bytes(32, "big" if codec.big_endian else "little") for h in order))
    b[0 if codec.big_endian else len(b) - 1] |= tag << 6
    return bytes(b)


def test_presets_are_what_the_table_says():
    assert [c.name for c in Z.PRESETS] == ["GNARK", "BN256_PAIRING", "ARKWORKS"]
    assert (Z.GNARK.big_endian, Z.GNARK.c1_first) == (True, True)
    assert (Z.BN256_PAIRING.big_endian, Z.BN256_PAIRING.c1_first) == (True, True)
    assert (Z.ARKWORKS.big_endian, Z.ARKWORKS.c1_first) == (False, False)
    for c in Z.PRESETS:
        s, l, i, bad = TAGS[c.name]
        assert (c.tags[s], c.tags[l], c.tags[i], c.tags[bad]) == (Z.SMALLER, Z.LARGER, Z.INFINITY, Z.INVALID)
    assert Z.PointCodec("x", True, True, Z.GNARK.tags) == Z.GNARK and Z.GNARK != Z.BN256_PAIRING and hash(Z.BN256_PAIRING) != hash(Z.ARKWORKS)
    with pytest.raises(AttributeError):
        Z.GNARK.big_endian = False
    with pytest.raises(ValueError):
        Z.PointCodec("x", True, True, (Z.SMALLER, Z.SMALLER, Z.LARGER, Z.INFINITY))


def test_g1_generator_its_negative_and_infinity_under_gnark_byte_by_byte():
    assert not larger(2)                                             # (1, 2): y is the smaller root
    x = capi.ints_to_u64([1, 1, 0])
    got = Z.EncodeG1(x, np.array([0, LARGEST, INF], dtype=np.uint8), Z.GNARK)
    assert got.shape == (3, 32) and got.dtype == np.uint8
    assert got[0].tobytes() == b"\x80" + bytes(30) + b"\x01"
    assert got[1].tobytes() == b"\xc0" + bytes(30) + b"\x01"
    assert got[2].tobytes() == b"\x40" + bytes(31)


@pytest.mark.parametrize("codec", Z.PRESETS, ids=lambda c: c.name)
def test_g1_vectors(codec):
    s, l, i, _ = TAGS[codec.name]
    x = capi.ints_to_u64([1, 1, 0])
    flags = np.array([0, LARGEST, INF], dtype=np.uint8)
    got = Z.EncodeG1(x, flags, codec)
    want = [want_bytes(codec, (1,), s), want_bytes(codec, (1,), l), want_bytes(codec, (0,), i)]
    assert [g.tobytes() for g in got] == want
    if not codec.big_endian:
        assert want[0] == b"\x01" + bytes(31) and want[1] == b"\x01" + bytes(30) + b"\x80" and want[2] == bytes(31) + b"\x40"
    dx, df = Z.DecodeG1(np.frombuffer(b"".join(want), dtype=np.uint8), codec)
    assert np.array_equal(dx, x) and np.array_equal(df, flags)


@pytest.mark.parametrize("codec", Z.PRESETS, ids=lambda c: c.name)
def test_g2_generator_and_its_negative_with_the_halves_in_the_presets_order(codec):
    s, l, _, _ = TAGS[codec.name]
    big = larger2(G2Y)
    x = capi.ints_to_u64([G2X[0], G2X[1]] * 2).reshape(2, 8)
    flags = np.array([LARGEST if big else 0, 0 if big else LARGEST], dtype=np.uint8)      # the generator, its negative
    got = Z.EncodeG2(x, flags, codec)
    want = [want_bytes(codec, G2X, l if big else s), want_bytes(codec, G2X, s if big else l)]
    assert got.shape == (2, 64) and [g.tobytes() for g in got] == want
    first = want[0][:32]
    if codec.c1_first:
        assert (int.from_bytes(first, "big") & ((1 << 254) - 1)) == G2X[1]
    else:
        assert int.from_bytes(first, "little") == G2X[0]
    dx, df = Z.DecodeG2(np.frombuffer(b"".join(want), dtype=np.uint8).reshape(2, 64), codec)
    assert np.array_equal(dx, x) and np.array_equal(df, flags)


@pytest.mark.parametrize("codec", Z.PRESETS, ids=lambda c: c.name)
def test_decode_of_encode_is_the_identity(codec):
    rng = np.random.default_rng(5)
    for words, enc, dec in ((4, Z.EncodeG1, Z.DecodeG1), (8, Z.EncodeG2, Z.DecodeG2)):
        x = rng.integers(0, 1 << 64, size=(300, words), dtype=np.uint64)
        x[:, 3::4] &= np.uint64((1 << 62) - 1)                        # 254 bits per coordinate
        flags = rng.integers(0, 3, size=300).astype(np.uint8)
        b = enc(x, flags, codec)
        assert b.shape == (300, 8 * words)
        dx, df = dec(b, codec)
        assert dx.dtype == np.uint64 and df.dtype == np.uint8 and np.array_equal(dx, x) and np.array_equal(df, flags)
        dx, df = dec(b.reshape(-1), codec)                            # a flat buffer is n encodings
        assert np.array_equal(dx, x) and np.array_equal(df, flags)
    assert Z.DecodeG1(np.zeros((0, 32), dtype=np.uint8), codec)[0].shape == (0, 4)


@pytest.mark.parametrize("codec", Z.PRESETS, ids=lambda c: c.name)
def test_an_invalid_tag_decodes_to_a_flag_the_device_rejects(codec):
    bad = TAGS[codec.name][3]
    for halves, dec in (((1,), Z.DecodeG1), (G2X, Z.DecodeG2)):
        b = want_bytes(codec, halves, bad)
        x, f = dec(np.frombuffer(b, dtype=np.uint8), codec)
        assert f.shape == (1,) and int(f[0]) & ~3 and capi.u64_to_ints(x) == list(halves)


def test_encode_refuses_what_has_no_encoding():
    with pytest.raises(ValueError):
        Z.EncodeG1(capi.ints_to_u64([1]), np.array([4], dtype=np.uint8), Z.GNARK)
    with pytest.raises(ValueError):
        Z.EncodeG1(capi.ints_to_u64([1 << 254]), np.array([0], dtype=np.uint8), Z.GNARK)
    with pytest.raises(ValueError):
        Z.EncodeG1(capi.ints_to_u64([1, 2]), np.array([0], dtype=np.uint8), Z.GNARK)
