"""Compressed points and proofs: the byte codecs of three libraries around gs_g1_decompress / gs_g2_decompress / gs_g*_compress.

A compressed point is its x coordinate and a two-bit tag in the two most significant bits of the most significant byte (q has 254 bits,
the bits are free): which of the two roots y is, or that the point is the one at infinity.  All three presets use ONE sign rule -- y is
the larger of {y, q - y} as canonical integers, an Fq2 element compared by c1 first and by c0 only when c1 = 0 -- and differ in byte
order, in the order of the Fq2 halves and in the tag values.  The device sees none of that (include/gosnark_hip.h, "compressed points"):
Decode* turn bytes into x words and flag bytes with numpy alone, a malformed encoding becomes a flag value the device rejects, and what
does not decode is reported per point, never raised.

    proofs, ok = DecompressProofs(blobs, GNARK)            # one G1 call over the 2n points A, C and one G2 call
    verdicts = groth16.VerifyProofsEachCompressed(vk, blobs, publicSignalsList, GNARK)

The layouts of the presets are written down from those projects' sources from memory; no file written by any of them has been read
(README, "Compressed points")."""
import numpy as np

from . import capi, groth16

SMALLER, LARGER, INFINITY, INVALID = "smaller", "larger", "infinity", "invalid"
_FLAG_OF = {SMALLER: 0, LARGER: capi.POINT_LARGEST_Y, INFINITY: capi.POINT_INFINITY, INVALID: 4}      # 4: a bit above bit 1, the device says bad


class PointCodec:
    """A wire format of compressed points: the byte order of a coordinate, the order of the Fq2 halves, and what each value of the
    two-bit tag (the two most significant bits of the encoding's most significant byte) means.  A value type: equal when the fields are."""

    __slots__ = ("name", "big_endian", "c1_first", "tags")

    def __init__(self, name, big_endian, c1_first, tags):
        tags = tuple(tags)
        if len(tags) != 4 or any(t not in _FLAG_OF for t in tags) or sorted(t for t in tags if t != INVALID) != sorted([SMALLER, LARGER, INFINITY]):
            raise ValueError("PointCodec: tags maps 0b00 .. 0b11 to smaller, larger, infinity and invalid, each once")
        object.__setattr__(self, "name", name)
        object.__setattr__(self, "big_endian", bool(big_endian))
        object.__setattr__(self, "c1_first", bool(c1_first))
        object.__setattr__(self, "tags", tags)

    def __setattr__(self, k, v):
        raise AttributeError("PointCodec is immutable")

    def _key(self):
        return (self.big_endian, self.c1_first, self.tags)

    def __eq__(self, other):
        return isinstance(other, PointCodec) and self._key() == other._key()

    def __hash__(self):
        return hash(self._key())

    def __repr__(self):
        return "PointCodec(%s)" % self.name

    def tag_of(self, meaning):
        return self.tags.index(meaning)


GNARK = PointCodec("GNARK", True, True, (INVALID, INFINITY, SMALLER, LARGER))               # 0b00 marks an uncompressed point there
BN256_PAIRING = PointCodec("BN256_PAIRING", True, True, (SMALLER, INFINITY, LARGER, INVALID))
ARKWORKS = PointCodec("ARKWORKS", False, False, (SMALLER, INFINITY, LARGER, INVALID))       # little-endian: the tag sits in the LAST byte
PRESETS = (GNARK, BN256_PAIRING, ARKWORKS)


def _decode(buf, codec, halves):
    size = 32 * halves
    b = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1, size).copy()
    top = 0 if codec.big_endian else size - 1
    tag = b[:, top] >> 6
    b[:, top] &= 0x3f
    h = b.reshape(-1, halves, 32)
    if codec.big_endian:
        h = h[:, :, ::-1]                                      # every coordinate to little-endian bytes
    if halves == 2 and codec.c1_first:
        h = h[:, ::-1, :]                                      # to c0 | c1
    x = np.ascontiguousarray(h).reshape(-1, size).view("<u8").astype(np.uint64).reshape(-1, 4 * halves)
    flags = np.array([_FLAG_OF[t] for t in codec.tags], dtype=np.uint8)[tag]
    return x, flags


def _encode(x_u64, flags, codec, halves):
    size = 32 * halves
    x = np.ascontiguousarray(x_u64, dtype="<u8").reshape(-1, 4 * halves)
    f = np.ascontiguousarray(flags, dtype=np.uint8).reshape(-1)
    if f.shape[0] != x.shape[0]:
        raise ValueError("%d x coordinates, %d flag bytes" % (x.shape[0], f.shape[0]))
    if np.any(f > 2):
        raise ValueError("a flag byte is none of 0, POINT_LARGEST_Y, POINT_INFINITY")
    h = x.view(np.uint8).reshape(-1, halves, 32)
    if np.any(h[:, :, 31] >> 6):
        raise ValueError("a coordinate has more than 254 bits: no room for the tag")
    if halves == 2 and codec.c1_first:
        h = h[:, ::-1, :]
    if codec.big_endian:
        h = h[:, :, ::-1]
    b = np.ascontiguousarray(h).reshape(-1, size).copy()
    tag_of_flag = np.array([codec.tag_of(SMALLER), codec.tag_of(LARGER), codec.tag_of(INFINITY)], dtype=np.uint8)
    b[:, 0 if codec.big_endian else size - 1] |= tag_of_flag[f] << 6
    return b


def DecodeG1(buf, codec):
    """[n, 32] uint8 (or n x 32 bytes) -> (x as [n, 4] uint64, flag bytes) as gs_g1_decompress takes them.  An invalid tag becomes a flag
    value with a bit above bit 1: the device reports the entry as bad."""
    return _decode(buf, codec, 1)


def DecodeG2(buf, codec):
    """[n, 64] uint8 -> (x as [n, 8] uint64 in the order c0 | c1, flag bytes)."""
    return _decode(buf, codec, 2)


def EncodeG1(x_u64, flags, codec):
    """The inverse of DecodeG1 -> [n, 32] uint8.  Flag bytes other than 0, POINT_LARGEST_Y, POINT_INFINITY and coordinates of more than 254
    bits have no encoding: ValueError."""
    return _encode(x_u64, flags, codec, 1)


def EncodeG2(x_u64, flags, codec):
    return _encode(x_u64, flags, codec, 2)


def _as_rows(buf, size):
    if isinstance(buf, (bytes, bytearray, memoryview)):
        buf = np.frombuffer(bytes(buf), dtype=np.uint8)
    a = np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1)
    if a.size % size:
        raise ValueError("%d bytes are not a whole number of %d-byte encodings" % (a.size, size))
    return a.reshape(-1, size)


def DecompressG1(buf, codec):
    """n x 32 bytes -> ([(x, y, 1), ...] as ints, (0, 0, 0) for infinity AND for an encoding that does not decode; a bool array: which
    decoded).  One gs_g1_decompress call."""
    h, ok = capi.g1_decompress(*DecodeG1(_as_rows(buf, 32), codec))
    return capi.g1_tuples(capi.g1_download(h)), ok


def DecompressG2(buf, codec):
    """n x 64 bytes -> ([((x0, x1), (y0, y1), (1, 0)), ...], which decoded).  The points are on the twist; membership of the order-r
    subgroup is not tested (capi.g2_subgroup_check)."""
    h, ok = capi.g2_decompress(*DecodeG2(_as_rows(buf, 64), codec))
    return capi.g2_tuples(capi.g2_download(h)), ok


def CompressG1(points, codec):
    """Jacobian int triples -> n x 32 bytes.  One upload (which refuses a point off the curve) and one gs_g1_compress call."""
    if not points:
        return b""
    return EncodeG1(*capi.g1_compress(capi.g1_upload(capi.g1_points_to_u64(points))), codec).tobytes()


def CompressG2(points, codec):
    if not points:
        return b""
    return EncodeG2(*capi.g2_compress(capi.g2_upload(capi.g2_points_to_u64(points))), codec).tobytes()


def CompressProofs(proofs, codec):
    """[groth16.Proof] -> [128 bytes each], A | B | C; the 2n G1 points in one call and the G2 points in one."""
    n = len(proofs)
    if not n:
        return []
    g1 = np.frombuffer(CompressG1([p.PiA for p in proofs] + [p.PiC for p in proofs], codec), dtype=np.uint8).reshape(2 * n, 32)
    g2 = np.frombuffer(CompressG2([p.PiB for p in proofs], codec), dtype=np.uint8).reshape(n, 64)
    blobs = np.concatenate([g1[:n], g2, g1[n:]], axis=1)
    return [blobs[i].tobytes() for i in range(n)]


def CompressProof(proof, codec):
    """groth16.Proof -> 128 bytes, A | B | C."""
    return CompressProofs([proof], codec)[0]


def decompress_proof_arrays(blobs, codec):
    """n blobs of 128 bytes -> (A as [n, 12] uint64 Jacobian words, B as [n, 24], C as [n, 12], a bool array: every point of the proof
    decoded).  One gs_g1_decompress call over A and C and one gs_g2_decompress call; no Python integers on the way."""
    rows = _as_rows(b"".join(bytes(b) for b in blobs) if isinstance(blobs, (list, tuple)) else blobs, 128)
    n = rows.shape[0]
    if not n:
        return np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64), np.zeros((0, 12), dtype=np.uint64), np.zeros(0, dtype=bool)
    h1, ok1 = capi.g1_decompress(*DecodeG1(np.concatenate([rows[:, :32], rows[:, 96:]]), codec))
    h2, ok2 = capi.g2_decompress(*DecodeG2(rows[:, 32:96], codec))
    g1 = capi.g1_download(h1)
    return g1[:n], capi.g2_download(h2), g1[n:], ok1[:n] & ok2 & ok1[n:]


def DecompressProofs(blobs, codec):
    """n blobs of 128 bytes (A | B | C) -> ([groth16.Proof], a bool array: every point of the proof decoded).  A point that does not
    decode is the point at infinity in its proof.  B is not tested for subgroup membership."""
    a, b, c, ok = decompress_proof_arrays(blobs, codec)
    pa, pb, pc = capi.g1_tuples(a), capi.g2_tuples(b), capi.g1_tuples(c)
    return [groth16.Proof(pa[i], pb[i], pc[i]) for i in range(len(pa))], ok
