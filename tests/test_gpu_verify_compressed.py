"""-m gpu: groth16.VerifyProofsEachCompressed / VerifyProofsCompressed -- proofs as 128-byte blobs of compressed points, decompressed on the
device and verified there.

The proofs and the key are those of test_gpu_verify_each.py (its `batch` fixture: device-made proofs of the committed x^3 + x + 5 key).
The yardstick is VerifyProofsEach on the same proofs; a blob with a point that does not decompress must read False at its own index and
nowhere else.  Batches of 1, 65 and 130: both sides of the one-wave workgroup seam of the decompression kernels (the 2n G1 points of a
batch go through one call)."""
import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, compressed as Z, groth16
import point_codec_util as P
from oracle import ref_py as O
from test_gpu_verify_each import batch  # noqa: F401

pytestmark = pytest.mark.gpu
SIZES = [1, 65, 130]
CODECS = pytest.mark.parametrize("codec", Z.PRESETS, ids=lambda c: c.name)


@pytest.fixture(autouse=True)
def _init():
    capi.init()


def no_root_g1():
    return next(x for x in range(2, 60) if P.g1_point(x, 0) is None)


def no_root_g2():
    return next((x, 1) for x in range(2, 60) if P.g2_point((x, 1), 0) is None)


@CODECS
def test_round_trip_of_proofs(batch, codec):      # noqa: F811
    vk, proofs, pubs = batch
    blobs = Z.CompressProofs(proofs[:65], codec)
    assert len(blobs) == 65 and all(len(b) == 128 for b in blobs)
    assert Z.CompressProof(proofs[3], codec) == blobs[3]
    back, ok = Z.DecompressProofs(blobs, codec)
    assert ok.tolist() == [True] * 65
    assert [(p.PiA, p.PiB, p.PiC) for p in back] == [(p.PiA, p.PiB, p.PiC) for p in proofs[:65]]
    # A | B | C, each point the integer encoding of the oracle's affine point
    xa, fa = Z.DecodeG1(np.frombuffer(blobs[3][:32], dtype=np.uint8), codec)
    xb, fb = Z.DecodeG2(np.frombuffer(blobs[3][32:96], dtype=np.uint8), codec)
    xc, fc = Z.DecodeG1(np.frombuffer(blobs[3][96:], dtype=np.uint8), codec)
    assert (capi.u64_to_ints(xa)[0], int(fa[0])) == P.g1_encoding(proofs[3].PiA)
    assert (tuple(capi.u64_to_ints(xb)), int(fb[0])) == P.g2_encoding(proofs[3].PiB)
    assert (capi.u64_to_ints(xc)[0], int(fc[0])) == P.g1_encoding(proofs[3].PiC)


@CODECS
def test_verdicts_equal_verify_proofs_each_also_with_invalid_proofs_planted(batch, codec):      # noqa: F811
    vk, base, pubs = batch
    for n in SIZES:
        blobs = Z.CompressProofs(base[:n], codec)
        assert groth16.VerifyProofsEachCompressed(vk, blobs, pubs[:n], codec) == [True] * n
        assert groth16.VerifyProofsCompressed(vk, blobs, pubs[:n], codec, seed=n) is True
        proofs, signals = list(base[:n]), [list(s) for s in pubs[:n]]
        spots = sorted({0, n // 2, n - 1})
        for k, at in enumerate(spots):
            p = base[at]
            if k == 0:
                proofs[at] = groth16.Proof(O.G1.Add(p.PiA, O.G1_GEN), p.PiB, p.PiC)
            elif k == 1:
                proofs[at] = groth16.Proof(p.PiA, p.PiB, O.G1.Neg(p.PiC))
            else:
                signals[at][0] += 1
        want = groth16.VerifyProofsEach(vk, proofs, signals)
        assert want == [i not in spots for i in range(n)]
        blobs = Z.CompressProofs(proofs, codec)
        assert groth16.VerifyProofsEachCompressed(vk, blobs, signals, codec) == want
        assert groth16.VerifyProofsCompressed(vk, blobs, signals, codec, seed=n) is False


def _with(blob, lo, hi, piece):
    return blob[:lo] + bytes(piece) + blob[hi:]


@CODECS
def test_a_blob_that_does_not_decompress_reads_false_at_its_own_index_only(batch, codec):      # noqa: F811
    vk, base, pubs = batch
    bad_tag = codec.tag_of(Z.INVALID) << 6
    top = 0 if codec.big_endian else 31
    for n in SIZES:
        clean = Z.CompressProofs(base[:n], codec)
        a_bad = Z.EncodeG1(capi.ints_to_u64([no_root_g1()]), [0], codec)[0].tobytes()
        b_bad = Z.EncodeG2(capi.ints_to_u64(list(no_root_g2())).reshape(1, 8), [capi.POINT_LARGEST_Y], codec)[0].tobytes()
        at_a, at_b, at_tag = 0, n // 2, n - 1
        cases = {"A": (at_a, _with(clean[at_a], 0, 32, a_bad)), "B": (at_b, _with(clean[at_b], 32, 96, b_bad))}
        c = bytearray(clean[at_tag][96:])
        c[top] = (c[top] & 0x3f) | bad_tag
        cases["tag"] = (at_tag, _with(clean[at_tag], 96, 128, c))
        for what, (at, blob) in cases.items():
            blobs = list(clean)
            blobs[at] = blob
            assert groth16.VerifyProofsEachCompressed(vk, blobs, pubs[:n], codec) == [i != at for i in range(n)], (what, n)
            assert groth16.VerifyProofsCompressed(vk, blobs, pubs[:n], codec, seed=1) is False, (what, n)
            _, ok = Z.DecompressProofs(blobs, codec)
            assert ok.tolist() == [i != at for i in range(n)]
        blobs = list(clean)                                                  # all three at once (distinct indices when n > 2)
        for at, blob in cases.values():
            blobs[at] = blob
        bad = {at for at, _ in cases.values()}
        assert groth16.VerifyProofsEachCompressed(vk, blobs, pubs[:n], codec) == [i not in bad for i in range(n)]


def test_ragged_input_is_refused_and_an_empty_batch_is_empty(batch):      # noqa: F811
    vk, base, pubs = batch
    blobs = Z.CompressProofs(base[:2], Z.GNARK)
    with pytest.raises(ValueError):
        groth16.VerifyProofsEachCompressed(vk, blobs, pubs[:1], Z.GNARK)
    with pytest.raises(ValueError):
        groth16.VerifyProofsEachCompressed(vk, [blobs[0][:127]], pubs[:1], Z.GNARK)
    assert groth16.VerifyProofsEachCompressed(vk, [], [], Z.GNARK) == []
