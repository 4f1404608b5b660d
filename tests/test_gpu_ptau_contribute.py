"""-m gpu: gs_g1_scale_powers / gs_g2_scale_powers and circom.NewPtau / ContributePtau -- one phase-1 contribution on the points.

Every input point is a known multiple k_i G of its generator, so every output point has the closed form (k_i c t^i mod r) G; both the
inputs and the expected outputs are made by the C oracle (oracle.c_oracle.g1_mul_scalar / g2_mul_scalar), never by the library's own
fixed-base route.  Every comparison is byte for byte on the .ptau encoding of affine points."""
import functools
import os
import random
import struct

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom
import c_util
import circom_util as CU
from setup_util import Circuit
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = CU.R
SIZE = {False: 64, True: 128}


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)
    yield
    capi.set_table_policy("auto")


@functools.lru_cache(maxsize=None)
def point_bytes(k, g2):
    """(k mod r) G in the .ptau encoding, by the oracle"""
    if g2:
        return circom.G2ToZkey(C.g2_mul_scalar(O.G2_GEN, k % R))
    return circom.G1ToZkey(C.g1_mul_scalar(O.G1_GEN, k % R))


def points(ks, g2):
    return np.frombuffer(b"".join(point_bytes(k, g2) for k in ks), dtype=np.uint8)


def upload(ks, g2):
    return (capi.g2_upload_affine_mont if g2 else capi.g1_upload_affine_mont)(points(ks, g2))


def scale_powers(h, off, n, c, t, g2):
    out = (capi.g2_scale_powers if g2 else capi.g1_scale_powers)(h, off, n, c, t)
    assert len(out) == n
    return (capi.g2_download_affine_mont if g2 else capi.g1_download_affine_mont)(out)


def expected(ks, off, n, c, t, g2):
    return points([ks[off + i] * (c % R) * (pow(t % R, i, R) if i else 1) for i in range(n)], g2)


def multipliers(n, seed):
    rng = random.Random(seed)
    return [rng.randrange(1, R) for _ in range(n)]


# ---- the kernel ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("off", [0, 5])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_sizes_and_offsets(n, off, g2):
    """the launch's block edge and a ragged last block; off + n = the array's length, and one beyond it"""
    rng = random.Random(100 * n + off)
    ks = multipliers(off + n, 7)
    c, t = rng.randrange(1 << 256), rng.randrange(1 << 256)
    h = upload(ks, g2)
    assert np.array_equal(scale_powers(h, off, n, c, t, g2), expected(ks, off, n, c, t, g2))
    for bad_off, bad_n in ((off, n + 1), (off + 1, n), (off + n + 1, 0)):
        with pytest.raises(capi.GosnarkHipError, match="were asked for") as e:
            (capi.g2_scale_powers if g2 else capi.g1_scale_powers)(h, bad_off, bad_n, c, t)
        assert e.value.code == -4                                      # GS_ERR_SHAPE


SCALARS = {"random": (0x2b3c4d5e6f708192a3b4c5d6e7f8091a2b3c4d5e6f708192a3b4c5d6e7f80912 % R, 0x1f2e3d4c5b6a79887766554433221100ffeeddccbbaa99887766554433221101 % R),
           "t=1": (0x123456789abcdef0fedcba9876543210123456789abcdef0fedcba987654321 % R, 1), "t=r-1": (12345, R - 1), "t=0": (R - 2, 0),
           "c=0": (0, 3), "c=r-1": (R - 1, 0x1234567), "unreduced": ((1 << 256) - 1, (1 << 256) - 1)}


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
@pytest.mark.parametrize("kind", list(SCALARS))
def test_scalars(kind, g2):
    c, t = SCALARS[kind]
    n = 65
    ks = multipliers(n, 7)
    got = scale_powers(upload(ks, g2), 0, n, c, t, g2)
    assert np.array_equal(got, expected(ks, 0, n, c, t, g2))
    if kind == "c=0":
        assert not got.any()
    if kind == "t=0":
        assert got[:SIZE[g2]].any() and not got[SIZE[g2]:].any()        # t^0 = 1: c P[0], then infinities


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_infinities_do_not_poison_their_group(g2):
    """infinities at 0, 31, 63, 64 and a whole block of 64 of them (128 .. 191), finite points around them: whatever group of points
    shares one inversion, it holds infinities and finite points side by side"""
    n = 200
    ks = multipliers(n, 8)
    for i in [0, 31, 63, 64] + list(range(128, 192)):
        ks[i] = 0
    c, t = SCALARS["random"]
    got = scale_powers(upload(ks, g2), 0, n, c, t, g2)
    assert np.array_equal(got, expected(ks, 0, n, c, t, g2))
    rows = got.reshape(n, -1)
    assert [i for i in range(n) if not rows[i].any()] == [0, 31, 63, 64] + list(range(128, 192))


@pytest.mark.parametrize("g2", [False, True], ids=["g1", "g2"])
def test_equal_and_opposite_neighbours(g2):
    """P, P and -P side by side, with t = 1 and with a series"""
    k = multipliers(1, 9)[0]
    ks = [k, k, R - k] * 3 + [1, R - 1]
    for c, t in (SCALARS["t=1"], SCALARS["random"]):
        assert np.array_equal(scale_powers(upload(ks, g2), 0, len(ks), c, t, g2), expected(ks, 0, len(ks), c, t, g2))


def test_uniform_scale_equals_gs_g1_scale():
    ks = multipliers(130, 10)
    ks[3] = 0
    h = upload(ks, False)
    for c in (SCALARS["random"][0], 0, 1, R - 1):
        want = capi.g1_download_affine_mont(capi.g1_scale(h, c))
        assert np.array_equal(scale_powers(h, 0, len(ks), c, 1, False), want)


def test_bad_handles_and_kinds():
    h1, h2 = upload([1, 2], False), upload([1, 2], True)
    for f, wrong in ((capi.g1_scale_powers, h2), (capi.g2_scale_powers, h1), (capi.g1_scale_powers, capi.DeviceHandle(0))):
        with pytest.raises(capi.GosnarkHipError, match="bad base-array handle") as e:
            f(wrong, 0, 1, 2, 3)
        assert e.value.code == -3                                      # GS_ERR_ARG


# ---- transcripts -----------------------------------------------------------------------------------------------------------------
def oracle_sections(power, tau, alpha, beta):
    """{section id: bytes} of the transcript of (tau, alpha, beta), every point by the oracle"""
    n = 1 << power
    pw = [pow(tau, i, R) for i in range(2 * n - 1)]
    return {2: points(pw, False), 3: points(pw[:n], True), 4: points([alpha * x for x in pw[:n]], False),
            5: points([beta * x for x in pw[:n]], False), 6: points([beta], True)}


def file_sections(path):
    data = open(path, "rb").read()
    nsec, pos, out = struct.unpack("<I", data[8:12])[0], 12, []
    for _ in range(nsec):
        sid, length = struct.unpack("<IQ", data[pos:pos + 12])
        out.append((sid, np.frombuffer(data[pos + 12:pos + 12 + length], dtype=np.uint8)))
        pos += 12 + length
    assert pos == len(data)
    return out


def assert_transcript(path, want):
    got = dict(file_sections(path))
    for sid in (2, 3, 4, 5, 6):
        assert np.array_equal(got[sid], want[sid]), "section %d" % sid


TOXIC = [tuple(random.Random(40 + i).randrange(2, R) for _ in range(3)) for i in range(2)]


def test_slab_seams(tmp_path):
    """power 4: 31 tauG1 points in slabs of 4 (a ragged last slab, 8 slabs) against one slab, and against the oracle"""
    src, a, b = (str(tmp_path / n) for n in ("new.ptau", "a.ptau", "b.ptau"))
    circom.NewPtau(src, 4)
    tau, alpha, beta = TOXIC[0]
    ta, tb = {}, {}
    circom.ContributePtau(src, a, tau, alpha, beta, slab_log2=2, timing=ta)
    circom.ContributePtau(src, b, tau, alpha, beta, slab_log2=22, timing=tb)
    assert open(a, "rb").read() == open(b, "rb").read()
    assert (ta["slabs"], tb["slabs"]) == (8 + 4 + 4 + 4 + 1, 5) and ta["power"] == 4
    assert_transcript(a, oracle_sections(4, tau, alpha, beta))
    assert bytes(dict(file_sections(a))[1]) == bytes(dict(file_sections(src))[1])
    # device memory is bounded by the slab, not by the section: in + out of the largest slab (4 G2 points) and nothing kept
    assert ta["library_bytes_max"] <= tb["library_bytes_max"]


def test_composition(tmp_path):
    """two contributions on the transcript of ones = the transcript of the products, betaG2 included; and = WritePtau of the products"""
    p0, p1, p2, pw = (str(tmp_path / n) for n in ("0.ptau", "1.ptau", "2.ptau", "w.ptau"))
    (t1, a1, b1), (t2, a2, b2) = TOXIC
    circom.NewPtau(p0, 3)
    circom.ContributePtau(p0, p1, t1, a1, b1)
    circom.ContributePtau(p1, p2, t2, a2, b2, slab_log2=3)
    tau, alpha, beta = t1 * t2 % R, a1 * a2 % R, b1 * b2 % R
    assert_transcript(p1, oracle_sections(3, t1, a1, b1))
    assert_transcript(p2, oracle_sections(3, tau, alpha, beta))
    circom.WritePtau(pw, 3, tau, alpha, beta)
    assert [s for s, _ in file_sections(p2)] == [1, 2, 3, 4, 5, 6]
    assert open(p2, "rb").read() == open(pw, "rb").read()


def test_sections_7_is_copied_12_is_dropped_and_ceremony_power_stays(tmp_path):
    src, dst = str(tmp_path / "in.ptau"), str(tmp_path / "out.ptau")
    rec, unknown = bytes(range(200)), b"\x01\x02\x03"
    circom.WritePtau(src, 2, 5, 6, 7, extra_sections=[(7, rec), (12, bytes(4 * 64)), (99, unknown), (15, b"")])
    data = bytearray(open(src, "rb").read())
    off = 12 + 12 + 40                                                 # the header section's ceremonyPower
    assert struct.unpack("<I", data[off:off + 4])[0] == 2
    data[off:off + 4] = struct.pack("<I", 9)
    with open(src, "wb") as f:
        f.write(bytes(data))
    tau, alpha, beta = TOXIC[1]
    circom.ContributePtau(src, dst, tau, alpha, beta)
    secs = file_sections(dst)
    assert [s for s, _ in secs] == [1, 2, 3, 4, 5, 6, 7, 99]
    assert bytes(dict(secs)[7]) == rec and bytes(dict(secs)[99]) == unknown
    p = circom.ReadPtau(dst)
    assert (p.power, p.ceremonyPower) == (2, 9)
    assert_transcript(dst, oracle_sections(2, 5 * tau % R, 6 * alpha % R, 7 * beta % R))


def test_end_to_end_with_a_contributed_transcript(tmp_path):
    """NewPtau -> two contributions -> VerifyPtau; SetupFromPtau -> ContributeDelta -> VerifyZkey; the key proves; and a transcript
    where only tauG1 was contributed fails VerifyPtau"""
    k, npub, nc = 3, 1, 3                                                # the k3 shape of tests/test_gpu_setup_ptau.py
    c = Circuit(k, npub, nc, 1000 + 10 * k + npub)
    paths = {n: str(tmp_path / n) for n in ("c.r1cs", "0.ptau", "1.ptau", "2.ptau", "c.zkey", "d.zkey", "mixed.ptau")}
    c.write_r1cs(paths["c.r1cs"])
    t1, a1, b1 = TOXIC[0]
    t2, a2, b2 = (x * pow(y, -1, R) % R for x, y in ((c.tau, t1), (c.alpha, a1), (c.beta, b1)))      # the products are the circuit's toxic values
    circom.NewPtau(paths["0.ptau"], k + 1)
    circom.ContributePtau(paths["0.ptau"], paths["1.ptau"], t1, a1, b1)
    circom.ContributePtau(paths["1.ptau"], paths["2.ptau"], t2, a2, b2, slab_log2=3)
    assert circom.VerifyPtau(paths["2.ptau"], seed=1)
    circom.SetupFromPtau(paths["c.r1cs"], paths["2.ptau"], paths["c.zkey"])
    delta = random.Random(9).randrange(2, R)
    circom.ContributeDelta(paths["c.zkey"], paths["d.zkey"], delta)
    assert circom.VerifyZkey(paths["c.r1cs"], paths["2.ptau"], paths["d.zkey"], seed=2)
    key, system = circom.UploadZkey(paths["d.zkey"])
    vk = circom.VerificationKeyFromZkey(circom.ReadZkey(paths["d.zkey"]))
    public = c.w[1:npub + 1]
    proof = circom.GenerateProofsWithRS(key, system, c.w, 11, 12)
    CU.assert_closed_form(proof, c.proof_scalars(c.w, 11, 12, delta))
    assert circom.VerifyFromCircom(vk, proof, public)
    assert not circom.VerifyFromCircom(vk, proof, [(public[0] + 1) % R])
    # section 2 of the contributed file in the file of ones: tauG1 no longer fits tauG2
    new, done = dict(file_sections(paths["0.ptau"])), dict(file_sections(paths["1.ptau"]))
    with open(paths["mixed.ptau"], "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, 6))
        for sid in range(1, 7):
            body = bytes((done if sid == 2 else new)[sid])
            f.write(struct.pack("<IQ", sid, len(body)) + body)
    rep = circom.VerifyPtau(paths["mixed.ptau"], seed=3)
    assert not rep and "tau" in rep.failed


def test_ptau_contribute_c_sequence_gives_the_python_routes_sections(tmp_path):
    """tests/c/ptau_contribute.c, the call sequence of go/gosnarkhip/ptau.go from a process without Python"""
    src, dst, sc, out = (str(tmp_path / n) for n in ("in.ptau", "out.ptau", "scalars.bin", "c.out"))
    circom.WritePtau(src, 3, 11, 12, 13)
    tau, alpha, beta = TOXIC[0]
    circom.ContributePtau(src, dst, tau, alpha, beta)
    c_util._blob(sc, [capi.ints_to_u64([tau, alpha, beta])])
    stdout = c_util.build_and_run("ptau_contribute.c", [src, sc, out], tmp_path)
    assert "OK power 3" in stdout, stdout
    want = dict(file_sections(dst))
    assert open(out, "rb").read() == b"".join(bytes(want[sid]) for sid in (2, 3, 4, 5, 6))
    assert os.path.getsize(out) == (15 + 16) * 64 + 9 * 128
