"""-m gpu: circom.SetupFromPtau / ContributeDelta -- circuit.r1cs + a powers-of-tau file -> circuit.zkey on the device.

The circuits are synthetic (a chain of products with a satisfying witness, nPublic in {0, 1, 3}) and the transcripts are written from
toxic values (circom.WritePtau), so every point of the key has a closed form in the generators: scalars in Python integers, points by the
C oracle or gs_g*_fixed_base.  Every comparison is bit for bit on affine points."""
import random
import struct

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom, groth16
import circom_util as CU
from setup_util import Circuit
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = CU.R
SHAPES = {"k1": (1, 0, 1), "k3_full": (3, 3, 4), "k3": (3, 1, 3), "k10": (10, 1, 600)}      # name -> (k, nPublic, nConstraints)


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)
    yield
    capi.set_table_policy("auto")


_BUILT = {}


def built(name, extra_power, tmp_path_factory):
    """-> (Circuit, paths, the objects SetupFromPtau returned); one setup per (shape, power) and session"""
    key = (name, extra_power)
    if key not in _BUILT:
        k, npub, nc = SHAPES[name]
        c = Circuit(k, npub, nc, 1000 + 10 * k + npub)
        d = tmp_path_factory.mktemp("setup_%s_%d" % key)
        paths = {n: str(d / n) for n in ("c.r1cs", "t.ptau", "c.zkey")}
        c.write_r1cs(paths["c.r1cs"])
        circom.WritePtau(paths["t.ptau"], k + extra_power, c.tau, c.alpha, c.beta)
        _BUILT[key] = (c, paths, circom.SetupFromPtau(paths["c.r1cs"], paths["t.ptau"], paths["c.zkey"]))
    return _BUILT[key]


def g1_rows(scalars):
    return capi.g1_download(capi.g1_fixed_base(CU.u64(scalars)))


def section_rows(buf, g2=False):
    """a .zkey section through the existing upload and download"""
    return capi.g2_download(capi.g2_upload_affine_mont(buf)) if g2 else capi.g1_download(capi.g1_upload_affine_mont(buf))


def g1_point(k):
    x, y = C.g1_affine(C.g1_mul_scalar(O.G1_GEN, k))
    return (x, y, 1)


def g2_point(k):
    p = C.g2_affine(C.g2_mul_scalar(O.G2_GEN, k))
    return (tuple(p[0]), tuple(p[1]), (1, 0))


@pytest.mark.parametrize("extra_power", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_setup_sections_have_their_closed_forms(name, extra_power, tmp_path_factory):
    c, paths, _ = built(name, extra_power, tmp_path_factory)
    z = circom.ReadZkey(paths["c.zkey"])
    assert (z.nVars, z.nPublic, z.domainSize) == (c.nvars, c.npub, c.m)
    assert z.alfa1 == g1_point(c.alpha) and z.beta1 == g1_point(c.beta) and z.delta1 == g1_point(1)
    norm2 = lambda p: tuple(tuple(int(v) for v in q) for q in p)              # noqa: E731
    assert norm2(z.beta2) == g2_point(c.beta) and norm2(z.gamma2) == g2_point(1) and norm2(z.delta2) == g2_point(1)
    assert np.array_equal(section_rows(z.A), g1_rows(c.at))
    assert np.array_equal(section_rows(z.B1), g1_rows(c.bt))
    assert np.array_equal(section_rows(z.B2, True), capi.g2_download(capi.g2_fixed_base(CU.u64(c.bt))))
    assert np.array_equal(section_rows(z.IC), g1_rows(c.kk[:c.npub + 1]))
    assert np.array_equal(section_rows(z.C), g1_rows(c.kk[c.npub + 1:]))
    h = c.h_scalars(with_last=extra_power > 0)
    if c.k <= 3:
        assert h == c.h_scalars_by_definition(with_last=extra_power > 0)
        assert h != c.h_scalars(with_last=extra_power == 0)
    assert np.array_equal(section_rows(z.H), g1_rows(h))
    rec = z.coefs.reshape(-1, circom.COEF_BYTES)
    got = [struct.unpack("<III", bytes(x[:12])) + (int.from_bytes(bytes(x[12:]), "little"),) for x in rec]
    assert got == c.expected_records()


@pytest.mark.parametrize("name", list(SHAPES))
def test_proving_with_the_new_key(name, tmp_path_factory):
    c, paths, (key0, sys0, vk0) = built(name, 0, tmp_path_factory)
    key, system = circom.UploadZkey(paths["c.zkey"])
    vk = circom.VerificationKeyFromZkey(paths["c.zkey"])
    public = c.w[1:c.npub + 1]
    rng = random.Random(5)
    for policy in ("always", "never"):
        capi.set_table_policy(policy)
        r, s = rng.randrange(R), rng.randrange(R)
        proof = circom.GenerateProofsWithRS(key, system, c.w, r, s)
        CU.assert_closed_form(proof, c.proof_scalars(c.w, r, s))
        assert circom.VerifyFromCircom(vk, proof, public) and groth16.VerifyProof(vk0, proof, public)
        assert CU.words(circom.GenerateProofsWithRS(key0, sys0, c.w, r, s)) == CU.words(proof)
    wrong = list(c.w)
    wrong[-1] = (wrong[-1] + 1) % R
    assert not circom.VerifyFromCircom(vk, circom.GenerateProofsWithRS(key, system, wrong, 3, 4), public)
    if c.npub:
        assert not circom.VerifyFromCircom(vk, proof, [(public[0] + 1) % R] + public[1:])


def test_contribution(tmp_path_factory):
    c, paths, _ = built("k3", 1, tmp_path_factory)
    delta = random.Random(9).randrange(2, R)
    dinv = pow(delta, -1, R)
    out = paths["c.zkey"] + ".contributed"
    circom.ContributeDelta(paths["c.zkey"], out, delta)
    z0, z1 = circom.ReadZkey(paths["c.zkey"]), circom.ReadZkey(out)
    assert np.array_equal(section_rows(z1.C), g1_rows([x * dinv % R for x in c.kk[c.npub + 1:]]))
    assert np.array_equal(section_rows(z1.H), g1_rows([x * dinv % R for x in c.h_scalars(True)]))
    assert z1.delta1 == g1_point(delta)
    assert tuple(tuple(int(v) for v in q) for q in z1.delta2) == g2_point(delta)
    b0, b1 = open(paths["c.zkey"], "rb").read(), open(out, "rb").read()
    assert len(b0) == len(b1)
    diff = np.nonzero(np.frombuffer(b0, dtype=np.uint8) != np.frombuffer(b1, dtype=np.uint8))[0]
    data, sec = circom._read_sections(out, b"zkey", 1, circom._ZKEY_NAMES, (2, 8, 9))
    d1 = sec[2][0] + sec[2][1] - 192
    allowed = lambda i: d1 <= i < d1 + 192 or any(sec[s][0] <= i < sec[s][0] + sec[s][1] for s in (8, 9))      # noqa: E731
    assert diff.size and all(allowed(int(i)) for i in diff)
    for name in ("IC", "coefs", "A", "B1", "B2"):
        assert np.array_equal(getattr(z0, name), getattr(z1, name))
    assert (z0.alfa1, z0.beta1, z0.beta2, z0.gamma2) == (z1.alfa1, z1.beta1, z1.beta2, z1.gamma2)
    key, system = circom.UploadZkey(out)
    vk_new, vk_old = circom.VerificationKeyFromZkey(z1), circom.VerificationKeyFromZkey(z0)
    public = c.w[1:c.npub + 1]
    proof = circom.GenerateProofsWithRS(key, system, c.w, 11, 12)
    CU.assert_closed_form(proof, c.proof_scalars(c.w, 11, 12, delta))
    assert circom.VerifyFromCircom(vk_new, proof, public) and not circom.VerifyFromCircom(vk_old, proof, public)
    with pytest.raises(ValueError, match="delta"):
        circom.ContributeDelta(paths["c.zkey"], out, R)


@pytest.mark.parametrize("n", [1, 63, 65])
def test_download_round_trip(n):
    rng = random.Random(n)
    ks = [rng.randrange(1, R) for _ in range(n)]
    ks[n // 2] = 0
    if n > 2:
        ks[0] = ks[n - 1] = 0
    for g2 in (False, True):
        fixed = (capi.g2_fixed_base if g2 else capi.g1_fixed_base)(CU.u64(ks))
        pts = (capi.g2_tuples(capi.g2_download(fixed)) if g2 else capi.g1_tuples(capi.g1_download(fixed)))
        data = np.frombuffer(b"".join((circom.G2ToZkey if g2 else circom.G1ToZkey)(p) for p in pts), dtype=np.uint8)
        up = (capi.g2_upload_affine_mont if g2 else capi.g1_upload_affine_mont)(data)
        down = (capi.g2_download_affine_mont if g2 else capi.g1_download_affine_mont)
        assert np.array_equal(down(up), data)
        assert np.array_equal(down(fixed), data)
        size = 128 if g2 else 64
        assert np.array_equal(down(up, n=n // 2), data[:(n // 2) * size])
        with pytest.raises(capi.GosnarkHipError, match="were asked for"):
            down(up, out=np.zeros((n + 1) * size, dtype=np.uint8), n=n + 1)
