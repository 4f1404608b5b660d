"""-m gpu: gs_groth16_verify_batch / groth16.VerifyProofs -- many proofs of one key in one randomised product check on the device.

Proofs of the committed x^3 + x + 5 key (wasm_groth_x3.json) from the device prover, one witness x = 3 + i and one (r, s) per proof.  For
every batch the device's answer must be all(VerifyProof(...)) computed one proof at a time on the host.  Sizes 1, 2, 65, 130: one pair,
two, and both sides of the 64-lane workgroup seam of the Miller kernel with a partial product on top."""
import ctypes
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16, utils
import golden_util as GU
import membership_util as M
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R, Q = O.R, O.Q
NMAX = 130
SIZES = [1, 2, 65, 130]
SEED = 20240


@pytest.fixture(autouse=True)
def _init():
    capi.init()


@pytest.fixture(scope="module")
def batch():
    """(vk, proofs, public signal lists): NMAX valid proofs, each accepted by the host verifier for its own public input."""
    capi.init()
    rec = GU.load("groth_x3")
    opk = GU.groth_pk(rec["setup"])
    _, vk = utils.GrothSetupFromString(rec["setup"])
    circ = groth16.Circuit(rec["circuit"]["NVars"], rec["circuit"]["NPublic"])
    pk = groth16.Pk(BACDelta=opk.BACDelta, Z=opk.Z, G1_Alpha=opk.G1_Alpha, G1_Beta=opk.G1_Beta, G1_Delta=opk.G1_Delta,
                    G1_At=opk.G1_At, G1_BACGamma=opk.G1_BACGamma, G2_Beta=opk.G2_Beta, G2_Delta=opk.G2_Delta,
                    G2_BACGamma=opk.G2_BACGamma, PowersTauDelta=opk.PowersTauDelta)
    al, be, ga, _ = O.PF.R1CSToQAP(O.X3_R1CS_A, O.X3_R1CS_B, O.X3_R1CS_C)
    rng = random.Random(77)
    proofs, pubs = [], []
    for i in range(NMAX):
        x = 3 + i
        out = x ** 3 + x + 5
        w = [1, out, x, x * x, x ** 3, x ** 3 + x, out, 1]
        px = O.PF.CombinePolynomials(w, al, be, ga)[3]
        proofs.append(groth16.GenerateProofsWithRS(circ, pk, w, px, rng.randrange(1, R), rng.randrange(1, R)))
        pubs.append([out])
    assert all(groth16.VerifyProof(vk, p, s) for p, s in zip(proofs, pubs))
    assert not groth16.VerifyProof(vk, proofs[0], pubs[1])
    assert len({p.PiA for p in proofs}) == NMAX
    return vk, proofs, pubs


def agree(batch, n, changed=(), proofs=None, pubs=None):
    """The device's verdict on the first n proofs (some replaced) against the host's, one proof at a time; returns it."""
    vk, base_proofs, base_pubs = batch
    proofs = list(base_proofs[:n]) if proofs is None else proofs
    pubs = list(base_pubs[:n]) if pubs is None else pubs
    host = all(groth16.VerifyProof(vk, proofs[i], pubs[i]) for i in changed)      # the others are the fixture's, accepted there
    got = groth16.VerifyProofs(vk, proofs, pubs, seed=SEED)
    assert got == host, (n, changed)
    return got


def g1_mul(k):
    return O.G1.MulScalar(O.G1_GEN, k % R)


def g1_add(p, q):
    return O.G1.Add(p, q)


@pytest.mark.parametrize("n", SIZES)
def test_valid_batches_are_accepted(batch, n):
    assert agree(batch, n) is True


@pytest.mark.parametrize("n", SIZES)
def test_one_tampered_proof_rejects_the_batch(batch, n):
    vk, base, pubs = batch
    other_b = O.G2.MulScalar(O.G2_GEN, 12345)
    for at in sorted({0, n // 2, n - 1}):
        p = base[at]
        for what, bad in (("A", groth16.Proof(g1_add(p.PiA, O.G1_GEN), p.PiB, p.PiC)), ("B", groth16.Proof(p.PiA, other_b, p.PiC)),
                          ("C", groth16.Proof(p.PiA, p.PiB, g1_add(p.PiC, O.G1_GEN)))):
            proofs = list(base[:n])
            proofs[at] = bad
            assert agree(batch, n, [at], proofs=proofs) is False, (what, at)
        signals = [list(s) for s in pubs[:n]]
        signals[at][0] += 1
        assert agree(batch, n, [at], pubs=signals) is False, ("public", at)


def test_swapped_publics_an_infinite_a_and_points_outside(batch):
    vk, base, pubs = batch
    n = 65
    signals = [list(s) for s in pubs[:n]]
    signals[3], signals[64] = signals[64], signals[3]
    assert agree(batch, n, [3, 64], pubs=signals) is False
    proofs = list(base[:n])
    proofs[7] = groth16.Proof(O.G1_ZERO, base[7].PiB, base[7].PiC)
    assert agree(batch, n, [7], proofs=proofs) is False
    for at, b in ((0, M.twist_points(1)[0]), (64, M.complete_add(M.jac(O.G2.Affine(base[64].PiB)), M.small_order_point()))):
        assert not M.in_subgroup(b)
        proofs = list(base[:n])
        proofs[at] = groth16.Proof(base[at].PiA, b, base[at].PiC)
        assert agree(batch, n, [at], proofs=proofs) is False                                  # a B on the twist outside G2
    x, y, z = base[64].PiA
    proofs = list(base[:n])
    proofs[64] = groth16.Proof((x, (y + 1) % Q, z), base[64].PiB, base[64].PiC)
    assert agree(batch, n, [64], proofs=proofs) is False                                      # an A off the curve: 0, not an error


def test_the_compensating_pair_is_rejected(batch):
    """C_1 + D and C_2 - D leave the UNWEIGHTED sum of the C unchanged: only weights that differ per proof see it."""
    vk, base, pubs = batch
    d = g1_mul(random.Random(3).randrange(1, R))
    for n, (i, j) in ((2, (0, 1)), (130, (64, 129))):
        proofs = list(base[:n])
        proofs[i] = groth16.Proof(base[i].PiA, base[i].PiB, g1_add(base[i].PiC, d))
        proofs[j] = groth16.Proof(base[j].PiA, base[j].PiB, g1_add(base[j].PiC, O.G1.Neg(d)))
        assert O.G1.Affine(g1_add(proofs[i].PiC, proofs[j].PiC)) == O.G1.Affine(g1_add(base[i].PiC, base[j].PiC))
        assert agree(batch, n, [i, j], proofs=proofs) is False


def _raw_call(vk, proofs, pubs, challenge):
    ic, nic, _, _ = groth16._scheme.verify_inputs(vk, [0] * len(pubs[0]))
    g1 = capi.g1_points_to_u64([vk.G1_Alpha])
    g2 = capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta])
    pub = capi.ints_to_u64([x for s in pubs for x in s])
    a, b, c = (capi.g1_points_to_u64([p.PiA for p in proofs]), capi.g2_points_to_u64([p.PiB for p in proofs]),
               capi.g1_points_to_u64([p.PiC for p in proofs]))
    ok = ctypes.c_int(7)
    rc = capi.load_library().gs_groth16_verify_batch(capi.ptr64(g1[0]), capi.ptr64(g2[0]), capi.ptr64(g2[1]), capi.ptr64(g2[2]), ic, nic, capi.ptr64(pub),
                                                     len(pubs[0]), capi.ptr64(a), capi.ptr64(b), capi.ptr64(c), len(proofs),
                                                     capi.ptr64(capi.ints_to_u64([challenge])), ctypes.byref(ok))
    return rc, ok.value


def test_constant_challenges_strict_mode_and_balanced_allocations(batch):
    vk, base, pubs = batch
    n = 65
    lib = capi.load_library()
    assert _raw_call(vk, base[:n], pubs[:n], 12345) == (0, 1)
    before = capi.alloc_counters()
    for challenge in (0, 1, R, R + 1):
        assert _raw_call(vk, base[:n], pubs[:n], challenge) == (-3, 7)
        assert b"gs_groth16_verify_batch" in lib.gs_last_error()
    assert _raw_call(vk, base[:n], pubs[:n], R + 2) == (0, 1)
    x, y, z = base[9].PiA
    aliased = list(base[:n])
    aliased[9] = groth16.Proof((x + Q, y, z), base[9].PiB, base[9].PiC)
    assert _raw_call(vk, aliased, pubs[:n], 12345) == (0, 1)             # the reference's big.Int behaviour: X + q names the same point
    assert groth16.VerifyProof(vk, aliased[9], pubs[9])
    try:
        assert lib.gs_verify_set_strict(1) == 0
        assert _raw_call(vk, base[:n], pubs[:n], 12345) == (0, 1)
        assert _raw_call(vk, aliased, pubs[:n], 12345) == (0, 0)
        assert not groth16.VerifyProof(vk, aliased[9], pubs[9])
    finally:
        lib.gs_verify_set_strict(0)
    off = list(base[:n])
    off[0] = groth16.Proof((x, (y + 1) % Q, z), base[0].PiB, base[0].PiC)
    assert _raw_call(vk, off, pubs[:n], 12345) == (0, 0)
    outside = list(base[:n])
    outside[1] = groth16.Proof(base[1].PiA, M.twist_points(1)[0], base[1].PiC)
    assert _raw_call(vk, outside, pubs[:n], 12345) == (0, 0)
    after = capi.alloc_counters()
    assert after[0] - before[0] == after[1] - before[1]                 # every temporary array is freed on every path
