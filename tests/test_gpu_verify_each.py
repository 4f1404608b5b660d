"""-m gpu: gs_groth16_verify_each / groth16.VerifyProofsEach -- a verdict per proof of a batch under one key, on the device.

Proofs of the committed x^3 + x + 5 key (wasm_groth_x3.json) from the device prover, one witness x = 3 + i and one (r, s) per proof, as
in test_gpu_verify_batch.py (built again here).  The yardstick is the host verifier, one proof at a time: every changed position must
get the host's verdict and every other position must stay True.  Sizes 1, 2, 65, 130: both sides of the one-wave workgroup seam.
Keys with 0 and 3 public inputs are made from known discrete logs: A = a G1, B = b G2, C = ((ab - alpha beta - gamma vkx) / delta) G1."""
import ctypes
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16, utils
import golden_util as GU
import membership_util as M
import multikey_util as MK
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R, Q = O.R, O.Q
NMAX = 130
SIZES = [1, 2, 65, 130]


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
    rng = random.Random(78)
    proofs, pubs = [], []
    for i in range(NMAX):
        x = 3 + i
        out = x ** 3 + x + 5
        w = [1, out, x, x * x, x ** 3, x ** 3 + x, out, 1]
        px = O.PF.CombinePolynomials(w, al, be, ga)[3]
        proofs.append(groth16.GenerateProofsWithRS(circ, pk, w, px, rng.randrange(1, R), rng.randrange(1, R)))
        pubs.append([out])
    assert all(groth16.VerifyProof(vk, p, s) for p, s in zip(proofs[:3], pubs[:3]))
    assert not groth16.VerifyProof(vk, proofs[0], pubs[1])
    return vk, proofs, pubs


def agree(vk, proofs, pubs, changed, expect_false=True):
    """The device's verdicts against the host's at the changed positions and True everywhere else; returns them."""
    got = groth16.VerifyProofsEach(vk, proofs, pubs)
    assert len(got) == len(proofs)
    for i in range(len(proofs)):
        if i in changed:
            host = groth16.VerifyProof(vk, proofs[i], pubs[i])
            assert got[i] == host, i
            if expect_false:
                assert got[i] is False, i
        else:
            assert got[i] is True, i
    return got


def g1_mul(k):
    return O.G1.MulScalar(O.G1_GEN, k % R)


def g1_add(p, q):
    return O.G1.Add(p, q)


@pytest.mark.parametrize("n", SIZES)
def test_valid_batches_get_true_everywhere(batch, n):
    vk, base, pubs = batch
    assert groth16.VerifyProofsEach(vk, base[:n], pubs[:n]) == [True] * n


@pytest.mark.parametrize("n", SIZES)
def test_exactly_the_tampered_positions_get_false(batch, n):
    vk, base, pubs = batch
    other_b = O.G2.MulScalar(O.G2_GEN, 12345)
    spots = sorted({0, n // 2, n - 1})
    kinds = ("A", "B", "C", "public")
    for shift in range(len(kinds)):                                     # every kind of change visits every position
        proofs, signals = list(base[:n]), [list(s) for s in pubs[:n]]
        for k, at in enumerate(spots):
            p, what = base[at], kinds[(k + shift) % len(kinds)]
            if what == "A":
                proofs[at] = groth16.Proof(g1_add(p.PiA, O.G1_GEN), p.PiB, p.PiC)
            elif what == "B":
                proofs[at] = groth16.Proof(p.PiA, other_b, p.PiC)
            elif what == "C":
                proofs[at] = groth16.Proof(p.PiA, p.PiB, g1_add(p.PiC, O.G1_GEN))
            else:
                signals[at][0] += 1
        agree(vk, proofs, signals, set(spots))


def test_the_compensating_pair_gets_false_twice(batch):
    vk, base, pubs = batch
    d = g1_mul(random.Random(3).randrange(1, R))
    for n, (i, j) in ((2, (0, 1)), (130, (64, 129))):
        proofs = list(base[:n])
        proofs[i] = groth16.Proof(base[i].PiA, base[i].PiB, g1_add(base[i].PiC, d))
        proofs[j] = groth16.Proof(base[j].PiA, base[j].PiB, g1_add(base[j].PiC, O.G1.Neg(d)))
        agree(vk, proofs, pubs[:n], {i, j})


def test_infinite_and_outside_points_and_several_bad_proofs(batch):
    vk, base, pubs = batch
    n = 130
    proofs, signals = list(base[:n]), [list(s) for s in pubs[:n]]
    proofs[7] = groth16.Proof(O.G1_ZERO, base[7].PiB, base[7].PiC)                              # an infinite A
    x, y, z = base[64].PiA
    proofs[64] = groth16.Proof((x, (y + 1) % Q, z), base[64].PiB, base[64].PiC)                # an A off the curve: 0, not an error
    for at, b in ((0, M.twist_points(1)[0]), (65, M.complete_add(M.jac(O.G2.Affine(base[65].PiB)), M.small_order_point()))):
        assert not M.in_subgroup(b)
        proofs[at] = groth16.Proof(base[at].PiA, b, base[at].PiC)                              # a B on the twist outside G2
    signals[3], signals[129] = signals[129], signals[3]                                       # swapped publics
    proofs[63] = groth16.Proof(base[63].PiA, base[63].PiB, O.G1_ZERO)                           # an infinite C
    proofs[20] = groth16.Proof(base[21].PiA, base[20].PiB, base[20].PiC)                       # several in one wave and across two
    proofs[100] = groth16.Proof(base[100].PiA, base[101].PiB, base[100].PiC)
    agree(vk, proofs, signals, {7, 64, 0, 65, 3, 129, 63, 20, 100})


def _raw_call(vk, proofs, pubs, nbad=True):
    npublic = len(pubs[0]) if pubs else 0
    ic, nic, _, _ = groth16._scheme.verify_inputs(vk, [0] * npublic)
    g1 = capi.g1_points_to_u64([vk.G1_Alpha])
    g2 = capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta])
    flat = [x for s in pubs for x in s]
    pub = capi.ints_to_u64(flat) if flat else np.zeros((1, 4), dtype=np.uint64)
    a, b, c = (capi.g1_points_to_u64([p.PiA for p in proofs]), capi.g2_points_to_u64([p.PiB for p in proofs]),
               capi.g1_points_to_u64([p.PiC for p in proofs]))
    ok, bad = np.full(len(proofs), 7, dtype=np.intc), ctypes.c_uint64(77)
    rc = capi.load_library().gs_groth16_verify_each(capi.ptr64(g1[0]), capi.ptr64(g2[0]), capi.ptr64(g2[1]), capi.ptr64(g2[2]), ic, nic, capi.ptr64(pub),
                                                    npublic, capi.ptr64(a), capi.ptr64(b), capi.ptr64(c), len(proofs), ok.ctypes.data_as(capi.intp),
                                                    ctypes.byref(bad) if nbad else None)
    return rc, [int(x) for x in ok], bad.value


def test_strict_mode_the_count_and_balanced_allocations(batch):
    vk, base, pubs = batch
    n = 65
    lib = capi.load_library()
    assert _raw_call(vk, base[:n], pubs[:n]) == (0, [1] * n, 0)
    before = capi.alloc_counters()
    x, y, z = base[9].PiA
    aliased = list(base[:n])
    aliased[9] = groth16.Proof((x + Q, y, z), base[9].PiB, base[9].PiC)
    noncanon = [list(s) for s in pubs[:n]]
    noncanon[64][0] += R
    assert _raw_call(vk, aliased, noncanon) == (0, [1] * n, 0)           # the reference's big.Int behaviour: X + q names the same point
    assert groth16.VerifyProof(vk, aliased[9], pubs[9])
    try:
        assert lib.gs_verify_set_strict(1) == 0
        assert _raw_call(vk, base[:n], pubs[:n]) == (0, [1] * n, 0)
        want = [0 if i in (9, 64) else 1 for i in range(n)]
        assert _raw_call(vk, aliased, noncanon) == (0, want, 2)
        assert not groth16.VerifyProof(vk, aliased[9], pubs[9])
    finally:
        lib.gs_verify_set_strict(0)
    rc, ok, _ = _raw_call(vk, aliased, noncanon, nbad=False)
    assert rc == 0 and ok == [1] * n
    ax, ay, az = vk.G1_Alpha
    bad_key = groth16.Vk(IC=vk.IC, G1_Alpha=(ax, (ay + 1) % Q, az), G2_Beta=vk.G2_Beta, G2_Gamma=vk.G2_Gamma, G2_Delta=vk.G2_Delta)
    assert _raw_call(bad_key, base[:n], pubs[:n]) == (0, [0] * n, n)    # a key point off its curve: every verdict 0
    assert not groth16.VerifyProof(bad_key, base[0], pubs[0])
    ix, iy, iz = vk.IC[1]
    bad_key = groth16.Vk(IC=[vk.IC[0], (ix, (iy + 1) % Q, iz)], G1_Alpha=vk.G1_Alpha, G2_Beta=vk.G2_Beta, G2_Gamma=vk.G2_Gamma, G2_Delta=vk.G2_Delta)
    assert _raw_call(bad_key, base[:n], pubs[:n]) == (0, [0] * n, n)
    assert not groth16.VerifyProof(bad_key, base[0], pubs[0])
    after = capi.alloc_counters()
    assert after[0] - before[0] == after[1] - before[1]                 # every temporary array is freed on every path


def dlog_batch(npublic, n, seed):
    """A key with npublic inputs and n proofs from known discrete logs; every odd proof is perturbed.  -> vk, proofs, signals"""
    rng = random.Random(seed)
    alpha, beta, gamma, delta = (rng.randrange(1, R) for _ in range(4))
    ics = [rng.randrange(1, R) for _ in range(npublic + 1)]
    g2 = lambda k: O.G2.MulScalar(O.G2_GEN, k % R)   # noqa: E731
    vk = groth16.Vk(IC=[g1_mul(k) for k in ics], G1_Alpha=g1_mul(alpha), G2_Beta=g2(beta), G2_Gamma=g2(gamma), G2_Delta=g2(delta))
    proofs, signals = [], []
    for i in range(n):
        a, b = rng.randrange(1, R), rng.randrange(1, R)
        sig = [rng.choice((0, 1, R - 1, rng.randrange(R))) for _ in range(npublic)]
        vkx = (ics[0] + sum(s * k for s, k in zip(sig, ics[1:]))) % R
        c = (a * b - alpha * beta - gamma * vkx) * pow(delta, R - 2, R) % R
        if i % 2:
            what = rng.randrange(3 if npublic else 2)
            if what == 0:
                a += 1
            elif what == 1:
                c += 1
            else:
                sig[rng.randrange(npublic)] += 1
        proofs.append(groth16.Proof(g1_mul(a), g2(b), g1_mul(c)))
        signals.append(sig)
    return vk, proofs, signals


@pytest.mark.parametrize("npublic", [0, 3])
def test_keys_with_0_and_3_public_inputs_from_known_discrete_logs(npublic):
    n = 66
    vk, proofs, signals = dlog_batch(npublic, n, 500 + npublic)
    host = [groth16.VerifyProof(vk, p, s) for p, s in zip(proofs, signals)]
    assert host == [i % 2 == 0 for i in range(n)]                       # the construction accepts, the perturbation does not
    assert groth16.VerifyProofsEach(vk, proofs, signals) == host


@pytest.mark.parametrize("which", ["gamma", "delta"])
def test_an_infinite_gamma_or_delta_in_one_full_group_and_two_lanes(which):
    """The key's skip flags travel in the call's key record: 66 proofs, one change of every kind on both sides of the group seam.  With an
    infinite gamma the signals, with an infinite delta C, do not enter the product: the host verifier says what such a change does."""
    d = MK.DlogKey(1, 620 + len(which), gamma_infinite=which == "gamma", delta_infinite=which == "delta")
    proofs, signals = d.proofs(66)
    changed = {0: "A", 63: "B", 64: "C", 65: "public"}
    for at, what in changed.items():
        proofs[at], signals[at] = MK.tamper(proofs[at], signals[at], what)
    before = capi.alloc_counters()
    got = agree(d.vk, proofs, signals, set(changed), expect_false=False)
    after = capi.alloc_counters()
    assert got[0] is False and got[63] is False                         # A and B enter the product whatever the key is
    assert after[0] - before[0] == after[1] - before[1]                 # the key made for the call leaves nothing behind


def test_fewer_signals_than_ic_points_outside_strict_mode():
    """npublic = 2 under a key with four IC points: the call's key record carries the call's count, not the key's.  The yardstick is
    gs_groth16_verify with the same two signals, which reads the missing third one as 0."""
    d = MK.DlogKey(3, 640)
    n = 65
    both = [d.proof(sig=[d.rng.randrange(R), d.rng.randrange(R), 0]) for _ in range(n)]
    proofs, pubs = [p for p, _ in both], [s[:2] for _, s in both]
    for at, what in ((0, "A"), (64, "public")):
        proofs[at], pubs[at] = MK.tamper(proofs[at], pubs[at], what)
    host = [groth16.VerifyProof(d.vk, p, s) for p, s in zip(proofs, pubs)]
    assert host == [i not in (0, 64) for i in range(n)]
    lib = capi.load_library()
    before = capi.alloc_counters()
    assert _raw_call(d.vk, proofs, pubs) == (0, [int(h) for h in host], 2)
    try:
        assert lib.gs_verify_set_strict(1) == 0
        assert _raw_call(d.vk, proofs, pubs) == (-4, [7] * n, 77)       # GS_ERR_SHAPE, nothing written
        assert b"exactly 3 public signals" in lib.gs_last_error()
    finally:
        lib.gs_verify_set_strict(0)
    dx, dy, dz = d.vk.G2_Delta
    bad_key = groth16.Vk(IC=d.vk.IC, G1_Alpha=d.vk.G1_Alpha, G2_Beta=d.vk.G2_Beta, G2_Gamma=d.vk.G2_Gamma, G2_Delta=(dx, (dy[0], (dy[1] + 1) % Q), dz))
    assert not groth16.VerifyProof(bad_key, proofs[1], pubs[1])
    assert _raw_call(bad_key, proofs, pubs) == (0, [0] * n, n)           # a key point off its curve: every verdict 0
    after = capi.alloc_counters()
    assert after[0] - before[0] == after[1] - before[1]


def test_ragged_input_raises_like_verify_proofs(batch):
    vk, base, pubs = batch
    with pytest.raises(ValueError):
        groth16.VerifyProofsEach(vk, base[:2], pubs[:1])
    with pytest.raises(ValueError):
        groth16.VerifyProofsEach(vk, base[:2], [pubs[0], []])
    assert groth16.VerifyProofsEach(vk, [], []) == []
