"""-m gpu: proving with snarkjs / circom Groth16 keys -- the QAP over a power-of-two domain (csrc/domain.h), Z = x^m - 1.

The reference's own fixture (externalVerif/circom-test, the multiplier over a domain of 4 points) proves bit for bit the same on every
route and the proofs verify against the recorded verification key; synthetic instances over domains 2^1 .. 2^15, whose keys are built
from toxic values (tests/circom_util.py), pin the transforms' seams, the coset evaluation-basis array itself, raw witness words,
violated witnesses and the refusals, all against closed forms in the generators."""
import ctypes
import functools
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom, groth16, r1csqap, snark
import circom_util as CU
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = CU.R
GS_ERR_ARG, GS_ERR_SHAPE = -3, -4


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)
    yield
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)


def prove_blocking(dev, w, px, r, s):
    """gs_groth16_prove: w and px from the host, blocking"""
    wa, pa = CU.u64(w), CU.u64(px)
    rs = capi.ints_to_u64([r % R, s % R])
    out = np.zeros(32, dtype=np.uint64)
    inf = (ctypes.c_int * 3)()
    capi.check(capi.load_library().gs_groth16_prove(capi.Handle(dev.handle.h), capi.ptr64(wa), wa.shape[0], capi.ptr64(pa), pa.shape[0],
                                                    capi.ptr64(rs[0]), capi.ptr64(rs[1]), capi.ptr64(out), inf))
    return groth16._proof_from_words(out, inf)


def rs_pairs(seed, count=2):
    rng = random.Random(seed)
    return [(rng.randrange(R), rng.randrange(R)) for _ in range(count)]


# ---- 4. the fixture key, every route, bit for bit -----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def fixture_parts():
    pkj = circom.ParseProvingKey(CU.fixture_json("proving_key"))
    w = circom.ParseWitness(CU.fixture_json("witness"))
    px = CU.px_naive(pkj.rows_a, pkj.rows_b, pkj.rows_c, w, pkj.domainBits)
    opk = O.GrothPk()
    opk.G1_At, opk.G1_BACGamma, opk.G2_BACGamma, opk.BACDelta, opk.PowersTauDelta, opk.Z = pkj.A, pkj.B1, pkj.B2, pkj.C, pkj.hExps, pkj.Z()
    opk.G1_Alpha, opk.G1_Beta, opk.G1_Delta, opk.G2_Beta, opk.G2_Delta = pkj.alfa1, pkj.beta1, pkj.delta1, pkj.beta2, pkj.delta2
    return pkj, w, px, opk


@functools.lru_cache(maxsize=None)
def fixture_oracle_proof(r, s):
    pkj, w, px, opk = fixture_parts()
    a, b, c = O.groth16_GenerateProofs(pkj.nVars, pkj.nPublic, opk, w, px, r, s)
    aa, bb, cc = O.G1.Affine(a), O.G2.Affine(b), O.G1.Affine(c)
    return ((aa[0], aa[1], 1), (bb[0], bb[1], (1, 0)), (cc[0], cc[1], 1))


@pytest.mark.parametrize("policy", ["always", "never"])
def test_fixture_key_proves_the_same_on_every_route_and_verifies(policy):
    capi.set_table_policy(policy)
    pkj, w, px, _ = fixture_parts()
    assert len(px) == 2 * pkj.domainSize - 1
    vk = CU.fixture_json("verification_key")
    dev, r1cs = circom.UploadProvingKey(pkj)
    dev_e, r1cs_e = circom.UploadProvingKey(pkj)
    circom.DeriveEvalBasis(dev_e, pkj.domainBits)
    assert capi.pk_eval_count(dev.handle) == 0 and capi.pk_eval_count(dev_e.handle) == pkj.domainSize
    wh = capi.scalars_upload(CU.u64(w))
    for r, s in [(0, 0), (1, 0)] + rs_pairs(20):
        want = fixture_oracle_proof(r, s)
        routes = {
            "prove(px)": prove_blocking(dev, w, px, r, s),
            "prove_r1cs": groth16.prove_from_r1cs(dev, r1cs, wh, r, s)[0],
            "witness, no E": groth16.prove_from_witness(dev, r1cs, wh, r, s),
            "witness, E": groth16.prove_from_witness(dev_e, r1cs_e, wh, r, s),
            "resident ticket": groth16.prove_end(groth16.prove_witness_begin(dev_e, r1cs_e, wh, r, s)),
            "host ticket": groth16.prove_end(groth16.prove_witness_host_begin(dev_e, r1cs_e, w, r, s)),
            "host ticket, no E": groth16.prove_end(groth16.prove_witness_host_begin(dev, r1cs, w, r, s)),
            "circom.GenerateProofs": circom.GenerateProofs(dev_e, r1cs_e, w, r, s),
        }
        for name, got in routes.items():
            assert CU.words(got) == want, (name, r, s)
        assert capi.last_timing()["fallbacks"] == 0
        proof = routes["witness, E"]
        assert circom.VerifyFromCircom(vk, proof, [33]) is True
        assert circom.VerifyFromCircom(vk, proof, [34]) is False
        assert circom.VerifyFromCircom(vk, circom.ProofToJSON(proof), ["33"]) is True
    # the resident px of the domain system is the one computed above
    pxh = r1cs.ComputePxResident(wh)
    assert capi.u64_to_ints(capi.scalars_download(pxh)) == px


def test_binary_container_carries_the_coset_basis(tmp_path):
    pkj, w, _, _ = fixture_parts()
    dev, r1cs = circom.UploadProvingKey(pkj)
    circom.DeriveEvalBasis(dev, pkj.domainBits)
    e = groth16.ExportPkArray(dev, "PowersTauDeltaEval")
    path = str(tmp_path / "key.bin")
    circom.ProvingKeyToBinary(path, pkj, e)
    dev2, r1cs2 = circom.UploadProvingKeyBinary(path)
    assert groth16.ExportPkArray(dev2, "PowersTauDeltaEval") == e
    r, s = rs_pairs(21, 1)[0]
    assert CU.words(circom.GenerateProofs(dev2, r1cs2, w, r, s)) == fixture_oracle_proof(r, s)


# ---- synthetic instances -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def instance(k, n, seed=1, tau=None):
    return CU.Instance(k, n, seed, tau)


def both_routes(inst, dev, r1cs, wh, w, r, s):
    """the E route and the px route of one witness: equal to each other (returned once) -- the key holds the array"""
    capi.set_eval_basis(True)
    e = groth16.prove_from_witness(dev, r1cs, wh, r, s)
    assert capi.last_timing()["fallbacks"] == 0
    capi.set_eval_basis(False)
    p = groth16.prove_from_witness(dev, r1cs, wh, r, s)
    capi.set_eval_basis(True)
    assert CU.words(e) == CU.words(p)
    return e


# ---- 5. the seams of the transforms ------------------------------------------------------------------------------------------
# below one pass, exactly one 7-stage pass, pass + 1, a full 1024 tile, tile + 1, exactly two passes, three passes; full and ragged n
@pytest.mark.parametrize("k,short", [(1, 0), (2, 1), (3, 3), (7, 0), (8, 3), (10, 3), (11, 0), (14, 3), (15, 0)])
def test_transform_seams_on_both_routes_equal_the_closed_form(k, short):
    m = 1 << k
    inst = instance(k, m - short)
    dev, r1cs = inst.upload()
    circom.DeriveEvalBasis(dev, k)
    wh = capi.scalars_upload(CU.u64(inst.w))
    r, s = rs_pairs(50 + k, 1)[0]
    got = both_routes(inst, dev, r1cs, wh, inst.w, r, s)
    CU.assert_closed_form(got, inst.expected_scalars(inst.w, r, s))
    via_px = groth16.prove_from_r1cs(dev, r1cs, wh, r, s)[0]
    assert CU.words(via_px) == CU.words(got)
    if k in (10, 11):                                       # three tickets in flight, distinct witnesses (the input differs)
        ws, tickets = [], []
        for i in range(3):
            rng = random.Random(900 + i)
            w = [1, rng.randrange(2, R)]
            for c in range(inst.n):
                dot = lambda row: sum(v * w[x] for x, v in row.items()) % R       # noqa: E731
                w.append(dot(inst.rows_a[c]) * dot(inst.rows_b[c]) % R)
            ws.append(w)
        handles = [capi.scalars_upload(CU.u64(w)) for w in ws]
        pairs = rs_pairs(70 + k, 3)
        for h, (rr, ss) in zip(handles, pairs):
            tickets.append(groth16.prove_witness_begin(dev, r1cs, h, rr, ss))
        for t, w, (rr, ss) in zip(tickets, ws, pairs):
            CU.assert_closed_form(groth16.prove_end(t), inst.expected_scalars(w, rr, ss))
        assert capi.last_timing()["fallbacks"] == 0


# ---- 6. the coset evaluation-basis array itself ------------------------------------------------------------------------------
def g1_multiples(ks):
    """k G as affine (x, y, 1) / (0, 0, 0), from the oracle"""
    out = []
    for k in ks:
        a = C.g1_affine(C.g1_mul_scalar(O.G1_GEN, k)) if k % R else None
        out.append((0, 0, 0) if a is None else (a[0], a[1], 1))
    return out


def naive_eval_basis(hexps_scalars, k):
    """E_j = -(1/(2m)) sum_i y_j^(-i) T_i on the scalars t_i of T_i = t_i G (the definition, O(m^2))"""
    m, g, w = 1 << k, CU.coset_gen(k), CU.omega(k)
    f = (-pow(2 * m, -1, R)) % R
    out = []
    for j in range(m):
        yi = pow(g * pow(w, j, R) % R, -1, R)
        out.append(f * sum(t * pow(yi, i, R) for i, t in enumerate(hexps_scalars[:m])) % R)
    return out


@pytest.mark.parametrize("k", [1, 2, 3, 7, 8, 11])
def test_derived_coset_basis_equals_its_closed_form(k):
    m = 1 << k
    inst = instance(k, m)
    dev, _ = inst.upload()
    circom.DeriveEvalBasis(dev, k)
    got = groth16.ExportPkArray(dev, "PowersTauDeltaEval")
    want = inst.eval_basis_scalars()
    assert len(got) == m
    assert got == g1_multiples(want)
    if k <= 3:
        assert want == naive_eval_basis(inst.hexps, k)
    dev2, _ = inst.upload()
    assert capi.handle_bytes(dev.handle)[0] - capi.handle_bytes(dev2.handle)[0] >= m * 64      # accounted like the node basis: 64 B per point
    # set / export round trip
    circom.SetEvalBasis(dev2, got, k)
    assert groth16.ExportPkArray(dev2, "PowersTauDeltaEval") == got


@pytest.mark.parametrize("k", [2, 3, 7])
@pytest.mark.parametrize("kind", ["tau = 0", "tau^3 = 1"])
def test_derivation_survives_hostile_keys(k, kind):
    """tau = 0: every T_i but T_0 is infinity.  tau a primitive cube root of unity: T has period 3, so the butterflies meet P + P and
    P - P.  (Z(tau) != 0 in both: 3 does not divide m.)"""
    m = 1 << k
    tau = 0 if kind == "tau = 0" else pow(5, (R - 1) // 3, R)
    assert kind == "tau = 0" or (pow(tau, 3, R) == 1 and tau != 1)
    inst = CU.Instance(k, m, 3, tau=tau)
    assert inst.zt != 0
    dev, r1cs = inst.upload()
    circom.DeriveEvalBasis(dev, k)
    got = groth16.ExportPkArray(dev, "PowersTauDeltaEval")
    assert got == g1_multiples(naive_eval_basis(inst.hexps, k))
    wh = capi.scalars_upload(CU.u64(inst.w))
    r, s = rs_pairs(60 + k, 1)[0]
    CU.assert_closed_form(both_routes(inst, dev, r1cs, wh, inst.w, r, s), inst.expected_scalars(inst.w, r, s))


# ---- 7. witness words ------------------------------------------------------------------------------------------------------
def test_raw_witness_limbs_above_r_give_the_same_proof():
    k, m = 7, 128
    inst = instance(k, m - 3)
    dev, r1cs = inst.upload()
    circom.DeriveEvalBasis(dev, k)
    rng = random.Random(5)
    raw = [v + rng.randrange(1, 5) * R for v in inst.w]                       # in [r, 2^256): r < 2^254, so v + 4 r < 2^256
    raw[3] = (1 << 256) - 1 - (((1 << 256) - 1 - inst.w[3]) % R)             # the largest representative of w[3]
    assert all(R <= v < (1 << 256) and v % R == x for v, x in zip(raw, inst.w))
    raw_u64 = capi.ints_to_u64(raw)
    r, s = rs_pairs(77, 1)[0]
    wh, rh = capi.scalars_upload(CU.u64(inst.w)), capi.scalars_upload(raw_u64)
    want = both_routes(inst, dev, r1cs, wh, inst.w, r, s)
    CU.assert_closed_form(want, inst.expected_scalars(inst.w, r, s))
    assert CU.words(both_routes(inst, dev, r1cs, rh, raw, r, s)) == CU.words(want)
    assert CU.words(groth16.prove_end(groth16.prove_witness_host_begin(dev, r1cs, raw_u64, r, s))) == CU.words(want)
    assert CU.words(groth16.prove_from_witness_host(dev, r1cs, raw_u64, r, s)) == CU.words(want)


# ---- 8. violated witness ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 11])
def test_violated_witness_takes_the_exact_route(k):
    m = 1 << k
    inst = instance(k, m - 3 if k == 11 else m)
    dev, r1cs = inst.upload()
    circom.DeriveEvalBasis(dev, k)
    bad = list(inst.w)
    bad[2 + inst.n // 2] = (bad[2 + inst.n // 2] + 1) % R
    wh = capi.scalars_upload(CU.u64(bad))
    r, s = rs_pairs(80 + k, 1)[0]
    pxh = r1cs.ComputePxResident(wh)
    want = CU.words(groth16.prove_resident(dev, wh, pxh, r, s))                 # the floor quotient
    px = capi.u64_to_ints(capi.scalars_download(pxh))
    assert any(sum(px[i::m]) % R for i in range(m)), "px of a violated witness leaves a remainder mod x^m - 1"
    good = capi.scalars_upload(CU.u64(inst.w))
    groth16.prove_from_witness(dev, r1cs, good, r, s)
    assert capi.last_timing()["fallbacks"] == 0
    assert CU.words(groth16.prove_from_witness(dev, r1cs, wh, r, s)) == want
    assert capi.last_timing()["fallbacks"] == 1
    groth16.prove_from_witness(dev, r1cs, good, r, s)
    assert capi.last_timing()["fallbacks"] == 0
    assert CU.words(groth16.prove_end(groth16.prove_witness_begin(dev, r1cs, wh, r, s))) == want
    assert capi.last_timing()["fallbacks"] == 1
    assert CU.words(groth16.prove_end(groth16.prove_witness_host_begin(dev, r1cs, bad, r, s))) == want
    assert capi.last_timing()["fallbacks"] == 1
    assert CU.words(groth16.prove_from_r1cs(dev, r1cs, wh, r, s)[0]) == want


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------
def refused(codes, fn, *args):
    with pytest.raises(capi.GosnarkHipError) as e:
        fn(*args)
    assert e.value.code in codes, str(e.value)
    assert len(str(e.value)) > 40, "a refusal says why"
    return str(e.value)


def test_refusals_and_the_node_routes_beside_a_domain_key():
    inst = instance(3, 5)
    a, b, c = inst.csr()
    refused((GS_ERR_ARG,), circom.DeviceDomainR1CS, 0, a, b, c, inst.nvars)
    refused((GS_ERR_ARG,), circom.DeviceDomainR1CS, 28, a, b, c, inst.nvars)
    refused((GS_ERR_SHAPE,), circom.DeviceDomainR1CS, 2, a, b, c, inst.nvars)        # 5 rows > 4 points
    dev, r1cs = inst.upload()
    circom.DeriveEvalBasis(dev, 3)
    wh = capi.scalars_upload(CU.u64(inst.w))
    r, s = rs_pairs(90, 1)[0]
    want = groth16.prove_from_witness(dev, r1cs, wh, r, s)
    CU.assert_closed_form(want, inst.expected_scalars(inst.w, r, s))

    def every_witness_entry_point_refuses(key, codes=(GS_ERR_SHAPE,)):
        refused(codes, groth16.prove_from_witness, key, r1cs, wh, r, s)
        refused(codes, groth16.prove_from_witness_host, key, r1cs, inst.w, r, s)
        refused(codes + (GS_ERR_ARG,), groth16.prove_witness_begin, key, r1cs, wh, r, s)
        refused(codes + (GS_ERR_ARG,), groth16.prove_witness_host_begin, key, r1cs, inst.w, r, s)
        refused(codes, groth16.prove_from_r1cs, key, r1cs, wh, r, s)

    # a key of the reference's setup (nodes 1..n) for the same system, and the node routes with it
    toxic = (inst.tau, inst.alpha, inst.beta, inst.gamma, inst.delta)
    ref_key, _ = groth16.GenerateTrustedSetupSparse(inst.n, inst.nvars, inst.npublic, a, b, c, toxic)
    every_witness_entry_point_refuses(ref_key)
    refused((GS_ERR_SHAPE,), circom.DeriveEvalBasis, ref_key, 3)
    refused((GS_ERR_SHAPE,), circom.SetEvalBasis, ref_key, groth16.ExportPkArray(dev, "PowersTauDeltaEval"), 3)
    nodes = r1csqap.DeviceR1CS(a, b, c, inst.nvars)
    node_px = groth16.prove_resident(ref_key, wh, nodes.ComputePxResident(wh), r, s)
    assert CU.words(groth16.prove_from_witness(ref_key, nodes, wh, r, s)) == CU.words(node_px)
    assert CU.words(groth16.prove_end(groth16.prove_witness_begin(ref_key, nodes, wh, r, s))) == CU.words(node_px)
    assert capi.last_timing()["fallbacks"] == 0 and CU.words(node_px) != CU.words(want)
    assert CU.words(groth16.prove_from_witness(dev, r1cs, wh, r, s)) == CU.words(want)           # ... next to the domain one
    # a domain key of another m (same variables)
    other = CU.Instance(4, 5, 1)
    other_key, _ = other.upload()
    every_witness_entry_point_refuses(other_key)
    refused((GS_ERR_SHAPE,), circom.DeriveEvalBasis, dev, 4)
    # a key with too short an h array
    short_key, _ = inst.upload(n_hexps=6)
    every_witness_entry_point_refuses(short_key)
    # a key slice, the multi-device entry points, Pinocchio
    every_witness_entry_point_refuses(groth16.ShardPk(dev, 0, 2), (GS_ERR_SHAPE, GS_ERR_ARG))
    refused((GS_ERR_SHAPE,), groth16.witness_values, dev, r1cs, wh)
    refused((GS_ERR_SHAPE,), groth16.witness_values, dev, nodes, wh)                             # a coset basis is no node basis
    pin_key, _ = snark.GenerateTrustedSetupSparse(inst.n, inst.nvars, inst.npublic, a, b, c, (inst.tau,) + tuple(range(11, 18)))
    refused((GS_ERR_SHAPE,), snark.prove_from_witness, pin_key, r1cs, wh)
    refused((GS_ERR_SHAPE, GS_ERR_ARG), snark.prove_witness_begin, pin_key, r1cs, wh)
    # nothing above left the device in an error state
    assert CU.words(groth16.prove_from_witness(dev, r1cs, wh, r, s)) == CU.words(want)
    capi.trim()                                                                                   # releases the cached spectrum; rebuilt on demand
    assert CU.words(groth16.prove_from_witness(dev, r1cs, wh, r, s)) == CU.words(want)
