"""-m gpu: the quotient-basis array of a proving key (csrc/prove.h, ProverKey::h_quot) and the prover route it opens.

With D = deg Z, g = 1 / rev(Z) as a power series and T the key's h array (PowersTauDelta / G1T),
    Q[m] = sum_{d <= m} g_d T[m - d],   m < len(T),
and for every px:  sum_j floor(px / Z)_j T[j] = sum_m px[D + m] Q[m]  -- the h-sum of a proof as ONE MSM over the top coefficients of
px, nothing divided by Z.  Here: the array the setups emit is that convolution (g from Python integers, the sums from the C oracle's
naive MSM); proofs with the array, after detaching it and in closed form are the same points on every entry point and px shape;
keys built elsewhere (the reference's compiled prover's goldens) prove the recorded proof with an attached array; and the route
costs no table bytes and has no polynomial phase."""
import os
import subprocess
import sys

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16, snark, synth
import golden_util as GU
from r1cs_shapes import lagrange_at
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = O.R


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    yield
    capi.set_table_policy("auto")


# ---- the definition, outside the library ------------------------------------------------------------------------------------------
def series_inverse_of_reversed(z, k):
    """first k coefficients of 1 / rev(z) over Fr (z: coefficients, lowest first, leading one non-zero)"""
    f = [c % R for c in reversed(z)]
    inv0 = pow(f[0], R - 2, R)
    g = []
    for i in range(k):
        acc = 1 if i == 0 else 0
        for d in range(1, min(i, len(f) - 1) + 1):
            acc -= f[d] * g[i - d]
        g.append(acc % R * inv0 % R)
    return g


def pts_u64(points):
    return capi.ints_to_u64([c for p in points for c in p]).reshape(-1, 12)


def naive_quot_basis(t_points, z):
    """Q[m] = sum_{d <= m} g_d T[m - d] by the C oracle's literal double-and-add MSM -> affine (x, y) or None"""
    n = len(t_points)
    g = series_inverse_of_reversed(z, n)
    gs = capi.ints_to_u64(g).reshape(-1, 4)
    rev = pts_u64(t_points)[::-1]                       # rev[n - 1 - i] = T[i]
    return [C.g1_affine(C.g1_msm_naive(np.ascontiguousarray(rev[n - 1 - m:]), gs[:m + 1])) for m in range(n)]


def affine_of(points):
    return [None if p[2] == 0 else (p[0], p[1]) for p in points]


def groth_z(pk):
    z = np.zeros((pk.nvars - 1, 4), dtype=np.uint64)
    capi.check(capi.load_library().gs_groth16_pk_export(capi.Handle(pk.handle.h), 6, capi.ptr64(z), pk.nvars - 1))
    return capi.u64_to_ints(z)


@pytest.mark.parametrize("n", [2, 3, 8, 33, 257])
@pytest.mark.parametrize("extra", [0, 1])
def test_setup_emits_the_convolution_of_the_inverse_series_with_the_h_array(n, extra):
    inst = synth.sqchain_setup_instance(n, 0x9100 + 2 * n + extra, extra)
    pk = inst.device_pk()
    assert capi.pk_quot_count(pk.handle) == inst.m - 1
    t = groth16.ExportPkArray(pk, "PowersTauDelta")
    q = groth16.ExportPkArray(pk, "PowersTauDeltaQuot")
    assert len(q) == len(t) == inst.m - 1
    assert affine_of(q) == naive_quot_basis(t, groth_z(pk))


def test_pinocchio_setup_emits_the_same_convolution():
    inst = synth.sqchain_pinocchio_instance(33, 0x9180, 1)
    pk = inst.device_pk()
    z = np.zeros((pk.nvars - 1, 4), dtype=np.uint64)
    capi.check(capi.load_library().gs_pinocchio_pk_export(capi.Handle(pk.h), 8, capi.ptr64(z), pk.nvars - 1))
    t, q = snark.ExportPkArray(pk, "G1T"), snark.ExportPkArray(pk, "G1TQuot")
    assert len(q) == len(t) == inst.m - 1
    assert affine_of(q) == naive_quot_basis(t, capi.u64_to_ints(z))


# ---- proofs: with the array == after detaching it == closed form ----------------------------------------------------------------
def qap_at_tau(r1cs, n, w, lag, npublic):
    """(A(tau), B(tau), C(tau)) over the whole witness, and per matrix the column values a_i(tau) of the variables i <= npublic"""
    sums, cols = [], []
    for rp, cl, vl in r1cs:
        rp, cl, vals = [int(x) for x in rp], [int(x) for x in cl], capi.u64_to_ints(vl)
        tot, col = 0, [0] * (npublic + 1)
        for j in range(n):
            acc = 0
            for e in range(rp[j], rp[j + 1]):
                acc += vals[e] * w[cl[e]]
                if cl[e] <= npublic:
                    col[cl[e]] = (col[cl[e]] + vals[e] * lag[j]) % R
            tot += acc % R * lag[j]
        sums.append(tot % R)
        cols.append(col)
    return sums, cols


def groth_closed_form(inst, npublic, r, s):
    """synth.SqchainSetupInstance.expected_proof_scalars for any NPublic (groth16.go:243-275 with the toxic values known)"""
    T, Ka, Kb, _, Kd = inst.toxic
    w = capi.u64_to_ints(inst.w_host)
    (At, Bt, Ct), cols = qap_at_tau(inst.r1cs, inst.n, w, lagrange_at(inst.n, T), npublic)
    a = (At + Ka + r * Kd) % R
    b = (Bt + Kb + s * Kd) % R
    priv = (Kb * At + Ka * Bt + Ct) % R
    for i in range(npublic + 1):
        priv = (priv - w[i] * (Kb * cols[0][i] + Ka * cols[1][i] + cols[2][i])) % R
    c = ((priv + At * Bt - Ct) * pow(Kd, R - 2, R) + s * a + r * b - r * s % R * Kd) % R
    return a, b, c


def g1_multiple(k):
    a = C.g1_affine(C.g1_mul_scalar(O.G1_GEN, k))
    return (0, 0, 0) if a is None else (a[0], a[1], 1)


def g2_multiple(k):
    a = C.g2_affine(C.g2_mul_scalar(O.G2_GEN, k))
    return ((0, 0), (0, 0), (0, 0)) if a is None else (a[0], a[1], (1, 0))


def groth_points(p):
    return (p.PiA, p.PiB, p.PiC)


def groth_all_entry_points(pk, w, px, w_host, px_host, r, s):
    """the proof through the blocking call, three tickets in flight and a host-buffer ticket: one value, or an assertion"""
    first = groth_points(groth16.prove_resident(pk, w, px, r, s))
    tickets = [groth16.prove_begin(pk, w, px, r, s) for _ in range(3)]
    assert all(groth_points(groth16.prove_end(t)) == first for t in tickets)
    assert groth_points(groth16.prove_end(groth16.prove_host_begin(pk, w_host, px_host, r, s))) == first
    return first


def px_shapes(px_host, nz):
    """full length | three coefficients short | shorter than Z (no quotient: the h-sum is infinity) | entries in [r, 2^256) as raw limbs"""
    ints = capi.u64_to_ints(px_host)
    top = (1 << 256) - 1
    raised = [v + ((top - v) // R) * R if i % 3 == 0 else v + R if i % 3 == 1 else v for i, v in enumerate(ints)]
    assert all(v < 1 << 256 for v in raised) and max(raised) >= 5 * R
    return {"full": px_host, "short3": np.ascontiguousarray(px_host[:-3]), "below_z": np.ascontiguousarray(px_host[:nz - 1]),
            "raw": capi.ints_to_u64(raised).reshape(-1, 4)}


@pytest.mark.parametrize("n", [8, 257, 4096])
def test_groth16_proofs_with_the_array_detached_and_in_closed_form_are_equal(n):
    inst = synth.sqchain_setup_instance(n, 0x9200 + n)
    a, b, c = inst.r1cs
    r, s = synth.field_elems(2, 92)
    for npublic in (0, 1, 3):
        pk = inst.device_pk() if npublic == 1 else groth16.GenerateTrustedSetupSparse(n, inst.m, npublic, a, b, c, inst.toxic)[0]
        quot = groth16.ExportPkArray(pk, "PowersTauDeltaQuot")
        ea, eb, ec = groth_closed_form(inst, npublic, r, s)
        closed = (g1_multiple(ea), g2_multiple(eb), g1_multiple(ec))
        shapes = px_shapes(inst.px_host, pk.nvars - 1)
        with_array = {}
        for name, pxh in shapes.items():
            px = capi.scalars_upload(pxh)
            with_array[name] = groth_all_entry_points(pk, inst.w, px, inst.w_host, pxh, r, s)
        assert with_array["full"] == closed and with_array["raw"] == closed, npublic
        groth16.SetQuotBasis(pk, None)
        assert capi.pk_quot_count(pk.handle) == 0
        for name, pxh in shapes.items():
            px = capi.scalars_upload(pxh)
            assert groth_all_entry_points(pk, inst.w, px, inst.w_host, pxh, r, s) == with_array[name], (npublic, name)
        groth16.SetQuotBasis(pk, quot)
        assert capi.pk_quot_count(pk.handle) == len(quot)
        assert groth_points(groth16.prove_resident(pk, inst.w, inst.px, r, s)) == closed


PIN_FIELDS = ("PiA", "PiAp", "PiB", "PiBp", "PiC", "PiCp", "PiH", "PiKp")


def pin_points(p):
    return tuple(getattr(p, k) for k in PIN_FIELDS)


def pin_all_entry_points(pk, w, px, w_host, px_host):
    first = pin_points(snark.prove_resident(pk, w, px))
    tickets = [snark.prove_begin(pk, w, px) for _ in range(3)]
    assert all(pin_points(snark.prove_end(t)) == first for t in tickets)
    assert pin_points(snark.prove_end(snark.prove_host_begin(pk, w_host, px_host))) == first
    return first


@pytest.mark.parametrize("n", [8, 257, 4096])
def test_pinocchio_proofs_with_the_array_detached_and_in_closed_form_are_equal(n):
    inst = synth.sqchain_pinocchio_instance(n, 0x9300 + n)
    a, b, c = inst.r1cs
    T = inst.toxic[0]
    w = capi.u64_to_ints(inst.w_host)
    (At, Bt, Ct), _ = qap_at_tau(inst.r1cs, n, w, lagrange_at(n, T), 0)
    zt = 1
    for k in range(1, inst.m - 1):
        zt = zt * (T - k) % R
    pih = g1_multiple((At * Bt - Ct) * pow(zt, R - 2, R) % R)            # PiH = H(tau) G, H Z = A B - C (snark.go:284-286)
    for npublic in (0, 1, 3):
        pk = inst.device_pk() if npublic == 1 else snark.GenerateTrustedSetupSparse(n, inst.m, npublic, a, b, c, inst.toxic)[0]
        quot = snark.ExportPkArray(pk, "G1TQuot")
        shapes = px_shapes(inst.px_host, pk.nvars - 1)
        with_array = {}
        for name, pxh in shapes.items():
            with_array[name] = pin_all_entry_points(pk, inst.w, capi.scalars_upload(pxh), inst.w_host, pxh)
        assert with_array["full"][6] == pih and with_array["raw"] == with_array["full"], npublic
        assert with_array["below_z"][6] == (0, 0, 0)
        snark.SetQuotBasis(pk, None)
        for name, pxh in shapes.items():
            assert pin_all_entry_points(pk, inst.w, capi.scalars_upload(pxh), inst.w_host, pxh) == with_array[name], (npublic, name)
        snark.SetQuotBasis(pk, quot)
        assert pin_points(snark.prove_resident(pk, inst.w, inst.px)) == with_array["full"]
        if npublic == 1:
            assert snark.VerifyProof(inst.vk, snark.prove_resident(pk, inst.w, inst.px), inst.public) is True


# ---- keys built elsewhere -----------------------------------------------------------------------------------------------------------
def jac_affine_g1(p):
    a = O.G1.Affine(p)
    return (0, 0, 0) if a is None else (a[0], a[1], 1)


def jac_affine_g2(p):
    a = O.G2.Affine(p)
    return ((0, 0), (0, 0), (0, 0)) if a is None else (a[0], a[1], (1, 0))


def as_jacobian(affine):
    return [(0, 0, 0) if a is None else (a[0], a[1], 1) for a in affine]


def test_foreign_groth16_key_proves_the_recorded_proof_with_an_attached_array():
    """tests/golden/wasm_groth_rand_m17.json: the reference's own key, witness and proof.  The array is the naive convolution of the
    file's PowersTauDelta (nobody knows tau); attached, the key takes the new route and still emits the recorded proof."""
    rec = GU.load("groth_rand_m17")
    opk = GU.groth_pk(rec["setup"])
    r, s = GU.rs_from_stream(rec["rand"])
    circ = groth16.Circuit(rec["circuit"]["NVars"], rec["circuit"]["NPublic"])
    pk = groth16.Pk(BACDelta=opk.BACDelta, Z=opk.Z, G1_Alpha=opk.G1_Alpha, G1_Beta=opk.G1_Beta, G1_Delta=opk.G1_Delta,
                    G1_At=opk.G1_At, G1_BACGamma=opk.G1_BACGamma, G2_Beta=opk.G2_Beta, G2_Delta=opk.G2_Delta,
                    G2_BACGamma=opk.G2_BACGamma, PowersTauDelta=opk.PowersTauDelta)
    want = (jac_affine_g1(GU.g1(rec["proof"]["PiA"])), jac_affine_g2(GU.g2(rec["proof"]["PiB"])), jac_affine_g1(GU.g1(rec["proof"]["PiC"])))
    dev = groth16.UploadPk(pk, circ)
    assert capi.pk_quot_count(dev.handle) == 0
    assert groth_points(groth16.GenerateProofsWithRS(circ, pk, rec["w"], rec["px"], r, s)) == want
    groth16.SetQuotBasis(dev, as_jacobian(naive_quot_basis([jac_affine_g1(p) for p in opk.PowersTauDelta], opk.Z)))
    assert capi.pk_quot_count(dev.handle) == len(opk.PowersTauDelta)
    assert groth_points(groth16.GenerateProofsWithRS(circ, pk, rec["w"], rec["px"], r, s)) == want
    assert capi.last_timing()["poly_ms"] == 0
    groth16.SetQuotBasis(dev, None)
    assert groth_points(groth16.GenerateProofsWithRS(circ, pk, rec["w"], rec["px"], r, s)) == want
    groth16.DeriveQuotBasis(dev)
    assert capi.pk_quot_count(dev.handle) == len(opk.PowersTauDelta)
    assert groth_points(groth16.GenerateProofsWithRS(circ, pk, rec["w"], rec["px"], r, s)) == want and capi.last_timing()["poly_ms"] == 0
    groth16.SetQuotBasis(dev, None)
    assert groth_points(groth16.GenerateProofsWithRS(circ, pk, rec["w"], rec["px"], r, s)) == want
    with pytest.raises(capi.GosnarkHipError):
        groth16.SetQuotBasis(dev, [jac_affine_g1(p) for p in opk.PowersTauDelta][:-1])       # not len(PowersTauDelta) points


def test_foreign_pinocchio_key_proves_the_recorded_proof_with_an_attached_array():
    rec = GU.load("pinocchio_rand_m9")
    opk = GU.pinocchio_pk(rec["setup"])
    circ = snark.Circuit(rec["circuit"]["NVars"], rec["circuit"]["NPublic"])
    pk = snark.Pk(G1T=opk.G1T, A=opk.A, B=opk.B, C=opk.C, Kp=opk.Kp, Ap=opk.Ap, Bp=opk.Bp, Cp=opk.Cp, Z=opk.Z)
    want = tuple(jac_affine_g2(GU.g2(rec["proof"][k])) if k == "PiB" else jac_affine_g1(GU.g1(rec["proof"][k])) for k in PIN_FIELDS)
    dev = snark.UploadPk(pk, circ)
    assert pin_points(snark.GenerateProofs(circ, pk, rec["w"], rec["px"])) == want
    snark.SetQuotBasis(dev, as_jacobian(naive_quot_basis([jac_affine_g1(p) for p in opk.G1T], opk.Z)))
    assert capi.pk_quot_count(dev) == len(opk.G1T)
    assert pin_points(snark.GenerateProofs(circ, pk, rec["w"], rec["px"])) == want
    snark.SetQuotBasis(dev, None)
    assert pin_points(snark.GenerateProofs(circ, pk, rec["w"], rec["px"])) == want
    capi.check(capi.load_library().gs_pinocchio_pk_derive_quot(capi.Handle(dev.h)))
    assert capi.pk_quot_count(dev) == len(opk.G1T)
    assert pin_points(snark.GenerateProofs(circ, pk, rec["w"], rec["px"])) == want
    snark.SetQuotBasis(dev, None)
    assert pin_points(snark.GenerateProofs(circ, pk, rec["w"], rec["px"])) == want


def test_binary_key_container_carries_the_quotient_basis(tmp_path):
    from gosnark_amd import utils
    inst = synth.sqchain_setup_instance(300, 0x9400)
    r, s = synth.field_elems(2, 94)
    want = groth_points(groth16.prove_resident(inst.device_pk(), inst.w, inst.px, r, s))
    path = str(tmp_path / "groth.key")
    utils.GrothSetupToBinary(path, groth16.Circuit(inst.m, 1), inst.device_pk(), inst.vk)
    assert utils.ReadBinary(path)[3]["PowersTauDeltaQuot"].shape == (inst.m - 1, 12)
    _, loaded = utils.UploadGrothPkBinary(path)
    assert capi.pk_quot_count(loaded.handle) == inst.m - 1
    assert groth_points(groth16.prove_resident(loaded, inst.w, inst.px, r, s)) == want and capi.last_timing()["poly_ms"] == 0
    pin = synth.sqchain_pinocchio_instance(300, 0x9401)
    want = pin_points(snark.prove_resident(pin.device_pk(), pin.w, pin.px))
    path = str(tmp_path / "pinocchio.key")
    utils.SetupToBinary(path, snark.Circuit(pin.m, 1), pin.device_pk(), pin.vk)
    _, loaded = utils.UploadPkBinary(path)
    assert capi.pk_quot_count(loaded.handle) == pin.m - 1
    assert pin_points(snark.prove_resident(loaded, pin.w, pin.px)) == want and capi.last_timing()["poly_ms"] == 0


# ---- derivation: the convolution by a transform in the group (csrc/ecntt.hip) ---------------------------------------------------
def rebuilt_groth_key(pk, nvars, npublic):
    """a key made of the exported arrays of `pk` alone (gs_groth16_pk_create: it has no quotient-basis array)"""
    arrays = {k: groth16.ExportPkArray(pk, k) for k in ("G1_At", "G1_BACGamma", "G2_BACGamma", "BACDelta", "PowersTauDelta")}
    singles = np.zeros(84, dtype=np.uint64)
    capi.check(capi.load_library().gs_groth16_pk_export(capi.Handle(pk.handle.h), 5, capi.ptr64(singles), 5))
    v = capi.u64_to_ints(singles)
    hpk = groth16.Pk(BACDelta=arrays["BACDelta"], Z=groth_z(pk), G1_Alpha=(v[0], v[1], v[2]), G1_Beta=(v[3], v[4], v[5]),
                     G1_Delta=(v[6], v[7], v[8]), G1_At=arrays["G1_At"], G1_BACGamma=arrays["G1_BACGamma"],
                     G2_Beta=((v[9], v[10]), (v[11], v[12]), (v[13], v[14])), G2_Delta=((v[15], v[16]), (v[17], v[18]), (v[19], v[20])),
                     G2_BACGamma=arrays["G2_BACGamma"], PowersTauDelta=arrays["PowersTauDelta"])
    return groth16.UploadPk(hpk, groth16.Circuit(nvars, npublic))


@pytest.mark.parametrize("n", [2, 3, 8, 33, 257, 1000])
@pytest.mark.parametrize("extra", [0, 1])
def test_derivation_gives_the_array_the_setup_emitted(n, extra):
    """transform lengths 4 .. 2048, len_h a power of two, one more, one less and far from one"""
    inst = synth.sqchain_setup_instance(n, 0x9600 + 2 * n + extra, extra)
    pk = inst.device_pk()
    want = groth16.ExportPkArray(pk, "PowersTauDeltaQuot")
    foreign = rebuilt_groth_key(pk, inst.m, 1)
    assert capi.pk_quot_count(foreign.handle) == 0
    groth16.DeriveQuotBasis(foreign)
    assert capi.pk_quot_count(foreign.handle) == inst.m - 1
    assert groth16.ExportPkArray(foreign, "PowersTauDeltaQuot") == want
    r, s = synth.field_elems(2, 96)
    assert groth_points(groth16.prove_resident(foreign, inst.w, inst.px, r, s)) == groth_points(groth16.prove_resident(pk, inst.w, inst.px, r, s))


def test_pinocchio_derivation_gives_the_array_the_setup_emitted():
    inst = synth.sqchain_pinocchio_instance(33, 0x9680, 1)
    pk = inst.device_pk()
    want = snark.ExportPkArray(pk, "G1TQuot")
    snark.SetQuotBasis(pk, None)
    snark.DeriveQuotBasis(pk)
    assert snark.ExportPkArray(pk, "G1TQuot") == want


@pytest.mark.parametrize("m", [6, 18, 34])
def test_derivation_on_repeated_opposite_and_infinite_points(m):
    """An h array of len_h = m - 1 <= 33 made of runs of one point, P next to -P and infinities: the butterflies meet P + P, P - P and
    infinity on either side.  The derived array is the oracle's naive convolution."""
    import random
    import gpu_util as U
    rng = random.Random(9700 + m)
    z = [1]
    for i in range(1, m - 1):
        z = O.PF.Mul(z, [O.FR.Neg(i), 1])
    base = [U.rand_g1_jac(rng) for _ in range(3)]
    neg = lambda p: (p[0], (O.Q - p[1]) % O.Q, p[2])   # noqa: E731
    pattern = [base[0], base[0], neg(base[0]), O.G1_ZERO, O.G1_ZERO, base[1], neg(base[1]), base[1], base[1], base[2], O.G1_ZERO]
    t = [pattern[i % len(pattern)] for i in range(len(z))]
    pk = groth16.Pk(BACDelta=[U.rand_g1_jac(rng) for _ in range(m)], Z=z, G1_Alpha=base[0], G1_Beta=base[1], G1_Delta=base[2],
                    G1_At=[U.rand_g1_jac(rng) for _ in range(m)], G1_BACGamma=[U.rand_g1_jac(rng) for _ in range(m)],
                    G2_Beta=U.rand_g2_jac(rng), G2_Delta=U.rand_g2_jac(rng), G2_BACGamma=[U.rand_g2_jac(rng) for _ in range(m)],
                    PowersTauDelta=t)
    dev = groth16.UploadPk(pk, groth16.Circuit(m, 1))
    groth16.DeriveQuotBasis(dev)
    assert affine_of(groth16.ExportPkArray(dev, "PowersTauDeltaQuot")) == naive_quot_basis([jac_affine_g1(p) for p in t], z)


# ---- what the route costs -----------------------------------------------------------------------------------------------------------
_CHILD = """
import sys
sys.path.insert(0, %r)
import gosnark_amd
from gosnark_amd import capi, groth16, synth
capi.init()
capi.set_table_policy("always")
inst = synth.sqchain_setup_instance(1 << 12, 0x9500)
r, s = synth.field_elems(2, 95)
p = groth16.prove_resident(inst.device_pk(), inst.w, inst.px, r, s)
print("RESULT", capi.handle_bytes(inst.device_pk().handle)[1], capi.last_timing()["poly_ms"], p.PiC[0], p.PiC[1])
"""


def test_the_route_costs_no_table_bytes_and_has_no_polynomial_phase():
    """Policy `always`: a setup key's tables with the route are no larger than with GS_NO_QUOT_BASIS (read once per process, hence the
    two child processes), gs_timing's polynomial phase is empty on the route and not without it, and the proof is the same."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = {}
    for label, extra in (("quot", {}), ("divide", {"GS_NO_QUOT_BASIS": "1"})):
        env = {k: v for k, v in os.environ.items() if k != "GS_NO_QUOT_BASIS"}
        env.update(extra)
        out = subprocess.run([sys.executable, "-c", _CHILD % root], env=env, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stderr[-2000:]
        line = [x for x in out.stdout.splitlines() if x.startswith("RESULT")][0].split()
        res[label] = (int(line[1]), float(line[2]), line[3], line[4])
    print(res)
    assert 0 < res["quot"][0] <= res["divide"][0]
    assert res["quot"][1] == 0 and res["divide"][1] > 0
    assert res["quot"][2:] == res["divide"][2:]
