"""-m gpu: gs_*_pk_derive_eval -- the evaluation-basis array of a key that was built elsewhere, computed on the device from its h array
alone (csrc/ecntt.hip: a transposed subproduct tree over the nodes n+1 .. 2n with the transforms carried out in the group).

With T the key's h array (PowersTauDelta / G1T) and l_j the Lagrange basis over the nodes n+1 .. 2n,
    E[j-1] = sum_{i < n} coeff_i(l_j) T[i],   j = 1..n,
so that sum_j H(n+j) E[j-1] = sum_i h_i T[i] for every H of degree < n.  Here: the derived array is that sum with the coefficients
from Python integers and the sums from the C oracle's naive MSM; it equals the array the device setup emits while it knows tau; a
foreign key with it proves what the setup key proves on every witness entry point; keys the reference built take it; repeated,
opposite and infinite points go through; wrong shapes are refused."""
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16, r1csqap, snark, synth, utils
import golden_util as GU
import gpu_util as U
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = O.R


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)
    yield
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)


# ---- the definition, outside the library ------------------------------------------------------------------------------------------
def lagrange_rows(n):
    """coefficients (lowest first) of l_j, j = 1..n, over the nodes n+1 .. 2n: schoolbook products of Python integers"""
    nodes = [n + j for j in range(1, n + 1)]
    full = [1]                                              # M(x) = prod (x - x_k)
    for xk in nodes:
        nxt = [0] * (len(full) + 1)
        for i, c in enumerate(full):
            nxt[i] = (nxt[i] - c * xk) % R
            nxt[i + 1] = (nxt[i + 1] + c) % R
        full = nxt
    rows = []
    for xj in nodes:
        q, carry = [0] * n, 0                               # M(x) / (x - xj) by synthetic division, then / M'(xj)
        for i in range(n, 0, -1):
            carry = (full[i] + carry * xj) % R
            q[i - 1] = carry
        den = 1
        for xk in nodes:
            if xk != xj:
                den = den * (xj - xk) % R
        inv = pow(den, R - 2, R)
        rows.append([c * inv % R for c in q])
    return rows


def pts_u64(points):
    return capi.ints_to_u64([c for p in points for c in p]).reshape(-1, 12)


def naive_eval_basis(t_points, n):
    """E[j-1] = sum_i coeff_i(l_j) T[i] by the C oracle's literal double-and-add MSM -> affine (x, y) or None"""
    t = np.ascontiguousarray(pts_u64(t_points)[:n])
    return [C.g1_affine(C.g1_msm_naive(t, capi.ints_to_u64(row).reshape(-1, 4), threads=8)) for row in lagrange_rows(n)]


def test_the_rows_outside_the_library_are_a_lagrange_basis():
    for n in (2, 5, 9):
        for j, row in enumerate(lagrange_rows(n)):
            assert [sum(c * pow(n + k, i, R) for i, c in enumerate(row)) % R for k in range(1, n + 1)] == [int(k == j + 1) for k in range(1, n + 1)]


def affine_of(points):
    return [None if p[2] == 0 else (p[0], p[1]) for p in points]


def jac_affine_g1(p):
    a = O.G1.Affine(p)
    return (0, 0, 0) if a is None else (a[0], a[1], 1)


def jac_affine_g2(p):
    a = O.G2.Affine(p)
    return ((0, 0), (0, 0), (0, 0)) if a is None else (a[0], a[1], (1, 0))


def g1_multiple(k):
    a = C.g1_affine(C.g1_mul_scalar(O.G1_GEN, k))
    return (0, 0, 0) if a is None else (a[0], a[1], 1)


def g2_multiple(k):
    a = C.g2_affine(C.g2_mul_scalar(O.G2_GEN, k))
    return ((0, 0), (0, 0), (0, 0)) if a is None else (a[0], a[1], (1, 0))


def groth_points(p):
    return (p.PiA, p.PiB, p.PiC)


def groth_z(pk):
    z = np.zeros((pk.nvars - 1, 4), dtype=np.uint64)
    capi.check(capi.load_library().gs_groth16_pk_export(capi.Handle(pk.handle.h), 6, capi.ptr64(z), pk.nvars - 1))
    return capi.u64_to_ints(z)


def rebuilt_groth_key(pk, nvars, npublic):
    """a key made of the exported arrays of `pk` alone (gs_groth16_pk_create: monomial-basis h array and nothing else)"""
    arrays = {k: groth16.ExportPkArray(pk, k) for k in ("G1_At", "G1_BACGamma", "G2_BACGamma", "BACDelta", "PowersTauDelta")}
    singles = np.zeros(84, dtype=np.uint64)
    capi.check(capi.load_library().gs_groth16_pk_export(capi.Handle(pk.handle.h), 5, capi.ptr64(singles), 5))
    v = capi.u64_to_ints(singles)
    hpk = groth16.Pk(BACDelta=arrays["BACDelta"], Z=groth_z(pk), G1_Alpha=(v[0], v[1], v[2]), G1_Beta=(v[3], v[4], v[5]),
                     G1_Delta=(v[6], v[7], v[8]), G1_At=arrays["G1_At"], G1_BACGamma=arrays["G1_BACGamma"],
                     G2_Beta=((v[9], v[10]), (v[11], v[12]), (v[13], v[14])), G2_Delta=((v[15], v[16]), (v[17], v[18]), (v[19], v[20])),
                     G2_BACGamma=arrays["G2_BACGamma"], PowersTauDelta=arrays["PowersTauDelta"])
    return groth16.UploadPk(hpk, groth16.Circuit(nvars, npublic))


def rebuilt_pinocchio_key(pk, nvars, npublic):
    arrays = {k: snark.ExportPkArray(pk, k) for k in ("G1T", "A", "B", "C", "Kp", "Ap", "Bp", "Cp")}
    z = np.zeros((nvars - 1, 4), dtype=np.uint64)
    capi.check(capi.load_library().gs_pinocchio_pk_export(capi.Handle(pk.h), 8, capi.ptr64(z), nvars - 1))
    dev = snark.UploadPk(snark.Pk(Z=capi.u64_to_ints(z), **arrays), snark.Circuit(nvars, npublic))
    return snark.DevicePk(dev, nvars, npublic)


# ---- 1. the definition ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3, 4, 5, 8, 9, 33])
@pytest.mark.parametrize("extra", [0, 1])
def test_derived_array_is_the_lagrange_combination_of_the_h_array(n, extra):
    """a power of two, one more, one less, a single level (n = 2), and r_L != r_R at several levels (n = 5, 9, 33)"""
    inst = synth.sqchain_setup_instance(n, 0xE100 + 2 * n + extra, extra)
    foreign = rebuilt_groth_key(inst.device_pk(), inst.m, 1)
    assert capi.pk_eval_count(foreign.handle) == 0
    groth16.DeriveEvalBasis(foreign, n)
    assert capi.pk_eval_count(foreign.handle) == n
    got = groth16.ExportPkArray(foreign, "PowersTauDeltaEval")
    assert affine_of(got) == naive_eval_basis(groth16.ExportPkArray(foreign, "PowersTauDelta"), n)


# ---- 2. agreement with the device setup, and the proofs -----------------------------------------------------------------------------
def groth_witness_entry_points(pk, dev, w, w_host, r, s):
    """the witness proof through the blocking call, three tickets in flight and a host-buffer ticket: one value, or an assertion"""
    first = groth_points(groth16.prove_from_witness(pk, dev, w, r, s))
    assert capi.last_timing()["fallbacks"] == 0
    tickets = [groth16.prove_witness_begin(pk, dev, w, r, s) for _ in range(3)]
    assert all(groth_points(groth16.prove_end(t)) == first for t in tickets)
    assert groth_points(groth16.prove_end(groth16.prove_witness_host_begin(pk, dev, w_host, r, s))) == first
    return first


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("extra", [0, 1])
def test_derived_array_equals_the_setups_and_the_foreign_key_proves_the_same(n, extra):
    inst = synth.sqchain_setup_instance(n, 0xE200 + 2 * n + extra, extra)
    pk = inst.device_pk()
    want = groth16.ExportPkArray(pk, "PowersTauDeltaEval")
    assert len(want) == n
    foreign = rebuilt_groth_key(pk, inst.m, 1)
    groth16.DeriveEvalBasis(foreign, n)
    assert capi.pk_eval_count(foreign.handle) == n
    assert groth16.ExportPkArray(foreign, "PowersTauDeltaEval") == want
    dev = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
    r, s = synth.field_elems(2, 0xE2 + n)
    a, b, c = inst.expected_proof_scalars(r, s)
    closed = (g1_multiple(a), g2_multiple(b), g1_multiple(c))
    assert groth_witness_entry_points(pk, dev, inst.w, inst.w_host, r, s) == closed
    assert groth_witness_entry_points(foreign, dev, inst.w, inst.w_host, r, s) == closed
    capi.set_eval_basis(False)
    assert groth_points(groth16.prove_from_witness(foreign, dev, inst.w, r, s)) == closed


# ---- 3. keys the reference built ----------------------------------------------------------------------------------------------------
X3_A = [[0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 1, 0, 1, 0, 0, 0], [5, 0, 0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0, 1, 0], [0, 1, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]]
X3_B = [[0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 1, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]]
X3_C = [[0, 0, 0, 1, 0, 0, 0, 0], [0, 0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 0, 0, 1, 0, 0], [0, 0, 0, 0, 0, 0, 1, 0], [0, 1, 0, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 0, 0, 0, 0]]


def file_groth_key(rec):
    opk = GU.groth_pk(rec["setup"])
    circ = groth16.Circuit(rec["circuit"]["NVars"], rec["circuit"]["NPublic"])
    pk = groth16.Pk(BACDelta=opk.BACDelta, Z=opk.Z, G1_Alpha=opk.G1_Alpha, G1_Beta=opk.G1_Beta, G1_Delta=opk.G1_Delta,
                    G1_At=opk.G1_At, G1_BACGamma=opk.G1_BACGamma, G2_Beta=opk.G2_Beta, G2_Delta=opk.G2_Delta,
                    G2_BACGamma=opk.G2_BACGamma, PowersTauDelta=opk.PowersTauDelta)
    return opk, groth16.UploadPk(pk, circ)


def test_the_references_x3_key_takes_the_derived_array_and_proves_the_recorded_proof():
    """tests/golden/wasm_groth_x3.json (n = 7, m = 8): nobody knows tau, so the array is pinned by the naive rows of the file's
    PowersTauDelta; the witness route over it gives the proof the reference's compiled prover recorded."""
    rec = GU.load("groth_x3")
    opk, dev = file_groth_key(rec)
    n = 7
    assert len(opk.Z) == n and len(opk.PowersTauDelta) == n and capi.pk_eval_count(dev.handle) == 0
    groth16.DeriveEvalBasis(dev, n)
    assert capi.pk_eval_count(dev.handle) == n
    assert affine_of(groth16.ExportPkArray(dev, "PowersTauDeltaEval")) == naive_eval_basis([jac_affine_g1(p) for p in opk.PowersTauDelta], n)
    rows = lambda mat: [{k: v for k, v in enumerate(row) if v} for row in mat]   # noqa: E731
    r1cs = r1csqap.DeviceR1CS(*(r1csqap.csr_from_rows(rows(m)) for m in (X3_A, X3_B, X3_C)), 8)
    r, s = GU.rs_from_stream(rec["rand"])
    want = (jac_affine_g1(GU.g1(rec["proof"]["PiA"])), jac_affine_g2(GU.g2(rec["proof"]["PiB"])), jac_affine_g1(GU.g1(rec["proof"]["PiC"])))
    w = capi.scalars_upload(capi.ints_to_u64([v % R for v in rec["w"]]))
    assert groth_points(groth16.prove_from_witness(dev, r1cs, w, r, s)) == want
    assert capi.last_timing()["fallbacks"] == 0


def defining_identity_holds(t_points, e_points, n, seed):
    """sum_j H(n+j) E[j-1] == sum_i h_i T[i] on a random H of degree n - 1, through two gs_msm_g1 calls"""
    rng = random.Random(seed)
    h = [rng.randrange(R) for _ in range(n)]
    vals = [sum(c * pow(n + j, i, R) for i, c in enumerate(h)) % R for j in range(1, n + 1)]
    mono = capi.msm(capi.g1_upload(pts_u64(t_points[:n])), capi.ints_to_u64(h))
    ev = capi.msm(capi.g1_upload(pts_u64(e_points)), capi.ints_to_u64(vals))
    return mono is not None and mono == ev


def test_the_references_m17_groth16_key():
    rec = GU.load("groth_rand_m17")
    opk, dev = file_groth_key(rec)
    n = 16
    assert len(opk.Z) == n
    groth16.DeriveEvalBasis(dev, n)
    e = groth16.ExportPkArray(dev, "PowersTauDeltaEval")
    t = [jac_affine_g1(p) for p in opk.PowersTauDelta]
    assert len(e) == n and defining_identity_holds(t, e, n, 1717)
    assert affine_of(e) == naive_eval_basis(t, n)


def test_the_references_m9_pinocchio_key():
    rec = GU.load("pinocchio_rand_m9")
    opk = GU.pinocchio_pk(rec["setup"])
    circ = snark.Circuit(rec["circuit"]["NVars"], rec["circuit"]["NPublic"])
    pk = snark.Pk(G1T=opk.G1T, A=opk.A, B=opk.B, C=opk.C, Kp=opk.Kp, Ap=opk.Ap, Bp=opk.Bp, Cp=opk.Cp, Z=opk.Z)
    dev = snark.DevicePk(snark.UploadPk(pk, circ), circ.NVars, circ.NPublic)
    n = 8
    assert len(opk.Z) == n and capi.pk_eval_count(dev.handle) == 0
    snark.DeriveEvalBasis(dev, n)
    e = snark.ExportPkArray(dev, "G1TEval")
    t = [jac_affine_g1(p) for p in opk.G1T]
    assert len(e) == n and defining_identity_holds(t, e, n, 909)
    assert affine_of(e) == naive_eval_basis(t, n)


# ---- 4. degenerate points -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [6, 18, 34])
def test_derivation_on_repeated_opposite_and_infinite_points(m):
    """An h array of m - 1 <= 33 points made of runs of one point, P next to -P and infinities: the butterflies meet P + P, P - P and
    infinity on either side, at both admissible n.  The derived array is the oracle's naive rows."""
    rng = random.Random(0xE400 + m)
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
    for n in (len(z), len(z) - 1):
        groth16.DeriveEvalBasis(dev, n)
        got = affine_of(groth16.ExportPkArray(dev, "PowersTauDeltaEval"))
        assert len(got) == n and got == naive_eval_basis([jac_affine_g1(p) for p in t], n), n


# ---- 5. shape and state -------------------------------------------------------------------------------------------------------------
def test_wrong_sizes_and_slices_are_refused():
    inst = synth.sqchain_setup_instance(12, 0xE500)
    foreign = rebuilt_groth_key(inst.device_pk(), inst.m, 1)
    nz = len(groth_z(foreign))
    assert nz == 12
    for bad in (nz - 2, nz + 1, 0, 1):
        with pytest.raises(capi.GosnarkHipError):
            groth16.DeriveEvalBasis(foreign, bad)
        assert capi.pk_eval_count(foreign.handle) == 0
    piece = groth16.ShardPk(foreign, 0, 2)
    with pytest.raises(capi.GosnarkHipError):
        groth16.DeriveEvalBasis(piece, nz)
    # deg Z + 1 would be admissible by Z, but the h array is one point short of it
    inst2 = synth.sqchain_setup_instance(2, 0xE501)
    f2 = rebuilt_groth_key(inst2.device_pk(), inst2.m, 1)
    with pytest.raises(capi.GosnarkHipError):
        groth16.DeriveEvalBasis(f2, 1)
    with pytest.raises(capi.GosnarkHipError):
        groth16.DeriveEvalBasis(f2, 3)
    pin = synth.sqchain_pinocchio_instance(12, 0xE502)
    pf = rebuilt_pinocchio_key(pin.device_pk(), pin.m, 1)
    for bad in (10, 13, 0, 1):
        with pytest.raises(capi.GosnarkHipError):
            snark.DeriveEvalBasis(pf, bad)
    ppiece = snark.ShardPk(pf, 0, 2)
    with pytest.raises(capi.GosnarkHipError):
        snark.DeriveEvalBasis(ppiece, 12)


def test_deriving_twice_and_over_an_attached_array():
    n = 100
    inst = synth.sqchain_setup_instance(n, 0xE510)
    want = groth16.ExportPkArray(inst.device_pk(), "PowersTauDeltaEval")
    foreign = rebuilt_groth_key(inst.device_pk(), inst.m, 1)
    groth16.DeriveEvalBasis(foreign, n)
    assert groth16.ExportPkArray(foreign, "PowersTauDeltaEval") == want
    groth16.DeriveEvalBasis(foreign, n)
    assert groth16.ExportPkArray(foreign, "PowersTauDeltaEval") == want
    other = want[1:] + want[:1]                               # a deliberately different array
    groth16.SetEvalBasis(foreign, other)
    assert groth16.ExportPkArray(foreign, "PowersTauDeltaEval") == other != want
    groth16.DeriveEvalBasis(foreign, n)
    assert groth16.ExportPkArray(foreign, "PowersTauDeltaEval") == want and capi.pk_eval_count(foreign.handle) == n


def test_memory_accounting_and_the_binary_container(tmp_path):
    n = 300
    inst = synth.sqchain_setup_instance(n, 0xE520)
    pk = inst.device_pk()
    dev = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
    r, s = synth.field_elems(2, 0xE521)
    want = groth_points(groth16.prove_from_witness(pk, dev, inst.w, r, s))
    foreign = rebuilt_groth_key(pk, inst.m, 1)
    obj_b, tab_b = capi.handle_bytes(foreign.handle)
    groth16.DeriveEvalBasis(foreign, n)
    assert capi.handle_bytes(foreign.handle) == (obj_b + 64 * n, tab_b)
    calls = 0
    while capi.handle_bytes(foreign.handle)[1] == tab_b and calls < 60:       # policy auto: tables arrive with the proofs that use the arrays
        assert groth_points(groth16.prove_from_witness(foreign, dev, inst.w, r, s)) == want
        calls += 1
    assert 1 <= calls < 60 and capi.handle_bytes(foreign.handle)[0] == obj_b + 64 * n
    path = str(tmp_path / "derived.key")
    utils.GrothSetupToBinary(path, groth16.Circuit(inst.m, 1), foreign, inst.vk)
    assert utils.ReadBinary(path)[3]["PowersTauDeltaEval"].shape == (n, 12)
    _, loaded = utils.UploadGrothPkBinary(path)
    assert capi.pk_eval_count(loaded.handle) == n
    assert groth16.ExportPkArray(loaded, "PowersTauDeltaEval") == groth16.ExportPkArray(pk, "PowersTauDeltaEval")
    assert groth_points(groth16.prove_from_witness(loaded, dev, inst.w, r, s)) == want and capi.last_timing()["fallbacks"] == 0


# ---- 6. Pinocchio -------------------------------------------------------------------------------------------------------------------
def lagrange_at(n, tau):
    """L_j(tau), j = 1..n, over the nodes 1..n"""
    fact = [1] * (n + 1)
    for k in range(1, n + 1):
        fact[k] = fact[k - 1] * k % R
    mt = 1
    for j in range(1, n + 1):
        mt = mt * (tau - j) % R
    out = []
    for j in range(1, n + 1):
        d = (tau - j) * fact[j - 1] % R * fact[n - j] % R
        if (n - j) % 2:
            d = R - d
        out.append(mt * pow(d, R - 2, R) % R)
    return out


def qap_at_tau(r1cs, n, w, lag):
    """(A(tau), B(tau), C(tau)) over the whole witness"""
    sums = []
    for rp, cl, vl in r1cs:
        rp, cl, vals = [int(x) for x in rp], [int(x) for x in cl], capi.u64_to_ints(vl)
        tot = 0
        for j in range(n):
            tot += sum(vals[e] * w[cl[e]] for e in range(rp[j], rp[j + 1])) % R * lag[j]
        sums.append(tot % R)
    return sums


def pin_points(p):
    return tuple(getattr(p, k) for k in snark.Proof.FIELDS)


def pin_witness_entry_points(pk, dev, w, w_host):
    first = pin_points(snark.prove_from_witness(pk, dev, w))
    tickets = [snark.prove_witness_begin(pk, dev, w) for _ in range(3)]
    assert all(pin_points(snark.prove_end(t)) == first for t in tickets)
    assert pin_points(snark.prove_end(snark.prove_witness_host_begin(pk, dev, w_host))) == first
    return first


@pytest.mark.parametrize("n", [33, 257])
@pytest.mark.parametrize("extra", [0, 1])
def test_pinocchio_derived_array_is_the_definition_equals_the_setups_and_proves_the_same(n, extra):
    inst = synth.sqchain_pinocchio_instance(n, 0xE600 + 2 * n + extra, extra)
    pk = inst.device_pk()
    want = snark.ExportPkArray(pk, "G1TEval")
    assert len(want) == n
    foreign = rebuilt_pinocchio_key(pk, inst.m, 1)
    assert capi.pk_eval_count(foreign.handle) == 0
    snark.DeriveEvalBasis(foreign, n)
    assert capi.pk_eval_count(foreign.handle) == n
    got = snark.ExportPkArray(foreign, "G1TEval")
    assert got == want
    assert affine_of(got) == naive_eval_basis(snark.ExportPkArray(foreign, "G1T"), n)
    dev = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
    proof = pin_witness_entry_points(pk, dev, inst.w, inst.w_host)
    assert pin_witness_entry_points(foreign, dev, inst.w, inst.w_host) == proof
    # PiH = H(tau) G with H Z = A B - C (snark.go:284-286), in closed form from the toxic tau
    T = inst.toxic[0]
    At, Bt, Ct = qap_at_tau(inst.r1cs, n, capi.u64_to_ints(inst.w_host), lagrange_at(n, T))
    zt = 1
    for k in range(1, inst.m - 1):
        zt = zt * (T - k) % R
    assert proof[6] == g1_multiple((At * Bt - Ct) * pow(zt, R - 2, R) % R)
    capi.set_eval_basis(False)
    assert pin_points(snark.prove_from_witness(foreign, dev, inst.w)) == proof


def test_pinocchio_uploaded_key_takes_the_setups_array_through_set_eval_basis():
    """snark.SetEvalBasis (gs_pinocchio_pk_set_eval): a foreign key uploaded with snark.UploadPk from the setup key's exported arrays,
    G1TEval attached as exported, proves field for field what the setup key proves -- on the witness route, the resident route and,
    as the DevicePk that UploadPk returns, through snark.prove_multi on one logical device."""
    n = 16
    inst = synth.sqchain_pinocchio_instance(n, 0xE700)
    pk = inst.device_pk()
    arrays = {k: snark.ExportPkArray(pk, k) for k in snark.PK_ARRAYS}
    assert len(arrays["G1TEval"]) == n == capi.pk_eval_count(pk)
    z = np.zeros((inst.m - 1, 4), dtype=np.uint64)
    capi.call("gs_pinocchio_pk_export", capi.raw(pk), 8, capi.ptr64(z), inst.m - 1)
    host = snark.Pk(Z=capi.u64_to_ints(z), **{k: arrays[k] for k in ("G1T", "A", "B", "C", "Kp", "Ap", "Bp", "Cp")})
    foreign = snark.UploadPk(host, snark.Circuit(inst.m, 1))
    assert isinstance(foreign, snark.DevicePk) and capi.pk_eval_count(foreign) == 0
    snark.SetEvalBasis(foreign, arrays["G1TEval"])
    assert capi.pk_eval_count(foreign) == capi.pk_eval_count(pk)
    assert snark.ExportPkArray(foreign, "G1TEval") == arrays["G1TEval"]
    dev = r1csqap.DeviceR1CS(*inst.r1cs, inst.m)
    want = pin_points(snark.prove_from_witness(pk, dev, inst.w))
    assert pin_points(snark.prove_from_witness(foreign, dev, inst.w)) == want
    assert pin_points(snark.prove_resident(foreign, inst.w, inst.px)) == want
    capi.comm_destroy()
    got, _ = snark.prove_multi([foreign], [inst.w], [inst.px])
    assert pin_points(got) == want
