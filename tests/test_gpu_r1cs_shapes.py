"""-m gpu: the sparse R1CS kernels (k_spmv, k_spmv_long, k_r1cs_check, the setups' transposed product and scalar kernels) on the
row shapes real front ends emit, against Python integers (tests/r1cs_shapes.py).

Rows of 0 .. ncols entries around every seam of the device product (the 256-thread tile, the 512 / 513 hand-off to the
one-workgroup-per-row kernel, more long rows than that kernel has workgroups, more than its hand-off list holds), column indices
unsorted and repeated, values and witness entries anywhere in [0, 2^256).  Every comparison is equality of integers mod r or of
affine coordinates; the table policy stays at the library's default."""
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, groth16, snark, r1csqap
import r1cs_shapes as S
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = O.R
INF1 = (0, 0, 0)


@pytest.fixture(scope="module", autouse=True)
def _init():
    capi.init()


def witness(m, seed):
    """[1, ...]: uniform elements, a third of them lifted into [r, 2^256), plus the corner values"""
    rng = random.Random(seed)
    w = [1] + [rng.randrange(R) for _ in range(m - 1)]
    for i in range(2, m, 3):
        w[i] += R * rng.randint(1, ((1 << 256) - 1 - w[i]) // R)
    for i, v in zip(range(3, m, max(1, m // 7)), (0, R, R + 1, 2 * R - 1, (1 << 256) - 1, R - 1)):
        w[i] = v
    return w


def expected_polys(mats, w):
    """ax, bx, cx by the C oracle's interpolation of the Python products, px = ax * bx - cx by its schoolbook product"""
    ax, bx, cx = (C.lagrange(S.times(mat, w)) for mat in mats)
    prod = C.poly_mul(ax, bx)
    return ax, bx, cx, [(p - (cx[i] if i < len(cx) else 0)) % R for i, p in enumerate(prod)]


def px_host(mats, w, m):
    return tuple(capi.u64_to_ints(x) for x in r1csqap.ComputePx(*mats, S.ints_to_rows(w), m))


def px_resident(dev, wh, px=None):
    px = dev.ComputePxResident(wh, px)
    return px, capi.u64_to_ints(capi.scalars_download(px))


# ---- (a) the forward product A w -----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def forward():
    n, m = 700, 1100
    mats = [S.ladder_csr(n, m, S.standard_lengths(n, m, 11 + k), 21 + k, cls) for k, cls in enumerate(("canonical", "mixed", "noncanonical"))]
    for rp, _, _ in mats:
        assert int((np.diff(rp.astype(np.int64)) > S.LONG_ROW).sum()) >= 130 + 2 * 9
    w = witness(m, 31)
    return n, m, mats, w, expected_polys(mats, w)


def test_forward_product_from_host_buffers_equals_the_python_products_interpolated(forward):
    n, m, mats, w, want = forward
    got = px_host(mats, w, m)
    for name, g, e in zip(("ax", "bx", "cx", "px"), got, want):
        assert g == e, name


def test_forward_product_of_a_resident_system_overwrites_its_px_handle(forward):
    """gs_r1cs_px hands out px alone (ax, bx, cx stay inside the library); px = ax * bx - cx with all three from the ladder rows.
    The second and third call write into the handle of the first: all zeros for the zero witness, px again for w mod r."""
    n, m, mats, w, want = forward
    dev = r1csqap.DeviceR1CS(*mats, m)
    px, got = px_resident(dev, capi.scalars_upload(S.ints_to_rows(w)))
    assert got == want[3]
    same, got = px_resident(dev, capi.scalars_upload(np.zeros((m, 4), dtype=np.uint64)), px)
    assert same is px and got == [0] * (2 * n - 1)
    same, got = px_resident(dev, capi.scalars_upload(S.ints_to_rows([x % R for x in w])), px)
    assert same is px and got == want[3]


def degenerate(case):
    """small systems at the edges of the CSR format; every one still holds rows on both sides of the 512 / 513 seam"""
    n, m = 40, 600
    if case == "one_constraint":
        n, m = 1, 3
        mats = [S.ladder_csr(1, 3, [k], 40 + k, "mixed") for k in (3, 2, 0)]
        return n, m, mats
    lengths = [S.standard_lengths(n, m, 50 + k, repeats=1, nlong=5) for k in range(3)]
    mats = [S.ladder_csr(n, m, lengths[k], 60 + k, "mixed") for k in range(3)]
    if case == "no_entries":                       # A = 0: ax = 0, px = -cx
        mats[0] = (np.zeros(n + 1, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros((0, 4), dtype=np.uint64))
    elif case == "last_row_only":                  # a long, a short and a seam row, each alone at the end of its matrix
        mats = [S.ladder_csr(n, m, [0] * (n - 1) + [k], 70 + k, "mixed") for k in (600, 3, 513)]
    elif case == "unreferenced_column":            # no row names column 7: whatever the witness holds there must not matter
        skip7 = np.array([k for k in range(m) if k != 7], dtype=np.uint32)
        mats = [S.ladder_csr(n, m, [min(x, m - 1) for x in lengths[k]], 80 + k, "mixed", [m - 1] * n, skip7) for k in range(3)]
        assert not any((mat[1] == 7).any() for mat in mats)
    elif case == "last_column_in_a_long_row":
        for rp, col, _ in mats:
            j = int(np.argmax(np.diff(rp.astype(np.int64))))
            col[int(rp[j + 1]) - 1] = m - 1
            col[int(rp[j]) + 300] = m - 1
    return n, m, mats


@pytest.mark.parametrize("case", ["no_entries", "one_constraint", "last_row_only", "unreferenced_column", "last_column_in_a_long_row"])
def test_forward_product_on_degenerate_matrices(case):
    n, m, mats = degenerate(case)
    w = witness(m, 90)
    want = expected_polys(mats, w)
    got = px_host(mats, w, m)
    for name, g, e in zip(("ax", "bx", "cx", "px"), got, want):
        assert g == e, name
    if case == "no_entries":
        assert got[0] == [0] * n
    assert px_resident(r1csqap.DeviceR1CS(*mats, m), capi.scalars_upload(S.ints_to_rows(w)))[1] == want[3]


# ---- (b) more long rows than the hand-off list holds -----------------------------------------------------------------------
def test_rows_beyond_the_hand_off_list_are_summed_all_the_same():
    """4100 of A's 4200 rows have 513..600 entries, the list from k_spmv to k_spmv_long holds 4096: the rest (which ones is up to an
    atomic) are summed by single threads.  Every row is checked at once by sum_j (A w)_j L_j(x) == ax(x) at two seeded points
    outside the nodes: one wrong or unwritten row breaks it except with probability about 1 / r."""
    n, m = 4200, 640
    rng = random.Random(0xCA9)
    long_rows = [rng.randint(513, 600) for _ in range(4100)]
    rest = [S.LADDER[i % 10] for i in range(n - 4100)]                  # 0 .. 513 again
    la = long_rows + rest
    rng.shuffle(la)
    mats = [S.ladder_csr(n, m, la, 101, "mixed"),
            S.ladder_csr(n, m, [rng.randint(0, 3) for _ in range(n)], 102, "noncanonical"),
            S.ladder_csr(n, m, [rng.randint(0, 3) for _ in range(n)], 103, "canonical")]
    assert sum(x > S.LONG_ROW for x in la) >= 4100 > 4096 and int(mats[0][0][-1]) > 2_200_000
    w = witness(m, 104)
    vals = [S.times(mat, w) for mat in mats]
    ax, bx, cx, px = px_host(mats, w, m)
    for x in (rng.randrange(n + 1, R), rng.randrange(n + 1, R)):
        lag = S.lagrange_at(n, x)
        at = [S.horner(p, x) for p in (ax, bx, cx)]
        for name, v, e in zip("abc", vals, at):
            assert sum(map(int.__mul__, v, lag)) % R == e, name
        assert S.horner(px, x) == (at[0] * at[1] - at[2]) % R
    assert max(ax + bx + cx + px) < R


# ---- (c) the transposed product and the scalar kernels of both setups -------------------------------------------------------
def g1_multiples(ks):
    v = capi.u64_to_ints(capi.g1_download(capi.g1_fixed_base(S.ints_to_rows([k % R for k in ks]))))
    return [tuple(v[3 * i:3 * i + 3]) for i in range(len(ks))]


def g2_multiples(ks):
    v = capi.u64_to_ints(capi.g2_download(capi.g2_fixed_base(S.ints_to_rows([k % R for k in ks]))))
    return [((v[6 * i], v[6 * i + 1]), (v[6 * i + 2], v[6 * i + 3]), (v[6 * i + 4], v[6 * i + 5])) for i in range(len(ks))]


@pytest.fixture(scope="module", params=[(0, 1), (1, 3)], ids=["m=n+1,NPublic=1", "m=n+2,NPublic=3"])
def transposed(request):
    """the VARIABLES follow the ladder: 0, 1, .., 512, 513, .., n constraints each, and 130 more above 512"""
    extra, npublic = request.param
    n = 1200
    m = n + 1 + extra
    mats = [S.transpose_ladder(n, m, S.standard_lengths(m, n, 200 + 3 * extra + k), 210 + 3 * extra + k, cls)
            for k, cls in enumerate(("mixed", "noncanonical", "canonical"))]
    for _, col, _ in mats:
        assert int((np.bincount(col, minlength=m) > S.LONG_ROW).sum()) >= 130 + 2 * 9
    return n, m, npublic, mats


def columns_at(mats, n, m, tau):
    lag = S.lagrange_at(n, tau)
    return [S.times_transposed(mat, m, lag) for mat in mats]


def z_at(m, tau):
    zt = 1
    for k in range(1, m - 1):
        zt = zt * (tau - k) % R
    return zt


def test_groth16_setup_on_ladder_columns_equals_the_reference_formulas(transposed):
    """groth16.go:139-175 and :177-219 as oracle/ref_py.py restates them, on at_i = sum_j A[j][i] L_j(tau) from Python integers; the
    points through the fixed-base route that tests/test_gpu_msm.py pins to the oracle's MulScalar."""
    n, m, npublic, mats = transposed
    rng = random.Random(300 + m)
    toxic = T, Ka, Kb, Kg, Kd = tuple(rng.randrange(n + 1, R) for _ in range(5))
    at, bt, ct = columns_at(mats, n, m, T)
    pk, vk = groth16.GenerateTrustedSetupSparse(n, m, npublic, *mats, toxic)
    inv_d, inv_g = pow(Kd, R - 2, R), pow(Kg, R - 2, R)
    bac = [(at[i] * Kb + bt[i] * Ka + ct[i]) % R for i in range(m)]
    ztd = z_at(m, T) * inv_d % R
    assert groth16.ExportPkArray(pk, "G1_At") == g1_multiples(at)
    assert groth16.ExportPkArray(pk, "G1_BACGamma") == g1_multiples(bt)
    assert groth16.ExportPkArray(pk, "G2_BACGamma") == g2_multiples(bt)
    assert groth16.ExportPkArray(pk, "BACDelta") == [INF1] * (npublic + 1) + g1_multiples([x * inv_d for x in bac[npublic + 1:]])
    assert groth16.ExportPkArray(pk, "PowersTauDelta") == g1_multiples([pow(T, i, R) * ztd for i in range(m - 1)])
    assert vk.IC == g1_multiples([x * inv_g for x in bac[:npublic + 1]])
    assert [vk.G1_Alpha] == g1_multiples([Ka]) and [vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta] == g2_multiples([Kb, Kg, Kd])


def test_pinocchio_setup_on_ladder_columns_equals_the_reference_formulas(transposed):
    """snark.go:150-240 as oracle/ref_py.py restates it, on the same Python scalars."""
    n, m, npublic, mats = transposed
    rng = random.Random(400 + m)
    toxic = T, Ka, Kb, Kc, Kbeta, Kgamma, RhoA, RhoB = tuple(rng.randrange(n + 1, R) for _ in range(8))
    RhoC = RhoA * RhoB % R
    at, bt, ct = columns_at(mats, n, m, T)
    pk, vk = snark.GenerateTrustedSetupSparse(n, m, npublic, *mats, toxic)
    sa, sb, sc = [RhoA * x % R for x in at], [RhoB * x % R for x in bt], [RhoC * x % R for x in ct]
    a_pts, ap_pts = g1_multiples(sa), g1_multiples([Ka * x for x in sa])
    hidden = [INF1] * (npublic + 1)                   # resident A / Ap carry infinity for i <= NPublic (what snark.go:265 sums)
    assert snark.ExportPkArray(pk, "A") == hidden + a_pts[npublic + 1:]
    assert snark.ExportPkArray(pk, "Ap") == hidden + ap_pts[npublic + 1:]
    assert snark.ExportPkArray(pk, "B") == g2_multiples(sb)
    assert snark.ExportPkArray(pk, "Bp") == g1_multiples([Kb * x for x in sb])
    assert snark.ExportPkArray(pk, "C") == g1_multiples(sc)
    assert snark.ExportPkArray(pk, "Cp") == g1_multiples([Kc * x for x in sc])
    assert snark.ExportPkArray(pk, "Kp") == g1_multiples([Kbeta * (x + y + z) for x, y, z in zip(sa, sb, sc)])
    assert snark.ExportPkArray(pk, "G1T") == g1_multiples([pow(T, i, R) for i in range(m - 1)])
    assert vk.IC == a_pts[:npublic + 1]
    kbg = Kbeta * Kgamma % R
    assert [vk.Vkb, vk.G1Kbg] == g1_multiples([Kb, kbg])
    assert [vk.Vka, vk.Vkc, vk.G2Kbg, vk.G2Kg, vk.Vkz] == g2_multiples([Ka, Kc, kbg, Kgamma, RhoC * z_at(m, T)])


# ---- (d) the violation count and the witness route ---------------------------------------------------------------------------
@pytest.fixture(scope="module", params=[0, 1], ids=["m=n+1", "m=n+2"])
def satisfied(request):
    """ladder rows in A, B and C of a satisfied system; the perturbed witnesses with the constraints that, by `times`, fail.
    NPublic = 2: v_1 (in constraint 1 alone, in C) and v_2 (in rows of A, B and C)."""
    extra = request.param
    n = 600
    m = n + 1 + extra
    dz = m - 2
    mats, w = S.satisfied_system(n, *(S.standard_lengths(n, n + 1, 500 + 3 * extra + k) for k in range(3)), 510 + extra, extra=extra,
                                 leaves=(1, n - 1, n))

    def failing(wit):
        va, vb, vc = (S.times(mat, wit) for mat in mats)
        return [j + 1 for j in range(n) if va[j] * vb[j] % R != vc[j]]

    assert failing(w) == [] and all((mat[1] == 2).any() for mat in mats)
    hub = int(np.argmax(np.bincount(mats[0][1], minlength=m)[3:])) + 3        # the variable in the most A rows (not `one`, not public)
    cases = {}
    for name, var, fails in (("constraint_1", 1, [1]), ("root_dz", dz, [dz]), ("constraint_n", n, [n]), ("hub_variable", hub, None)):
        bad = list(w)
        bad[var] = (bad[var] + 1) % R
        rows = failing(bad)
        assert fails is None or rows == fails
        cases[name] = (bad, sum(j <= dz for j in rows))
    assert cases["hub_variable"][1] >= 200 and cases["constraint_n"][1] == (0 if extra == 0 else 1)
    return n, m, dz, mats, w, cases


def groth_points(p):
    return (p.PiA, p.PiB, p.PiC)


def pino_points(p):
    return tuple(getattr(p, k) for k in snark.Proof.FIELDS)


def check_witness_route(satisfied, setup, values, by_px, by_witness, piped, points, verify, binds_c, same_proof):
    """binds_c: the verifier binds a public input that occurs in C alone.  same_proof: the (case, deg Z == n) pairs whose perturbed
    witness must give the very proof of w -- every other one must give another."""
    n, m, dz, mats, w, cases = satisfied
    dev = r1csqap.DeviceR1CS(*mats, m)
    pk, vk = setup(n, m, mats)
    wh = capi.scalars_upload(S.ints_to_rows(w))
    assert values(pk, dev, wh)[1] == 0
    want = points(by_px(pk, wh, dev.ComputePxResident(wh)))
    for on in (True, False):                   # H's values against the evaluation-basis array / H's coefficients
        capi.set_eval_basis(on)
        try:
            got = by_witness(pk, dev, wh)
            assert capi.last_timing()["fallbacks"] == 0
            assert points(got) == want and points(piped(pk, dev, wh)) == want, on
        finally:
            capi.set_eval_basis(True)
    assert verify(vk, got, [w[1], w[2]]) is True
    assert verify(vk, got, [w[1], (w[2] + 1) % R]) is False
    assert verify(vk, got, [(w[1] + 1) % R, w[2]]) is (not binds_c)
    for name, (bad, count) in cases.items():
        bh = capi.scalars_upload(S.ints_to_rows(bad))
        assert values(pk, dev, bh)[1] == count, name
        exact = points(by_px(pk, bh, dev.ComputePxResident(bh)))
        assert points(by_witness(pk, dev, bh)) == exact, name
        assert capi.last_timing()["fallbacks"] == (1 if count else 0), name
        assert points(piped(pk, dev, bh)) == exact, name
        assert (exact == want) == ((name, dz == n) in same_proof), name
    assert verify(vk, by_witness(pk, dev, bh), bad[1:3]) is False                   # (the last case: hundreds of violated constraints)


def test_groth16_witness_route_and_violation_count_on_ladder_rows(satisfied):
    """Two perturbed witnesses give the proof of w itself, and that is arithmetic, not a lost update: v_n at deg Z = n - 1 moves px by
    d L_n(x) = d Z(x) / Z(n), so H moves by d / Z(n) and PiC by d (L_n(tau) - Z(tau) / Z(n)) / delta = 0 (constraint n is outside Z: the
    reference's gap); the public v_1 has At = BACGamma = 0 and BACDelta = infinity, and at deg Z = n the floor
    quotient of px + d L_1(x) (degree n - 1) is that of px.  At deg Z = n - 1 the same d L_1(x) moves H's constant term."""
    rng = random.Random(600)
    toxic = tuple(rng.randrange(1 << 20, R) for _ in range(5))
    r, s = rng.randrange(R), rng.randrange(R)
    check_witness_route(
        satisfied,
        setup=lambda n, m, mats: groth16.GenerateTrustedSetupSparse(n, m, 2, *mats, toxic),
        values=groth16.witness_values,
        by_px=lambda pk, wh, px: groth16.prove_resident(pk, wh, px, r, s),
        by_witness=lambda pk, dev, wh: groth16.prove_from_witness(pk, dev, wh, r, s),
        piped=lambda pk, dev, wh: groth16.prove_end(groth16.prove_witness_begin(pk, dev, wh, r, s)),
        points=groth_points, verify=groth16.VerifyProof, binds_c=True, same_proof={("constraint_n", False), ("constraint_1", True)})


def test_pinocchio_witness_route_and_violation_count_on_ladder_rows(satisfied):
    """snark.go's Vk.IC holds the A points alone, so a public input that occurs only in C (v_1) is not bound by the verifier; PiC sums
    w_i C_i over every i, so every perturbed witness gives another proof."""
    rng = random.Random(700)
    toxic = tuple(rng.randrange(1 << 20, R) for _ in range(8))
    check_witness_route(
        satisfied,
        setup=lambda n, m, mats: snark.GenerateTrustedSetupSparse(n, m, 2, *mats, toxic),
        values=snark.witness_values,
        by_px=snark.prove_resident,
        by_witness=snark.prove_from_witness,
        piped=lambda pk, dev, wh: snark.prove_end(snark.prove_witness_begin(pk, dev, wh)),
        points=pino_points, verify=snark.VerifyProof, binds_c=False, same_proof=set())
