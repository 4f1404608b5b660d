"""-m gpu: gs_r1cs_check -- which constraints does a witness break?  All n rows, in order, with their values, no key, beside proofs in
flight -- and the layers above it (DeviceR1CS.CheckWitness, circom.CheckWtns, GenerateProofsChecked).

Every expectation is Python integers (tests/r1cs_shapes.py: times, satisfied_system, standard_lengths) or plain index arithmetic on
systems of one entry per row; nothing the library computes is used as an expectation."""
import ctypes
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom, groth16, snark, r1csqap
import r1cs_shapes as S
from setup_util import Circuit
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = O.R
SENTINEL32, SENTINEL64 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)


def raw_check(dev, wh, cap, with_values=True):
    """gs_r1cs_check into arrays this test filled with a sentinel -> (status, count, rows [cap], values [cap, 3, 4]); count starts at 77"""
    count = ctypes.c_uint64(77)
    rows = np.full(max(cap, 1), SENTINEL32, dtype=np.uint32)
    values = np.full((max(cap, 1), 3, 4), SENTINEL64, dtype=np.uint64)
    rc = capi.load_library().gs_r1cs_check(capi.raw(dev), capi.raw(wh), cap, ctypes.byref(count), capi.ptr32(rows),
                                           capi.ptr64(values) if with_values else None)
    return rc, int(count.value), rows, values


def assert_report(dev, wh, cap, want_rows, want_values):
    """want_rows: every violated row, ascending; want_values(j) -> (a, b, c) integers"""
    rc, count, rows, values = raw_check(dev, wh, cap)
    assert rc == 0, capi.load_library().gs_last_error()
    assert count == len(want_rows)
    k = min(cap, count)
    assert rows[:k].tolist() == list(want_rows[:k])
    assert [tuple(capi.u64_to_ints(v)) for v in values[:k]] == [tuple(want_values(j)) for j in want_rows[:k]]
    assert (rows[k:] == SENTINEL32).all() and (values[k:] == SENTINEL64).all()       # nothing at and beyond min(cap, count) is written


# ---- 1, 2. positions: systems of one entry per row -------------------------------------------------------------------------
def one_entry_system(n):
    """Variables [one, x_0 .. x_{n-1}, y_0 .. y_{n-1}]; row j: x_j * one = y_j.  -> the three CSR triples, m"""
    m = 2 * n + 1
    rp = np.arange(n + 1, dtype=np.uint32)
    one = np.zeros((n, 4), dtype=np.uint64)
    one[:, 0] = 1
    idx = np.arange(n, dtype=np.uint32)
    return ((rp, idx + 1, one), (rp, np.zeros(n, dtype=np.uint32), one), (rp, idx + 1 + n, one)), m


def one_entry_witness(n, violated):
    """x_j = 3 j + 5, y_j = x_j, and y_j = x_j + 1 in the violated rows"""
    w = np.zeros((2 * n + 1, 4), dtype=np.uint64)
    x = 3 * np.arange(n, dtype=np.uint64) + 5
    w[0, 0] = 1
    w[1:n + 1, 0] = x
    w[n + 1:, 0] = x
    w[n + 1 + np.asarray(violated, dtype=np.int64), 0] += 1
    return w


def one_entry_values(j):
    return (3 * j + 5, 1, 3 * j + 6)


def patterns(n):
    out = {"none": [], "row_0": [0], "row_last": [n - 1], "every_row": list(range(n)), "odd_rows": list(range(1, n, 2))}
    if n >= 2049:
        out["tile_seam"] = [2047, 2048]
    return out


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4097])
def test_positions_counts_and_values_at_the_wave_workgroup_and_tile_edges(n):
    mats, m = one_entry_system(n)
    dev = r1csqap.DeviceR1CS(*mats, m)
    for name, violated in patterns(n).items():
        wh = capi.scalars_upload(one_entry_witness(n, violated))
        for cap in (0, 1, 16, n + 5):
            assert_report(dev, wh, cap, violated, one_entry_values)
        rc, count, rows, _ = raw_check(dev, wh, 16, with_values=False)         # values may be NULL
        assert rc == 0 and count == len(violated) and rows[:min(16, count)].tolist() == violated[:16], name


def test_beyond_1024_scan_tiles():
    """n = 2^21 + 1: 1025 tiles of the prefix sums, so the tile-sum stage holds two tile sums per thread"""
    n = (1 << 21) + 1
    violated = [0, (1 << 21) - 1, 1 << 21]
    mats, m = one_entry_system(n)
    dev = r1csqap.DeviceR1CS(*mats, m)
    wh = capi.scalars_upload(one_entry_witness(n, violated))
    for cap in (0, 2, 16):
        assert_report(dev, wh, cap, violated, one_entry_values)
    assert_report(dev, capi.scalars_upload(one_entry_witness(n, [])), 16, [], one_entry_values)


# ---- 3, 4. real row shapes -------------------------------------------------------------------------------------------------
_SAT = {}


def satisfied(extra):
    """tests/test_gpu_r1cs_shapes.py's `satisfied` fixture rebuilt: ladder rows in A, B and C of a satisfied system of n = 600, m = n + 1 +
    extra, and its four perturbed witnesses.  -> (n, m, mats, w, {name: bad witness}, failing)"""
    if extra not in _SAT:
        n = 600
        m = n + 1 + extra
        mats, w = S.satisfied_system(n, *(S.standard_lengths(n, n + 1, 500 + 3 * extra + k) for k in range(3)), 510 + extra, extra=extra,
                                     leaves=(1, n - 1, n))
        hub = int(np.argmax(np.bincount(mats[0][1], minlength=m)[3:])) + 3
        cases = {}
        for name, var in (("constraint_1", 1), ("root_dz", m - 2), ("constraint_n", n), ("hub_variable", hub)):
            bad = list(w)
            bad[var] = (bad[var] + 1) % R
            cases[name] = bad
        _SAT[extra] = (n, m, mats, w, cases)
    return _SAT[extra]


def products(mats, wit):
    """-> ([(a_j, b_j, c_j)] in Python integers, the 0-based rows with a b != c)"""
    abc = list(zip(*(S.times(mat, wit) for mat in mats)))
    return abc, [j for j, (a, b, c) in enumerate(abc) if a * b % R != c]


@pytest.mark.parametrize("extra", [0, 1], ids=["m=n+1", "m=n+2"])
def test_ladder_rows_report_what_the_python_products_say(extra):
    n, m, mats, w, cases = satisfied(extra)
    dev = r1csqap.DeviceR1CS(*mats, m)
    abc, rows = products(mats, w)
    assert rows == []
    assert_report(dev, capi.scalars_upload(S.ints_to_rows(w)), 16, [], abc.__getitem__)
    for name, bad in cases.items():
        abc, rows = products(mats, bad)
        assert rows and (name == "hub_variable" or rows == [{"constraint_1": 0, "root_dz": m - 3, "constraint_n": n - 1}[name]])
        bh = capi.scalars_upload(S.ints_to_rows(bad))
        for cap in (0, 16, n):
            assert_report(dev, bh, cap, rows, abc.__getitem__)
        report = dev.CheckWitness(bad, cap=n)
        assert not report and report.count == len(rows) and report.rows == rows and report.values == [abc[j] for j in rows]


def test_the_last_constraint_of_the_reference_shape_is_reported_while_the_prover_counts_none():
    """m = n + 1: Z has n - 1 roots, the key does not enforce constraint n, the prover's count is 0 -- this call names row n - 1"""
    n, m, mats, w, cases = satisfied(0)
    dev = r1csqap.DeviceR1CS(*mats, m)
    rng = random.Random(600)
    pk, _ = groth16.GenerateTrustedSetupSparse(n, m, 2, *mats, tuple(rng.randrange(1 << 20, R) for _ in range(5)))
    bh = capi.scalars_upload(S.ints_to_rows(cases["constraint_n"]))
    assert groth16.witness_values(pk, dev, bh)[1] == 0
    report = dev.CheckWitness(bh)
    assert report.count == 1 and report.rows == [n - 1]


def test_witness_entries_count_mod_r():
    """r or 2r added wherever the sum stays below 2^256: the same verdicts and the same canonical values"""
    n, m, mats, w, cases = satisfied(1)
    dev = r1csqap.DeviceR1CS(*mats, m)
    rng = random.Random(41)
    for wit in (w, cases["hub_variable"], cases["constraint_1"]):
        abc, rows = products(mats, wit)
        lifted = [x + k * R if x + k * R < (1 << 256) else x for x, k in ((x, rng.choice((1, 2))) for x in wit)]
        assert any(x >= 2 * R for x in lifted) and [x % R for x in lifted] == [x % R for x in wit]
        assert_report(dev, capi.scalars_upload(S.ints_to_rows(lifted)), n, rows, abc.__getitem__)


# ---- 5. equality is mod r --------------------------------------------------------------------------------------------------
def test_equality_is_decided_mod_r():
    """rows a_j * b_j = c_j over variables [one, a_0, b_0, c_0, a_1, ...]: a b - c = +1, a b - c = -1, a b = c + r as integers, a b = c"""
    rng = random.Random(5)
    a, b = rng.randrange(2, R), rng.randrange(2, R)
    half = (R + 1) // 2
    trip = [(a, b, (a * b - 1) % R), (a, b, (a * b + 1) % R), (2, half, 1), (a, b, a * b % R)]
    assert 2 * half == 1 + R
    w = [1] + [x for t in trip for x in t]
    rows = lambda k: [{1 + 3 * j + k: 1} for j in range(len(trip))]              # noqa: E731
    dev = r1csqap.DeviceR1CS(*(r1csqap.csr_from_rows(rows(k)) for k in range(3)), len(w))
    assert_report(dev, capi.scalars_upload(S.ints_to_rows(w)), 16, [0, 1], trip.__getitem__)


# ---- 6. the domain form ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(5, 3), (8, 3), (600, 10)])
def test_domain_systems_report_the_same_and_never_a_padded_row(n, k):
    mats, m = one_entry_system(n)
    node, dom = r1csqap.DeviceR1CS(*mats, m), circom.DeviceDomainR1CS(k, *mats, m)
    for name, violated in patterns(n).items():
        wh = capi.scalars_upload(one_entry_witness(n, violated))
        for cap in (0, 16, (1 << k) + 5):
            assert_report(dom, wh, cap, violated, one_entry_values)
            assert_report(node, wh, cap, violated, one_entry_values)
    if n == 600:
        _, _, lmats, w, cases = satisfied(0)
        abc, rows = products(lmats, cases["hub_variable"])
        assert_report(circom.DeviceDomainR1CS(k, *lmats, n + 1), capi.scalars_upload(S.ints_to_rows(cases["hub_variable"])), 1 << k, rows,
                      abc.__getitem__)


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
_ZKEY = {}


def zkey_case(tmp_path_factory):
    """a circuit of 3 constraints and 1 public input, its .r1cs, .wtns, a transcript and the .zkey set up from them"""
    if not _ZKEY:
        c = Circuit(3, 1, 3, 1031)
        d = tmp_path_factory.mktemp("r1cs_check")
        paths = {name: str(d / name) for name in ("c.r1cs", "t.ptau", "c.zkey", "good.wtns", "bad.wtns")}
        c.write_r1cs(paths["c.r1cs"])
        circom.WritePtau(paths["t.ptau"], 3, c.tau, c.alpha, c.beta)
        circom.SetupFromPtau(paths["c.r1cs"], paths["t.ptau"], paths["c.zkey"])
        bad = list(c.w)
        bad[-2] = (bad[-2] + 1) % R                   # the product of constraint 1 (0-based); later rows may read it
        circom.WriteWtns(paths["good.wtns"], c.w)
        circom.WriteWtns(paths["bad.wtns"], bad)
        _ZKEY["case"] = (c, paths, bad)
    return _ZKEY["case"]


def circuit_failing(c, wit):
    dot = lambda lc: sum(v * wit[s] for s, v in lc) % R                          # noqa: E731
    abc = [tuple(dot(lc) for lc in lcs) for lcs in c.constraints]
    return abc, [j for j, (a, b, cc) in enumerate(abc) if a * b % R != cc]


def test_refusals_write_nothing(tmp_path_factory):
    c, paths, bad = zkey_case(tmp_path_factory)
    lib = capi.load_library()
    untouched = lambda res: res[1] == 77 and (res[2] == SENTINEL32).all() and (res[3] == SENTINEL64).all()      # noqa: E731
    _, product = circom.UploadZkey(paths["c.zkey"])
    wh = capi.scalars_upload(S.ints_to_rows(c.w))
    res = raw_check(product, wh, 4)
    assert res[0] == -4 and untouched(res) and b".r1cs" in lib.gs_last_error() and b"no C" in lib.gs_last_error()
    with pytest.raises(capi.GosnarkHipError) as e:
        product.CheckWitness(c.w)
    assert e.value.code == -4 and ".r1cs" in str(e.value)
    mats, m = one_entry_system(5)
    dev = r1csqap.DeviceR1CS(*mats, m)
    good = capi.scalars_upload(one_entry_witness(5, [2]))
    for short in (capi.scalars_upload(np.zeros((m - 1, 4), dtype=np.uint64)), capi.scalars_upload(np.zeros((m + 1, 4), dtype=np.uint64))):
        res = raw_check(dev, short, 4)
        assert res[0] == -4 and untouched(res)
    for r1cs, w in ((good, good), (dev, dev), (0, good), (dev, 0)):              # wrong handle kinds
        res = raw_check(r1cs, w, 4)
        assert res[0] == -3 and untouched(res)
    count = ctypes.c_uint64(77)
    assert lib.gs_r1cs_check(capi.raw(dev), capi.raw(good), 4, ctypes.byref(count), None, None) == -3 and count.value == 77
    assert lib.gs_r1cs_check(capi.raw(dev), capi.raw(good), 0, None, None, None) == -3
    assert lib.gs_r1cs_check(capi.raw(dev), capi.raw(good), 0, ctypes.byref(count), None, None) == 0 and count.value == 1


# ---- 8. beside proofs in flight --------------------------------------------------------------------------------------------
def test_checks_beside_three_proofs_in_flight():
    n, m, mats, w, cases = satisfied(1)
    dev = r1csqap.DeviceR1CS(*mats, m)
    rng = random.Random(800)
    pk, _ = groth16.GenerateTrustedSetupSparse(n, m, 2, *mats, tuple(rng.randrange(1 << 20, R) for _ in range(5)))
    assert capi.pk_eval_count(pk) == n
    wits = [w, cases["constraint_1"], w]
    rs = [(rng.randrange(R), rng.randrange(R)) for _ in wits]
    handles = [capi.scalars_upload(S.ints_to_rows(x)) for x in wits]
    blocking = [groth16.prove_from_witness(pk, dev, h, r, s) for h, (r, s) in zip(handles, rs)]
    bad_abc, bad_rows = products(mats, cases["hub_variable"])
    bh, gh = capi.scalars_upload(S.ints_to_rows(cases["hub_variable"])), capi.scalars_upload(S.ints_to_rows(w))
    tickets = [groth16.prove_witness_begin(pk, dev, h, r, s) for h, (r, s) in zip(handles, rs)]
    got_bad = capi.r1cs_check(dev, bh, n)
    capi.scalars_update(bh, S.ints_to_rows(w))                # right behind the check: must not reach into its report
    got_good = capi.r1cs_check(dev, gh, 16)
    proofs = [groth16.prove_end(t) for t in tickets]
    assert got_bad[0] == len(bad_rows) and got_bad[1].tolist() == bad_rows
    assert [tuple(capi.u64_to_ints(v)) for v in got_bad[2]] == [bad_abc[j] for j in bad_rows]
    assert got_good[0] == 0 and len(got_good[1]) == 0
    assert [(p.PiA, p.PiB, p.PiC) for p in proofs] == [(p.PiA, p.PiB, p.PiC) for p in blocking]
    assert capi.r1cs_check(dev, bh, 0)[0] == 0                # the updated vector is the good witness now


# ---- 9. GenerateProofsChecked, CheckWtns -----------------------------------------------------------------------------------
def test_generate_proofs_checked_groth16_and_pinocchio():
    n, m, mats, w, cases = satisfied(0)
    dev = r1csqap.DeviceR1CS(*mats, m)
    rng = random.Random(900)
    r, s = rng.randrange(R), rng.randrange(R)
    bad = cases["constraint_n"]                                # the one the prover's own count cannot see
    pk, _ = groth16.GenerateTrustedSetupSparse(n, m, 2, *mats, tuple(rng.randrange(1 << 20, R) for _ in range(5)))
    want = groth16.GenerateProofsFromWitnessWithRS(None, pk, dev, w, r, s)
    got = groth16.GenerateProofsChecked(None, pk, dev, w, r, s)
    assert (got.PiA, got.PiB, got.PiC) == (want.PiA, want.PiB, want.PiC)
    with pytest.raises(r1csqap.WitnessError) as e:
        groth16.GenerateProofsChecked(None, pk, dev, bad, r, s)
    assert e.value.report.rows == [n - 1] and e.value.report.count == 1 and capi.last_timing()["fallbacks"] == 0
    abc, rows = products(mats, cases["hub_variable"])
    with pytest.raises(r1csqap.WitnessError) as e:
        groth16.GenerateProofsChecked(None, pk, dev, cases["hub_variable"], r, s)
    assert e.value.report.count == len(rows) and e.value.report.rows == rows[:16] and capi.last_timing()["fallbacks"] == 0
    ppk, _ = snark.GenerateTrustedSetupSparse(n, m, 2, *mats, tuple(rng.randrange(1 << 20, R) for _ in range(8)))
    pwant, pgot = snark.GenerateProofsFromWitness(None, ppk, dev, w), snark.GenerateProofsChecked(None, ppk, dev, w)
    assert all(getattr(pgot, k) == getattr(pwant, k) for k in snark.Proof.FIELDS)
    with pytest.raises(r1csqap.WitnessError) as e:
        snark.GenerateProofsChecked(None, ppk, dev, bad)
    assert e.value.report.rows == [n - 1] and capi.last_timing()["fallbacks"] == 0


def test_a_zkey_key_refuses_through_the_r1cs_system_and_check_wtns_reads_the_files(tmp_path_factory):
    c, paths, bad = zkey_case(tmp_path_factory)
    abc, rows = circuit_failing(c, bad)
    assert rows and circuit_failing(c, c.w)[1] == []
    good_report, bad_report = circom.CheckWtns(paths["c.r1cs"], paths["good.wtns"]), circom.CheckWtns(paths["c.r1cs"], paths["bad.wtns"])
    assert good_report and good_report.count == 0 and good_report.rows == []
    assert not bad_report and bad_report.rows == rows and bad_report.values == [abc[j] for j in rows]
    parsed = circom.ReadR1cs(paths["c.r1cs"])
    for i, j in enumerate(rows):
        assert bad_report.explain(i, parsed) == tuple([(sig, v % R, bad[sig]) for sig, v in lc] for lc in c.constraints[j])
    key, system = circom.UploadZkey(paths["c.zkey"])
    vk = circom.VerificationKeyFromZkey(paths["c.zkey"])
    full = circom._setup_system(parsed, circom._setup_domain_bits(parsed))
    public = c.w[1:c.npub + 1]
    want = circom.GenerateProofsWithRS(key, system, c.w, 3, 4)
    got = circom.GenerateProofsChecked(key, system, c.w, full, 3, 4)
    assert (got.PiA, got.PiB, got.PiC) == (want.PiA, want.PiB, want.PiC) and circom.VerifyFromCircom(vk, got, public)
    with pytest.raises(r1csqap.WitnessError) as e:
        circom.GenerateProofsChecked(key, system, bad, full, 3, 4)
    assert e.value.report.rows == rows
    assert not circom.VerifyFromCircom(vk, circom.GenerateProofsWithRS(key, system, bad, 3, 4), public)      # the unchecked call still proves
    with pytest.raises(capi.GosnarkHipError) as e:
        circom.GenerateProofsChecked(key, system, c.w)           # no .r1cs system: the product system itself cannot be checked
    assert e.value.code == -4
