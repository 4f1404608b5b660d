"""-m gpu: gs_r1cs_solve_plan / gs_r1cs_solve -- witnesses solved from the system on the device -- and the layers above them
(DeviceR1CS.PlanSolve, SolvePlan.Solve, GenerateProofsFromInputs).

Every expectation is Python integers from tests/solve_util.py, which restates the level plan the slow way and evaluates the three
formulas; nothing the library computes is used as an expectation."""
import ctypes
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom, groth16, snark, r1csqap, synth
import solve_util as SU
from setup_util import Circuit
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = SU.R
SENTINEL32, SENTINEL64 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE
NONE = 0xFFFFFFFF


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)


def upload(system):
    A, B, C, m, inputs = system
    return r1csqap.DeviceR1CS(SU.csr(A), SU.csr(B), SU.csr(C), m)


def expect(system, values, p=None):
    A, B, C, m, inputs = system
    return SU.solve(A, B, C, m, inputs, values, p)


def assert_solves(system, batch, narrow=0, run_max_rows=0, into=None, dev=None):
    """batch: one list of input values per witness.  Every entry of every witness, nfailed and first_failed_row against integers."""
    A, B, C, m, inputs = system
    dev = dev or upload(system)
    plan = dev.PlanSolve(inputs, narrow, run_max_rows)
    want_plan = SU.plan(A, B, C, m, inputs)
    assert plan.unsolved() == want_plan["unsolved"]
    assert (plan.stats["solved"], plan.stats["checks"], plan.stats["stuck"], plan.stats["levels"]) == \
        (len(want_plan["entries"]), want_plan["checks"], want_plan["stuck"], len(want_plan["levels"]) - 1)
    handles, report = plan.Solve(batch, into)
    got = [capi.u64_to_ints(capi.scalars_download(h)) for h in handles]
    for b, values in enumerate(batch):
        w, nfailed, first = SU.solve(A, B, C, m, inputs, values, want_plan)
        assert got[b] == w, "witness %d" % b
        assert (report.nfailed[b], report.first_failed_row[b]) == (nfailed, first), "witness %d" % b
    return plan, handles, got


def inputs_for(nwit, seed, ninputs=1):
    rng = random.Random(seed)
    return [[rng.randrange(R) for _ in range(ninputs)] for _ in range(nwit)]


# ---- the reference's own circuit -----------------------------------------------------------------------------------------------
def x3():
    dense = lambda M: [[(v, c) for v, c in enumerate(row) if c] for row in M]      # noqa: E731
    return dense(O.X3_R1CS_A), dense(O.X3_R1CS_B), dense(O.X3_R1CS_C), 8, [2]


def test_x3_with_input_3_gives_the_reference_witness():
    plan, _, got = assert_solves(x3(), [[3]])
    assert got[0] == O.X3_WITNESS and plan.stats["levels"] == 5 and plan.stats["checks"] == 1


# ---- one level: rows x witnesses -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nrows", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_one_level_rows_times_witnesses(nrows):
    system = SU.independent(nrows)
    dev, m = upload(system), system[3]
    for nwit in (1, 2, 63, 64, 65, 130):
        plan, _, _ = assert_solves(system, inputs_for(nwit, 100 * nrows + nwit), dev=dev)
        assert plan.stats["levels"] == 1 and plan.stats["widest_level"] == nrows
    # overwrite: vectors of a sentinel end with none of it left (every one of their m elements is compared with the integers).  An
    # overwrite vector holds exactly m elements, so there is nothing of its own beyond them; the separate sentinel vector only shows
    # that the call does not write through another handle of the context -- where the allocator puts it is not in the test's hands
    fill = np.full((m, 4), SENTINEL64, dtype=np.uint64)
    into = [capi.scalars_upload(fill), None, capi.scalars_upload(fill)]
    guard = capi.scalars_upload(fill)
    _, handles, got = assert_solves(system, inputs_for(3, 7), into=into, dev=dev)
    assert handles[0] is into[0] and handles[2] is into[2] and len(handles[1]) == m
    assert (capi.scalars_download(guard) == SENTINEL64).all() and all(len(g) == m for g in got)


# ---- seams between wide launches and runs --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["widths", "chain16", "chain17", "chain33"])
def test_seams_and_defaults_agree(name):
    system = {"widths": SU.widths([3, 4, 5, 1, 1, 1, 6, 2, 2, 4, 1]), "chain16": SU.chain(16), "chain17": SU.chain(17),
              "chain33": SU.chain(33)}[name]
    dev = upload(system)
    batch = inputs_for(66, 31)
    plan, _, got = assert_solves(system, batch, narrow=4, run_max_rows=16, dev=dev)
    levels = SU.plan(*system)["levels"]
    want = SU.launches(levels, 4, 16)
    assert plan.stats["launches"] == len(want) and plan.stats["wide_launches"] == sum(1 for x in want if not x[2])
    _, _, again = assert_solves(system, batch, dev=dev)
    assert again == got
    _, _, wide_only = assert_solves(system, batch, narrow=1, dev=dev)          # narrow = 1: no level is narrower, no run at all
    assert wide_only == got


# ---- forms and coefficients ----------------------------------------------------------------------------------------------------
def forms_system():
    """variables: one, x, y | c1, c2, c3, qa, qb, s, d.  C coefficients 1, 2, r - 1; out * v = u in A and in B; a 600-entry sum; duplicate
    columns"""
    A = [[(1, 1)], [(1, 1)], [(1, 1)], [(6, 3)], [(1, 1)], [(1, 1)] * 300 + [(2, R - 2)] * 300, [(1, 5), (1, R - 2), (2, 1)]]
    B = [[(2, 1)], [(2, 1)], [(2, 1)], [(1, 1)], [(7, 5)], [(0, 1)], [(0, 2), (0, 5)]]
    C = [[(3, 1)], [(4, 2)], [(5, R - 1)], [(2, 1)], [(2, 1)], [(8, 1)], [(9, 3), (9, 4)]]
    return A, B, C, 10, [1, 2]


def test_forms_coefficients_long_rows_duplicates_and_lifted_inputs():
    system = forms_system()
    dev = upload(system)
    rng = random.Random(5)
    batch = [[rng.randrange(1, R), rng.randrange(1, R)] for _ in range(5)]
    _, _, got = assert_solves(system, batch, dev=dev)
    lifted = [[x + R, y + 2 * R] for x, y in batch]                       # any value below 2^256 counts mod r
    _, _, again = assert_solves(system, lifted, dev=dev)
    assert again == got and all(max(w) < R for w in got)
    x, y = batch[0]
    assert got[0][3] == x * y % R and got[0][4] == x * y * pow(2, R - 2, R) % R and got[0][5] == (R - x * y) % R
    assert got[0][6] * 3 * x % R == y and x * 5 * got[0][7] % R == y and got[0][8] == (300 * x - 600 * y) % R
    # sqchain's own rows, {one: -k, s: 1} in C
    a, b, c, w = synth.sqchain_r1cs(40, 11)
    chain = (SU.from_csr(a), SU.from_csr(b), SU.from_csr(c), 41, [1])
    _, _, got = assert_solves(chain, [[11], [R - 1]])
    assert got[0] == capi.u64_to_ints(w)


# ---- zero divisors -------------------------------------------------------------------------------------------------------------
def test_a_zero_divisor_fails_its_witness_alone():
    # one, x, y | q: q * x = y;  t: t = q + y.   x = 0 makes the divisor zero
    A = [[(3, 1)], [(3, 1), (2, 1)]]
    B = [[(1, 1)], [(0, 1)]]
    C = [[(2, 1)], [(4, 1)]]
    system = (A, B, C, 5, [1, 2])
    batch = inputs_for(65, 3, 2)
    batch[0][0], batch[64][0] = 0, R                                      # r counts as 0
    dev = upload(system)
    plan = dev.PlanSolve(system[4])
    nwit = len(batch)
    handles, nfailed, first = capi.r1cs_solve(plan.handle, batch)
    for b in range(nwit):
        w, nf, fr = expect(system, batch[b])
        assert capi.u64_to_ints(capi.scalars_download(handles[b])) == w
        assert (nfailed[b], first[b]) == ((1, 0) if b in (0, 64) else (0, None)) == (nf, fr)
    _, report = plan.Solve(batch)
    assert not report and report.nfailed[0] == 1 and "zero divisor" in repr(report)


# ---- partly solvable -----------------------------------------------------------------------------------------------------------
def test_partly_solvable_system():
    A = [[(1, 1)], [(2, 1)], [(2, 1)], [(3, 1)]]
    B = [[(1, 1)], [(2, 1)], [(1, 1)], [(1, 1)]]
    C = [[(3, 1)], [(3, 1)], [(4, 1)], [(5, 1)]]
    plan, _, got = assert_solves((A, B, C, 6, [1]), inputs_for(3, 9))
    assert plan.unsolved() == [2, 4] and all(w[2] == 0 and w[4] == 0 and w[5] == w[1] ** 3 % R for w in got)
    _, report = plan.Solve([[5]])
    assert not report and report.unsolved == [2, 4]


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def raw_plan(dev, inputs):
    cell, stats = capi.Handle(77), capi.SolveStats()
    ctypes.memset(ctypes.byref(stats), 0xEE, ctypes.sizeof(stats))
    iv = np.asarray(inputs, dtype=np.uint32)
    rc = capi.load_library().gs_r1cs_solve_plan(capi.raw(dev), capi.ptr32(iv), iv.size, None, ctypes.byref(cell), ctypes.byref(stats))
    return rc, cell.value == 77 and stats.solved == SENTINEL64 and stats.widest_level == SENTINEL64


def raw_solve(plan, nwit, handles):
    hs = (capi.Handle * nwit)(*[capi.raw(h) for h in handles])
    nfailed, first = np.full(nwit, SENTINEL64, dtype=np.uint64), np.full(nwit, SENTINEL32, dtype=np.uint32)
    inputs = capi.ints_to_u64([3] * max(nwit, 1))
    rc = capi.load_library().gs_r1cs_solve(capi.raw(plan), nwit, capi.ptr64(inputs), hs, capi.ptr64(nfailed), capi.ptr32(first))
    return rc, list(hs) == [capi.raw(h) for h in handles] and (nfailed == SENTINEL64).all() and (first == SENTINEL32).all()


def test_refusals_write_nothing(tmp_path_factory):
    lib = capi.load_library()
    c = Circuit(3, 1, 3, 1031)
    d = tmp_path_factory.mktemp("r1cs_solve")
    paths = {name: str(d / name) for name in ("c.r1cs", "t.ptau", "c.zkey")}
    c.write_r1cs(paths["c.r1cs"])
    circom.WritePtau(paths["t.ptau"], 3, c.tau, c.alpha, c.beta)
    circom.SetupFromPtau(paths["c.r1cs"], paths["t.ptau"], paths["c.zkey"])
    _, product = circom.UploadZkey(paths["c.zkey"])
    assert raw_plan(product, [1]) == (-4, True) and b".r1cs" in lib.gs_last_error() and b"no C" in lib.gs_last_error()
    system = SU.independent(5)
    dev, m = upload(system), system[3]
    for bad in ([0], [m], [1, 1], [2, 1, 2]):
        assert raw_plan(dev, bad) == (-3, True), bad
    vec = capi.scalars_upload(np.zeros((m, 4), dtype=np.uint64))
    assert raw_plan(vec, [1]) == (-3, True) and raw_plan(0, [1]) == (-3, True)
    plan = dev.PlanSolve([1])
    count = ctypes.c_uint64(77)
    assert lib.gs_r1cs_solve_unsolved(capi.raw(dev), 0, None, ctypes.byref(count)) == -3 and count.value == 77
    fill = lambda k: np.full((k, 4), SENTINEL64, dtype=np.uint64)         # noqa: E731
    for k in (m - 1, m + 1):
        short = capi.scalars_upload(fill(k))
        assert raw_solve(plan.handle, 2, [0, short]) == (-4, True)
        assert (capi.scalars_download(short) == SENTINEL64).all()
    good = capi.scalars_upload(fill(m))
    assert raw_solve(plan.handle, 2, [good, dev]) == (-3, True) and raw_solve(dev, 1, [0]) == (-3, True) and raw_solve(vec, 1, [0]) == (-3, True)
    assert raw_solve(plan.handle, 2, [good, good]) == (-3, True) and raw_solve(plan.handle, 0, [])[0] == -3
    assert (capi.scalars_download(good) == SENTINEL64).all()


# ---- a gates circuit: check, prove, verify ---------------------------------------------------------------------------------------
_GATES = {}


def gates_case():
    if not _GATES:
        n = 1 << 10
        a, b, c, w, _ = synth.gates_r1cs(n, 77)
        dev = r1csqap.DeviceR1CS(a, b, c, n + 1)
        _GATES["case"] = (n, (a, b, c), capi.u64_to_ints(w), dev, dev.PlanSolve([1]))
    return _GATES["case"]


def test_a_solved_gates_witness_checks_and_proves_like_the_integer_witness():
    n, mats, w, dev, plan = gates_case()
    (dw,), report = plan.Solve([[w[1]]])
    assert report and capi.u64_to_ints(capi.scalars_download(dw)) == w and dev.CheckWitness(dw)
    rng = random.Random(1200)
    pk, vk = groth16.GenerateTrustedSetupSparse(n, n + 1, 1, *mats, tuple(rng.randrange(1 << 20, R) for _ in range(5)))
    r, s = rng.randrange(R), rng.randrange(R)
    want = groth16.prove_from_witness(pk, dev, capi.scalars_upload(capi.ints_to_u64(w)), r, s)
    got = groth16.prove_from_witness(pk, dev, dw, r, s)
    assert (got.PiA, got.PiB, got.PiC) == (want.PiA, want.PiB, want.PiC)
    proof = groth16.GenerateProofsFromInputs(None, pk, dev, plan, [w[1]], r, s)
    assert (proof.PiA, proof.PiB, proof.PiC) == (want.PiA, want.PiB, want.PiC) and groth16.VerifyProof(vk, proof, [w[1]])
    ppk, pvk = snark.GenerateTrustedSetupSparse(n, n + 1, 1, *mats, tuple(rng.randrange(1 << 20, R) for _ in range(8)))
    assert snark.VerifyProof(pvk, snark.GenerateProofsFromInputs(None, ppk, dev, plan, [w[1]]), [w[1]])


def test_generate_proofs_from_inputs_raises_on_a_broken_check_row_and_on_an_unsolved_system():
    # x * x = y (defines y), and the check row y * one = z over the INPUT z: only z = x^2 passes
    A, B, C = [[(1, 1)], [(3, 1)], [(0, 1)]], [[(1, 1)], [(0, 1)], [(0, 1)]], [[(3, 1)], [(2, 1)], [(0, 1)]]
    system = (A, B, C, 4, [1, 2])
    dev = upload(system)
    plan = dev.PlanSolve([1, 2])
    assert plan.stats["checks"] == 2
    rng = random.Random(1300)
    mats = (SU.csr(A), SU.csr(B), SU.csr(C))
    pk, vk = groth16.GenerateTrustedSetupSparse(3, 4, 2, *mats, tuple(rng.randrange(1 << 20, R) for _ in range(5)))
    ppk, _ = snark.GenerateTrustedSetupSparse(3, 4, 2, *mats, tuple(rng.randrange(1 << 20, R) for _ in range(8)))
    assert groth16.VerifyProof(vk, groth16.GenerateProofsFromInputs(None, pk, dev, plan, [5, 25]), [5, 25])
    for call in (lambda: groth16.GenerateProofsFromInputs(None, pk, dev, plan, [5, 26]), lambda: snark.GenerateProofsFromInputs(None, ppk, dev, plan, [5, 26])):
        with pytest.raises(r1csqap.WitnessError) as e:
            call()
        assert e.value.report.rows == [1]
    with pytest.raises(r1csqap.SolveError) as e:
        groth16.GenerateProofsFromInputs(None, pk, dev, dev.PlanSolve([2]), [25])
    assert e.value.report.unsolved == [1]          # z gives y through row 1 (form A); x sits in A and B of row 0


# ---- beside proofs in flight ---------------------------------------------------------------------------------------------------
def test_a_solve_between_three_begins_and_their_ends():
    n, mats, w, dev, plan = gates_case()
    rng = random.Random(1400)
    pk, _ = groth16.GenerateTrustedSetupSparse(n, n + 1, 1, *mats, tuple(rng.randrange(1 << 20, R) for _ in range(5)))
    xs = [rng.randrange(R) for _ in range(3)]
    A, B, C = (SU.from_csr(t) for t in mats)
    wits = [SU.solve(A, B, C, n + 1, [1], [x])[0] for x in xs]
    handles = [capi.scalars_upload(capi.ints_to_u64(x)) for x in wits]
    rs = [(rng.randrange(R), rng.randrange(R)) for _ in wits]
    blocking = [groth16.prove_from_witness(pk, dev, h, r, s) for h, (r, s) in zip(handles, rs)]
    tickets = [groth16.prove_witness_begin(pk, dev, h, r, s) for h, (r, s) in zip(handles, rs)]
    solved, report = plan.Solve([[w[1]], [xs[0]]])
    proofs = [groth16.prove_end(t) for t in tickets]
    assert report and [capi.u64_to_ints(capi.scalars_download(h)) for h in solved] == [w, wits[0]]
    assert [(p.PiA, p.PiB, p.PiC) for p in proofs] == [(p.PiA, p.PiB, p.PiC) for p in blocking]
