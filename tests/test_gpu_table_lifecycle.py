"""-m gpu: every way out of a HALF-BUILT window table (csrc/tables.hip: a table is absent, building k of n, or resident).

Under policy `auto` a base array's table is built in instalments; tests/test_gpu_table_policy.py walks the schedule at 2^17.  Here the
smallest key at which a build is still half-way after a call, and from that state every transition the library has: a forced width
that supersedes the build, gs_build_tables that finishes or replaces it, gs_release_tables, the two other policies, an array whose
points are replaced under its build, and a plain base array through blocking and pipelined MSMs.  The result never changes.

The two knobs that make the build slow enough are read once per process, so every scenario runs in a child process (this file, run
as a script with the scenario's name): GS_TABLE_BG_SLAB_LOG2=10 gives G1 slabs of 1024 points (a G2 slab keeps its floor of 4096), and
GS_TABLE_BUDGET_PCT=2 grants a call 2^18 x 0.02 = 5243 point-builds where a G2 slab costs 4096 x 2.3 = 9421 and is bought once half of
it is covered: the 2^13 key needs about ten calls.  No scenario relies on that count: each one asserts that it SAW the half-way state
-- the handle holds table bytes while the last plan still had the table-free width -- before it acts on it.

Not reached from a half-built state: gs_groth16_pk_set_eval_domain.  It needs a key over a power-of-two domain, which the sqchain setup
key is not; it drops the array's table by the same BaseTable::invalidate as the calls of the eval and quot scenarios."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import gosnark_amd  # noqa: E402,F401
from gosnark_amd import capi, groth16, r1csqap, synth  # noqa: E402

pytestmark = pytest.mark.gpu

N = 1 << 13
KEY_SEED, RS_SEED, BASES_SEED = 0xA100, 0xA1, 0xA110
KNOBS = {"GS_TABLE_BG_SLAB_LOG2": "10", "GS_TABLE_BUDGET_PCT": "2"}
MAX_CALLS = 60                     # about ten are needed; a build that is not through by then never will be


def rs():
    return synth.field_elems(2, RS_SEED)


def msm_inputs():
    return synth.scalars_u64(N, BASES_SEED), synth.scalars_u64(N, BASES_SEED + 1)


def points(p):
    return [list(p.PiA), [list(x) for x in p.PiB], list(p.PiC)]


# ---- the child: one scenario, stops at its first failure ----------------------------------------------------------------------------
class Key:
    """a fresh 2^13 key; prove() is one blocking proof, checked against the closed form, and notes what the call left behind"""

    def __init__(self, want):
        self.inst = synth.sqchain_setup_instance(N, KEY_SEED)
        self.pk = self.inst.device_pk()
        self.want = want["proof"]
        self.witness = False
        self.dr = None
        assert self.held() == 0
        self.prove()
        assert self.held() == 0                               # the first use builds nothing
        self.free_width = self.width

    def held(self):
        return capi.handle_bytes(self.pk.handle)[1]

    def prove(self):
        r, s = rs()
        if self.witness:
            p = groth16.prove_from_witness(self.pk, self.dr, self.inst.w, r, s)
        else:
            p = groth16.prove_resident(self.pk, self.inst.w, self.inst.px, r, s)
        assert points(p) == self.want, "a proof differs from the closed form"
        self.width = capi.last_timing()["window_bits"]
        return self.width

    def to_half_way(self, above=0):
        """prove until the key holds more than `above` table bytes while the proof still ran table-free -> those bytes"""
        for _ in range(MAX_CALLS):
            self.prove()
            if self.held() > above:
                assert self.width == self.free_width, "the tables served before a half-way state was seen"
                return self.held()
        raise AssertionError("no build started")

    def to_tables(self):
        """prove until a proof runs on the tables -> the calls it took"""
        for i in range(MAX_CALLS):
            if self.prove() != self.free_width:
                return i + 1
        raise AssertionError("the tables never served")


def scenario_forced_width_supersedes(want):
    k = Key(want)
    half = k.to_half_way()
    capi.set_window_bits(17)                                  # tables of 15 rows; the table-free route clamps the width to 16
    assert k.prove() == 16
    forced = k.held()
    capi.set_window_bits(0)
    k.to_tables()
    rows = 254 // k.width + 1
    assert k.held() % rows == 0
    per_row = k.held() // rows                                # bytes of one row of every array this route sums
    # the build of the other width REPLACED the first one: one set of 15-row tables, not that on top of what was held before
    assert forced == 15 * per_row, (half, forced, k.held())
    print("RESULT", half, forced, k.held())


def scenario_build_tables_finishes(want):
    k = Key(want)
    half = k.to_half_way()
    capi.build_tables(k.pk.handle, 1)
    assert k.held() >= half
    assert k.prove() != k.free_width
    print("RESULT", half, k.held())


def scenario_build_tables_other_width(want):
    k = Key(want)
    half = k.to_half_way()
    capi.set_window_bits(17)
    capi.build_tables(k.pk.handle, 1)
    built = k.held()
    assert k.prove() == 17 and k.held() == built and built % 15 == 0
    capi.set_window_bits(0)
    print("RESULT", half, built)


def scenario_release(want):
    k = Key(want)
    half = k.to_half_way()
    capi.release_tables(k.pk.handle)
    assert k.held() == 0
    assert k.prove() == k.free_width and k.held() == 0        # the use count starts again: this call builds nothing
    assert k.to_half_way() > 0                                # a fresh build
    k.to_tables()
    print("RESULT", half, k.held())


def scenario_policy_always(want):
    k = Key(want)
    half = k.to_half_way()
    capi.set_table_policy("always")
    assert k.prove() != k.free_width and k.held() >= half
    print("RESULT", half, k.held())


def scenario_policy_never(want):
    k = Key(want)
    half = k.to_half_way()
    capi.set_table_policy("never")
    for _ in range(3):
        assert k.prove() == k.free_width and k.held() == half
    print("RESULT", half, k.held())


def scenario_eval_basis_replaced(want):
    """the witness route's own array (the evaluation basis) half-way, the arrays over w already on their tables"""
    k = Key(want)
    capi.build_tables(k.pk.handle, 1)
    px_tables = k.held()
    assert k.prove() != k.free_width
    k.witness, k.dr = True, r1csqap.DeviceR1CS(*k.inst.r1cs, k.inst.m)
    k.free_width = k.prove()                                  # the array's first use: table-free, nothing built
    assert k.held() == px_tables
    half = k.to_half_way(above=px_tables)
    eval_points = groth16.ExportPkArray(k.pk, "PowersTauDeltaEval")
    groth16.SetEvalBasis(k.pk, eval_points)                   # the array is replaced under its build
    assert k.held() == px_tables
    # the array keeps the uses it had: the VERY NEXT call begins the next build (after gs_release_tables it takes two: scenario_release)
    assert k.prove() == k.free_width and k.held() > px_tables
    again = k.held()
    groth16.DeriveEvalBasis(k.pk, N)                          # ... and once more, by the derivation
    assert k.held() == px_tables
    assert groth16.ExportPkArray(k.pk, "PowersTauDeltaEval") == eval_points
    assert k.prove() == k.free_width and k.held() > px_tables
    k.to_tables()
    assert k.held() > px_tables
    print("RESULT", px_tables, half, again, k.held())


def scenario_quot_basis_replaced(want):
    """the px route's own array (the quotient basis) half-way: detached, attached again, derived again"""
    k = Key(want)
    half = k.to_half_way()
    quot = groth16.ExportPkArray(k.pk, "PowersTauDeltaQuot")
    groth16.SetQuotBasis(k.pk, None)                          # detached under its build: the key divides px by Z again
    detached = k.held()
    assert detached < half
    k.prove()
    groth16.SetQuotBasis(k.pk, quot)
    attached = k.held()
    assert k.prove() == k.free_width and k.held() > attached  # its build begins again with the very next call
    rebuilding = k.held()
    groth16.DeriveQuotBasis(k.pk)
    derived = k.held()
    assert derived < rebuilding and groth16.ExportPkArray(k.pk, "PowersTauDeltaQuot") == quot
    assert k.prove() == k.free_width and k.held() > derived
    k.to_tables()
    print("RESULT", half, detached, attached, derived, k.held())


def scenario_base_array(want):
    ks, sc = msm_inputs()
    bases, h = capi.g1_fixed_base(ks), capi.scalars_upload(sc)
    expect = tuple(want["msm"])
    state = {"calls": 0}

    def msm():
        """blocking and pipelined calls in turn -> the width of the plan"""
        state["calls"] += 1
        got = capi.msm(bases, sc) if state["calls"] % 2 else capi.msm_end(capi.msm_begin(bases, h, N))
        assert got == expect, "an MSM differs from the closed form"
        return capi.last_timing()["window_bits"]

    def to_half_way():
        for _ in range(MAX_CALLS):
            width = msm()
            if capi.handle_bytes(bases)[1] > 0:
                assert width == free_width, "the table served before a half-way state was seen"
                return capi.handle_bytes(bases)[1]
        raise AssertionError("no build started")

    free_width = msm()
    assert capi.handle_bytes(bases)[1] == 0
    half = to_half_way()
    capi.release_tables(bases)
    assert capi.handle_bytes(bases)[1] == 0
    assert to_half_way() == half
    for _ in range(MAX_CALLS):
        if msm() != free_width:
            break
    assert msm() != free_width and msm() != free_width        # one call of each kind on the table
    print("RESULT", half, capi.handle_bytes(bases)[1], state["calls"])


SCENARIOS = ["forced_width_supersedes", "build_tables_finishes", "build_tables_other_width", "release", "policy_always", "policy_never",
             "eval_basis_replaced", "quot_basis_replaced", "base_array"]

if __name__ == "__main__":
    capi.init()
    capi.set_table_policy("auto")
    globals()["scenario_" + sys.argv[1]](json.loads(os.environ["GS_LIFECYCLE_WANT"]))
    sys.exit(0)


# ---- the parent: the closed forms once, a child per scenario ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def want():
    """what every proof of the key and every MSM of the base array must be, from the toxic values and the scalars alone"""
    import numpy as np
    import gpu_util as U
    from oracle import c_oracle as C
    from oracle import ref_py as O
    capi.init()
    inst = synth.sqchain_setup_instance(N, KEY_SEED)
    a, b, c = inst.expected_proof_scalars(*rs())
    ga, gb, gc = C.g1_affine(C.g1_mul_scalar(O.G1_GEN, a)), C.g2_affine(C.g2_mul_scalar(O.G2_GEN, b)), C.g1_affine(C.g1_mul_scalar(O.G1_GEN, c))
    ks, sc = msm_inputs()
    tot = int(np.sum(np.array(U.u64_rows_to_ints(ks), dtype=object) * np.array(U.u64_rows_to_ints(sc), dtype=object))) % O.R
    return json.dumps({"proof": [[ga[0], ga[1], 1], [list(gb[0]), list(gb[1]), [1, 0]], [gc[0], gc[1], 1]],
                       "msm": list(C.g1_affine(C.g1_mul_scalar(O.G1_GEN, tot)))})


@pytest.mark.parametrize("scenario", SCENARIOS)
def test_from_a_half_built_table(scenario, want):
    env = dict(os.environ, GS_LIFECYCLE_WANT=want, **KNOBS)
    out = subprocess.run([sys.executable, os.path.abspath(__file__), scenario], env=env, capture_output=True, text=True, timeout=10)
    print(out.stdout[-2000:])
    assert out.returncode == 0, out.stderr[-3000:]
    assert any(x.startswith("RESULT") for x in out.stdout.splitlines())
