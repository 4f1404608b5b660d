"""Field and curve primitives (csrc/fp29.h, fq2.h, ec.h) at the limits their bound types allow, on the HOST build of the raw-limb op
table tests/device/limit_ops.h: operands enter as raw limbs (saturated at kNearlyNormalMax - 1, values at B p - 1, k p +- 1, accumulators shifted
by the largest multiple of p their type admits) and every result is compared with Python integers -- exact identities, no tolerance.
tests/limits_util.py holds the inputs and the checks; tests/test_gpu_primitives.py runs the same plan on the device."""
import numpy as np
import pytest

import hostbuild
import limits_util as L


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build("fp_limits_host_test")


def _tables(exe, kind):
    tb = L.Tables(kind, lambda k, o, a: L.host_run(exe, [(k, o, a)])[0])
    tb.check()
    return tb


def test_op_table_has_a_check_for_every_op():
    names = [o.name for o in L.parse_ops()]
    assert len(names) == len(set(names)) and len(names) > 90
    for o in L.parse_ops():
        if o.name != "tables":
            assert o.bounds and (L.is_carry(o) or o.base in L.MONT or o.base in L.FQ2 or o.base in
                                 ("reduce2", "reduce2_normal", "canon", "is_zero", "equal", "inv", "fq2_inv")), o.name


@pytest.mark.parametrize("kind", [0, 1, 2], ids=["q", "r", "fq2"])
def test_field_ops_at_their_limits(exe, kind):
    """every op of the table for q, r and Fq2: the bias tables equal k p with the limb margins the subtractions rely on; carry ops equal
    their limb-wise formula limb for limb (no wrap-around) and their integer identity exactly; Montgomery results are congruent, below 2p
    and normal; reduce2 / canon / is_zero / equal decide exactly at every k p and k p +- 1"""
    tb = _tables(exe, 0 if kind == 2 else kind)
    plan = L.field_plan(kind, tb, 2024 + kind)
    if kind == 1:                                                # the value-bound type is checked against what the table really holds
        assert any(tb.tbias_k[k] != k for k in tb.tbias_k)
    outs = L.host_run(exe, [(kind, op.id, L.pack_field([s for s, _ in cases])) for op, cases in plan])
    for (op, cases), out in zip(plan, outs):
        assert len(out) == len(cases)
        L.check_field_op(op, kind, tb, cases, out)


@pytest.mark.parametrize("kind", [3, 4], ids=["g1", "g2"])
def test_point_ops_with_accumulators_at_the_top_of_their_types(exe, kind):
    """xyzz_madd (plain and negate), xyzz_add, xyzz_add_mem, xyzz_dbl and the tight G2 accumulator's xyzz_madd on raw XYZZ limbs with
    x < 9p, y < 5p (tight: 2p), zz, zzz < 2p: generic P + Q, P + P (doubling branch), P + (-P) (infinity), infinity on either side, each
    unshifted and shifted by the largest multiple of p per coordinate.  Output coordinates satisfy their types, ZZ^3 == ZZZ^2, and the
    affine point is the oracle's sum."""
    plan = L.point_plan(kind, 4040 + kind)
    assert set(plan) == ({0, 1, 2, 3, 4, 5, 6} if kind == 4 else {0, 1, 2, 3, 4})
    ops = sorted(plan)
    outs = L.host_run(exe, [(kind, op, np.array([r for r, _, _ in plan[op]], dtype=np.uint32)) for op in ops])
    for op, out in zip(ops, outs):
        assert len(out) == len(plan[op])
        L.check_point_op(kind, op, plan[op], out)
