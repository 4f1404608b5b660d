"""The generator and reference of tests/r1cs_shapes.py against the dense restatement of the reference (oracle.ref_py R1CSToQAP +
CombinePolynomials) on tiny systems: what the device tests compare with must itself be what the reference would compute on the
matrix with repeated entries summed and every value reduced mod r.  No GPU."""
import random

import numpy as np
import pytest

import r1cs_shapes as S
from oracle import ref_py as O

R = O.R


def tiny_system(n, extra, seed):
    """every row length 0..n + 3 occurs somewhere: rows longer than the variables before them repeat indices by construction"""
    rng = random.Random(seed)
    lengths = [[rng.randint(0, n + 3) for _ in range(n)] for _ in range(3)]
    return S.satisfied_system(n, *lengths, seed, extra=extra, leaves=(1, n))


def test_ladder_csr_has_the_lengths_the_order_the_repeats_and_the_values_it_promises():
    lengths = S.standard_lengths(200, 700, 5, repeats=1, nlong=3)
    assert all(x in lengths for x in S.LADDER + (700,)) and len(lengths) == 200
    for classes, share in (("canonical", 0), ("mixed", 32), ("noncanonical", 56)):
        rp, col, val = S.ladder_csr(200, 700, lengths, 9, classes)
        assert rp.dtype == np.uint32 and col.dtype == np.uint32 and val.dtype == np.uint64 and val.shape == (int(rp[-1]), 4)
        assert np.diff(rp.astype(np.int64)).tolist() == lengths and int(col.max()) < 700
        rows = [col[int(rp[j]):int(rp[j + 1])].tolist() for j in range(200)]
        assert any(r != sorted(r) for r in rows) and any(r == sorted(r) and len(r) > 3 for r in rows)
        assert any(len(set(r)) < len(r) for r in rows) and any(len(set(r)) == len(r) > 3 for r in rows)
        assert max(max(r.count(k) for k in set(r)) for r in rows if r) >= 4
        pal = S.palette(classes, 9)
        assert sum(v >= R for v in pal) == share and set(S.rows_to_ints(val)) <= set(pal)
        if share:
            assert {R, R + 1, 2 * R - 1, (1 << 256) - 1} <= set(pal)
        assert {0, 1, 2, R - 1} <= set(pal)


def test_transpose_ladder_puts_the_lengths_on_the_columns_and_keeps_every_entry():
    lengths = S.standard_lengths(90, 40, 6, repeats=0, nlong=0)
    lengths = [min(x * 13, 40) for x in lengths]
    csr = S.transpose_ladder(40, 90, lengths, 12, "mixed")
    assert np.bincount(csr[1], minlength=90).tolist() == lengths and int(csr[0][-1]) == sum(lengths)
    cp, ri, cv = S.ladder_csr(90, 40, lengths, 12, "mixed")           # the construction it transposes
    x = [random.Random(3).randrange(1 << 256) for _ in range(40)]
    assert S.times_transposed(csr, 90, x) == S.times((cp, ri, cv), x)
    rows = [csr[1][int(csr[0][j]):int(csr[0][j + 1])].tolist() for j in range(40)]
    assert any(r != sorted(r) for r in rows) and any(len(set(r)) < len(r) for r in rows)


@pytest.mark.parametrize("n,extra", [(2, 0), (5, 1), (12, 0), (12, 1)])
def test_times_and_satisfied_system_agree_with_the_dense_reference(n, extra):
    (a, b, c), w = tiny_system(n, extra, 100 + n)
    m = n + 1 + extra
    assert len(w) == m and w[0] == 1
    da, db, dc = (S.dense(x, m) for x in (a, b, c))
    # the helper's own premise: repeated indices and values >= r do occur at this size
    assert any(len(set(r)) < len(r) for r in (a[1][int(a[0][j]):int(a[0][j + 1])].tolist() for j in range(n)))
    assert any(v >= R for v in S.rows_to_ints(a[2]) + S.rows_to_ints(c[2]))
    al, be, ga, z = O.PF.R1CSToQAP(da, db, dc)
    ax, bx, cx, px = O.PF.CombinePolynomials(w, al, be, ga)
    ta, tb, tc = S.times(a, w), S.times(b, w), S.times(c, w)
    for poly, vals in ((ax, ta), (bx, tb), (cx, tc)):
        assert [O.PF.Eval(poly, j) for j in range(1, n + 1)] == vals
        assert [x % R for x in O.PF.LagrangeInterpolation(vals)] == [x % R for x in poly]
        for x in (n + 1, 0, R - 5):                        # sum_j (M w)_j L_j(x) == mx(x): the identity the cap case leans on
            assert sum(v * l for v, l in zip(vals, S.lagrange_at(n, x))) % R == O.PF.Eval(poly, x) == S.horner(poly, x)
    # satisfied: at every constraint, and so px is a multiple of the reference's Z (roots 1 .. m - 2)
    assert [x * y % R for x, y in zip(ta, tb)] == tc
    _, rem = O.PF.Div(px, z)
    assert not any(x % R for x in rem)
    # the transposed product is the reference's per-variable evaluation alphas[i](tau)
    tau = random.Random(n).randrange(n + 1, R)
    lag = S.lagrange_at(n, tau)
    for mat, polys in ((a, al), (b, be), (c, ga)):
        assert S.times_transposed(mat, m, lag) == [O.PF.Eval(p, tau) for p in polys]
    # a leaf variable breaks its own constraint and no other; a non-canonical witness entry is the same witness
    for leaf in (1, n):
        bad = list(w)
        bad[leaf] = (bad[leaf] + 1) % R
        fa, fb, fc = S.times(a, bad), S.times(b, bad), S.times(c, bad)
        assert [j + 1 for j in range(n) if fa[j] * fb[j] % R != fc[j]] == [leaf]
    lifted = [x + R * (i % 3) for i, x in enumerate(w)]
    assert S.times(a, lifted) == ta and S.times(c, lifted) == tc
    assert all(v == 0 for mat in (a, b, c) for v in S.times_transposed(mat, m, lag)[n + 1:])        # the free variables
