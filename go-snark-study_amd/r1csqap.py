"""Mirror of the reference's r1csqap.PolynomialField (r1csqap/r1csqap.go:45-216) on the HIP kernels.
Polynomials are lists of Python ints (coefficients mod r, lowest degree first), like []*big.Int."""
import numpy as np

from . import capi
from .capi import R


def _arr(v):
    return capi.ints_to_u64([x % R for x in v]) if len(v) else np.zeros((0, 4), dtype=np.uint64)


class PolynomialField:
    """r1csqap.go:45-54.  `F` is kept for signature parity; the modulus is BN128's r."""

    def __init__(self, f=None):
        self.F = f

    def Mul(self, a, b):                     # r1csqap.go:57-67
        capi.init()
        out = np.zeros((len(a) + len(b) - 1, 4), dtype=np.uint64)
        capi.call("gs_poly_mul", capi.ptr64(_arr(a)), len(a), capi.ptr64(_arr(b)), len(b), capi.ptr64(out))
        return capi.u64_to_ints(out)

    def Div(self, a, b):                     # r1csqap.go:70-84 -> (quotient, remainder)
        capi.init()
        nq, nr = len(a) - len(b) + 1, len(b) - 1
        q = np.zeros((nq, 4), dtype=np.uint64)
        r = np.zeros((max(nr, 1), 4), dtype=np.uint64)
        capi.call("gs_poly_div", capi.ptr64(_arr(a)), len(a), capi.ptr64(_arr(b)), len(b), capi.ptr64(q), capi.ptr64(r))
        return capi.u64_to_ints(q), capi.u64_to_ints(r)[:nr]

    def _addsub(self, a, b, name):
        capi.init()
        n = max(len(a), len(b))
        out = np.zeros((n, 4), dtype=np.uint64)
        capi.call(name, capi.ptr64(_arr(a)), len(a), capi.ptr64(_arr(b)), len(b), capi.ptr64(out))
        return capi.u64_to_ints(out)

    def Add(self, a, b):                     # r1csqap.go:94-103
        return self._addsub(a, b, "gs_poly_add")

    def Sub(self, a, b):                     # r1csqap.go:106-115
        return self._addsub(a, b, "gs_poly_sub")

    def Eval(self, v, x):                    # r1csqap.go:118-126
        capi.init()
        out = np.zeros(4, dtype=np.uint64)
        capi.call("gs_poly_eval", capi.ptr64(_arr(v)), len(v), capi.ptr64(_arr([x])), capi.ptr64(out))
        return capi.u64_to_ints(out)[0]

    def LagrangeInterpolation(self, v):      # r1csqap.go:150-158 (nodes 1..len(v))
        capi.init()
        out = np.zeros((len(v), 4), dtype=np.uint64)
        capi.call("gs_lagrange_interpolation", capi.ptr64(_arr(v)), len(v), capi.ptr64(out))
        return capi.u64_to_ints(out)

    def DivisorPolynomial(self, px, z):      # r1csqap.go:213-216
        return self.Div(px, z)[0]

    def R1CSToQAP(self, a, b, c):            # r1csqap.go:161-188 (dense n x m matrices, small instances)
        """-> (alphas, betas, gammas, z): per variable the interpolant of its column over the nodes 1..n."""
        def cols(mat):
            n, m = len(mat), len(mat[0])
            return [self.LagrangeInterpolation([mat[j][i] for j in range(n)]) for i in range(m)]
        alphas, betas, gammas = cols(a), cols(b), cols(c)
        return alphas, betas, gammas, ZPoly(len(alphas) - 2)      # r1csqap.go:177-186: degree len(alphas) - 2

    def NewPolZeroAt(self, pointPos, totalPoints, height):   # r1csqap.go:129-147
        """The polynomial of degree totalPoints - 1 that is `height` at node pointPos and 0 at the other nodes of 1..totalPoints:
        the interpolant of height * e_pointPos.  Exact for every n (the reference's int64 factorials overflow from n = 22 on,
        r1csqap.go:130-136; equal results for n <= 21)."""
        v = [0] * totalPoints
        v[pointPos - 1] = height % R
        return self.LagrangeInterpolation(v)

    def _lincomb(self, r, polys):
        """sum_i r_i * polys[i] (coefficient-wise, shorter polynomials padded like the reference's Add, r1csqap.go:94-103) with ONE
        device product: the coefficients are packed as F(x) = sum_k sum_i polys[i][k] x^(2 m k + i) and multiplied by
        rev(r)(x) = sum_i r_i x^(m - 1 - i); the blocks of 2 m exponents do not overlap, so the coefficient of x^(2 m k + m - 1) is
        sum_i r_i polys[i][k].  The host only places integers; every field operation runs in gs_poly_mul."""
        m = len(r)
        n = max(len(p) for p in polys[:m])
        stride = 2 * m
        packed = [0] * (stride * n)
        for i in range(m):
            for k, v in enumerate(polys[i]):
                packed[k * stride + i] = v % R
        prod = self.Mul(packed, [r[m - 1 - i] % R for i in range(m)])
        return [prod[k * stride + m - 1] for k in range(n)]

    def CombinePolynomials(self, r, ap, bp, cp):   # r1csqap.go:191-210
        """ax = sum_i r_i ap_i, bx, cx likewise, px = ax * bx - cx, as the reference forms them (it iterates i < len(r) and its Add
        pads the shorter operand) -- five device calls whatever m and n are: one packed product per linear combination (_lincomb),
        one product and one subtraction for px.  (Round 3 recovered the column values with 3 m n blocking gs_poly_eval round trips and
        assumed equal lengths: ADVICE r3.)  No field arithmetic on the host."""
        m = len(r)
        if m == 0:
            raise ValueError("CombinePolynomials: empty witness (the reference's Mul panics on empty operands)")
        for name, polys in (("ap", ap), ("bp", bp), ("cp", cp)):
            if len(polys) < m:
                raise ValueError("CombinePolynomials: len(r) = %d but len(%s) = %d (the reference indexes %s[i] for every i < len(r))"
                                 % (m, name, len(polys), name))
            if any(len(p) == 0 for p in polys[:m]):
                raise ValueError("CombinePolynomials: %s holds an empty polynomial" % name)
        ax, bx, cx = self._lincomb(r, ap), self._lincomb(r, bp), self._lincomb(r, cp)
        px = self.Sub(self.Mul(ax, bx), cx)
        return ax, bx, cx, px


def Transpose(matrix):                       # r1csqap.go:11-21
    return [list(col) for col in zip(*matrix)]


def csr_from_rows(rows):
    """rows: list (one per constraint) of {variable index: coefficient} -> (row_ptr uint32, col uint32, val [nnz,4] uint64)."""
    rowptr = np.zeros(len(rows) + 1, dtype=np.uint32)
    cols, vals = [], []
    for j, row in enumerate(rows):
        for k in sorted(row):
            cols.append(k)
            vals.append(row[k] % R)
        rowptr[j + 1] = len(cols)
    col = np.asarray(cols, dtype=np.uint32) if cols else np.zeros(0, dtype=np.uint32)
    val = capi.ints_to_u64(vals) if vals else np.zeros((0, 4), dtype=np.uint64)
    return rowptr, col, val


def ComputePx(a_csr, b_csr, c_csr, w_u64, nvars):
    """Sparse R1CS (three CSR triples over n constraints x nvars variables) + witness ([nvars,4] uint64) ->
    (ax, bx, cx, px) as uint64 limb arrays: the scalable form of R1CSToQAP + CombinePolynomials (gs_r1cs_to_px)."""
    capi.init()
    n = a_csr[0].shape[0] - 1
    w = np.ascontiguousarray(w_u64, dtype=np.uint64).reshape(-1, 4)
    assert w.shape[0] == nvars
    out = [np.zeros((n, 4), dtype=np.uint64) for _ in range(3)] + [np.zeros((2 * n - 1, 4), dtype=np.uint64)]
    capi.call("gs_r1cs_to_px", n, nvars, *capi.csr_args((a_csr, b_csr, c_csr)), capi.ptr64(w), *map(capi.ptr64, out))
    return tuple(out)


def ZPoly(deg):
    """Z(x) = prod_{i=1}^{deg} (x - i)  (r1csqap.go:177-186 / groth16.go:122-131)."""
    return capi.u64_to_ints(capi.zpoly(deg))


class WitnessReport:
    """The outcome of DeviceR1CS.CheckWitness / circom.CheckWtns: truthy only when the witness satisfies every constraint.  `count`:
    how many of ALL n rows it violates (not the roots of a key's Z, which is what the prover's own count looks at); `rows`: the first
    `cap` of them, 0-based, ascending; `values`: their (A w, B w, C w) as integers in [0, r)."""

    def __init__(self, count, rows, values, witness=None):
        self.count, self.rows, self.values = int(count), [int(j) for j in rows], [tuple(int(x) for x in v) for v in values]
        self._witness = witness

    def __bool__(self):
        return self.count == 0

    def __repr__(self):
        if self:
            return "WitnessReport(every constraint satisfied)"
        shown = ", ".join(str(j) for j in self.rows[:8]) + (", ..." if self.count > min(len(self.rows), 8) else "")
        return "WitnessReport(%d violated: rows %s)" % (self.count, shown)

    def explain(self, i, r1cs, w=None):
        """Host only.  The three linear combinations of the i-th reported row (self.rows[i]) of a parsed circuit (circom.R1cs, or
        anything with CSR triples a, b, c) -> (A, B, C), each a list of (signal, coefficient, witness value) in the file's order,
        integers in [0, r).  w: the witness, when the report was not made from integers or a file."""
        w = self._witness if w is None else w
        if w is None:
            raise ValueError("explain: the report was made from a resident vector; pass the witness")
        j = self.rows[i]
        out = []
        for rp, col, val in (r1cs.a, r1cs.b, r1cs.c):
            if j + 1 >= len(rp):
                raise ValueError("explain: row %d, the circuit has %d constraints" % (j, len(rp) - 1))
            lo, hi = int(rp[j]), int(rp[j + 1])
            coef = capi.u64_to_ints(np.asarray(val).reshape(-1, 4)[lo:hi]) if hi > lo else []
            sig = [int(s) for s in col[lo:hi]]
            wv = [int(x) % R for x in (capi.u64_to_ints(np.asarray(w)[sig]) if isinstance(w, np.ndarray) else [w[s] for s in sig])]
            out.append([(s, c % R, x) for s, c, x in zip(sig, coef, wv)])
        return tuple(out)


class WitnessError(ValueError):
    """GenerateProofsChecked refused a witness before proving anything: .report is its WitnessReport."""

    def __init__(self, report):
        super().__init__("the witness violates %d constraint(s): %r" % (report.count, report))
        self.report = report


class DeviceR1CS:
    """A sparse R1CS resident on the device (gs_r1cs_upload): upload once per circuit, then ComputePxResident per proof."""

    def __init__(self, a_csr, b_csr, c_csr, nvars):
        self._upload("gs_r1cs_upload", (), (a_csr, b_csr, c_csr), nvars)

    def _upload(self, name, domain, csrs, nvars):
        """gs_r1cs_upload / gs_r1cs_upload_domain (whose arguments begin with the domain's log2)."""
        capi.init()
        self.n, self.nvars = csrs[0][0].shape[0] - 1, nvars
        cell = capi.HandleCell()
        capi.call(name, *domain, self.n, nvars, *capi.csr_args(csrs), cell.ref)
        self.handle = cell.result()

    def ComputePxResident(self, w_handle, px_handle=None):
        """resident w (capi.scalars_upload) -> resident px (a capi.DeviceHandle; pass the previous one to overwrite it)."""
        cell = capi.HandleCell(px_handle)
        capi.call("gs_r1cs_px", capi.raw(self), capi.raw(w_handle), cell.ref)
        return cell.result()

    def CheckWitness(self, w, cap=16):
        """Which constraints does the witness break (gs_r1cs_check: all n rows, no key, beside proofs in flight)?  -> WitnessReport.
        w: a resident vector (capi.scalars_upload), or integers / an [nvars, 4] uint64 array, uploaded for the call and freed.  A
        product system (circom.DeviceZkeyR1CS) holds no C: the library's GS_ERR_SHAPE error comes through unchanged."""
        resident = isinstance(w, (capi.DeviceHandle, int))
        dw = w if resident else capi.scalars_upload(capi.u64_rows(w))
        try:
            count, rows, values = capi.r1cs_check(self, dw, cap)
        finally:
            if not resident:
                dw.free()
        return WitnessReport(count, rows, [capi.u64_to_ints(v) for v in values], witness=None if resident else w)

    def PlanSolve(self, input_vars, narrow=0, run_max_rows=0):
        """gs_r1cs_solve_plan: how to solve this system's witnesses from the values of `input_vars` (variable 0, the constant one, is
        never an input) -> SolvePlan.  Once per circuit; narrow / run_max_rows = 0 take the library's defaults."""
        return SolvePlan(self, input_vars, narrow, run_max_rows)


class SolveReport:
    """The outcome of SolvePlan.Solve: truthy only when every variable was solved and no divisor was zero.  `unsolved`: the variables
    no row defines (they are 0 in every witness); `nfailed[b]`: the rows of witness b whose divisor was zero (their target is 0);
    `first_failed_row[b]`: the first of them in solve order, or None."""

    def __init__(self, unsolved, nfailed, first_failed_row):
        self.unsolved, self.nfailed, self.first_failed_row = list(unsolved), list(nfailed), list(first_failed_row)

    def __bool__(self):
        return not self.unsolved and not any(self.nfailed)

    def __repr__(self):
        if self:
            return "SolveReport(%d witnesses solved)" % len(self.nfailed)
        bad = [b for b, k in enumerate(self.nfailed) if k]
        return "SolveReport(%d variables unsolved; zero divisor in witnesses %s)" % (len(self.unsolved), bad[:8])


class SolveError(ValueError):
    """GenerateProofsFromInputs could not make the witnesses: variables stay unsolved or a divisor was zero.  .report is the SolveReport."""

    def __init__(self, report):
        super().__init__("the system does not determine the witness: %r" % (report,))
        self.report = report


class SolvePlan:
    """The level plan of a DeviceR1CS for one list of input variables (gs_r1cs_solve_plan).  .stats: solved, unsolved, checks, stuck,
    levels, launches, wide_launches, widest_level.  The plan keeps its system alive on the device."""

    def __init__(self, r1cs, input_vars, narrow=0, run_max_rows=0):
        self.r1cs, self.input_vars = r1cs, [int(v) for v in input_vars]
        self.handle, st = capi.r1cs_solve_plan(r1cs, self.input_vars, narrow, run_max_rows)
        self.stats = {name: int(getattr(st, name)) for name, _ in st._fields_}
        self._unsolved = None

    def unsolved(self):
        if self._unsolved is None:
            self._unsolved = capi.r1cs_solve_unsolved(self.handle)
        return list(self._unsolved)

    def Solve(self, inputs, into=None):
        """inputs: one list of len(input_vars) integers per witness (any value below 2^256, counted mod r).  into: None, or one resident
        vector of nvars elements (or None) per witness to overwrite.  -> (resident witness handles, SolveReport).  The plan's check
        rows are not examined here: DeviceR1CS.CheckWitness does that."""
        for row in inputs:
            if len(row) != len(self.input_vars):
                raise ValueError("Solve: %d values for %d input variables" % (len(row), len(self.input_vars)))
        handles, nfailed, first = capi.r1cs_solve(self.handle, inputs, into)
        return handles, SolveReport(self.unsolved(), nfailed, first)
