"""The level plan of gs_r1cs_solve restated the slow way, in Python integers: the expectation of the solver's tests.  Test infrastructure.

A system is three lists of rows, each row a list of (column, coefficient) pairs; duplicate columns are allowed."""
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
FORM_C, FORM_A, FORM_B = 0, 1, 2


def coeff(row, x):
    return sum(c for v, c in row if v == x) % R


def plan(A, B, C, m, inputs):
    """-> dict(entries=[(row, target, form, element)], levels=[offsets], unsolved=[...], checks=, stuck=): a rescan of every row per
    level, exactly as the definition reads.  element: 1 / c_x for form C, a_x / b_x for forms A / B."""
    n = len(A)
    known = {0} | set(inputs)
    used = set()
    entries, levels = [], [0]
    variables = [sorted({v for v, _ in A[j]} | {v for v, _ in B[j]} | {v for v, _ in C[j]}) for j in range(n)]
    while True:
        level = []
        taken = set()
        for j in range(n):
            if j in used:
                continue
            unknown = [v for v in variables[j] if v not in known]
            if len(unknown) != 1:
                continue
            x = unknown[0]
            k = (coeff(A[j], x), coeff(B[j], x), coeff(C[j], x))
            if sum(1 for v in k if v) != 1 or x in taken:
                continue
            taken.add(x)
            form = FORM_C if k[2] else FORM_A if k[0] else FORM_B
            level.append((form, j, x, pow(k[2], R - 2, R) if k[2] else k[0] or k[1]))
        if not level:
            break
        for form, j, x, e in sorted(level):
            entries.append((j, x, form, e))
            used.add(j)
            known.add(x)
        levels.append(len(entries))
    unsolved = [v for v in range(m) if v not in known]
    checks = sum(1 for j in range(n) if j not in used and all(v in known for v in variables[j]))
    return dict(entries=entries, levels=levels, unsolved=unsolved, checks=checks, stuck=n - len(used) - checks)


def launches(levels, narrow, run_max_rows):
    """level offsets -> [(lo, hi, is_run)]: consecutive levels narrower than `narrow` merge into runs cut every run_max_rows rows."""
    out, run = [], None
    def flush():
        nonlocal run
        if run:
            lo, hi = run
            while lo < hi:
                out.append((lo, min(hi, lo + run_max_rows), True))
                lo += run_max_rows
        run = None
    for lo, hi in zip(levels, levels[1:]):
        if hi - lo < narrow:
            run = (run[0] if run else lo, hi)
        else:
            flush()
            out.append((lo, hi, False))
    flush()
    return out


def dot(row, w):
    return sum(c * w[v] for v, c in row) % R


def solve(A, B, C, m, inputs, values, p=None):
    """The witness of one input assignment (values: integers, counted mod r) -> (w, nfailed, first_failed_row or None)."""
    p = p or plan(A, B, C, m, inputs)
    w = [0] * m
    w[0] = 1
    for v, x in zip(inputs, values):
        w[v] = x % R
    nfailed, first = 0, None
    for j, x, form, e in p["entries"]:
        sa, sb, sc = dot(A[j], w), dot(B[j], w), dot(C[j], w)
        if form == FORM_C:
            w[x] = (sa * sb - sc) * e % R
            continue
        den = e * (sb if form == FORM_A else sa) % R
        if den == 0:
            nfailed += 1
            first = j if first is None else first
            w[x] = 0
        else:
            w[x] = (sc - sa * sb) * pow(den, R - 2, R) % R
    return w, nfailed, first


def csr(rows):
    """rows -> (row_ptr, col, val) numpy triple as gs_r1cs_upload takes it (duplicates kept)."""
    import numpy as np
    rp, cols, vals = [0], [], []
    for row in rows:
        for v, c in row:
            cols.append(v)
            vals.append(c % R)
        rp.append(len(cols))
    val = np.zeros((len(vals), 4), dtype=np.uint64)
    for i, c in enumerate(vals):
        for k in range(4):
            val[i, k] = (c >> (64 * k)) & 0xFFFFFFFFFFFFFFFF
    return np.asarray(rp, dtype=np.uint32), np.asarray(cols, dtype=np.uint32), val


def from_csr(t):
    """(row_ptr, col, val) with val as [nnz, 4] uint64 limbs or integers -> rows"""
    rp, col, val = t
    out = []
    for j in range(len(rp) - 1):
        row = []
        for e in range(int(rp[j]), int(rp[j + 1])):
            v = val[e]
            c = int(v) if not hasattr(v, "__len__") else sum(int(v[k]) << (64 * k) for k in range(4))
            row.append((int(col[e]), c % R))
        out.append(row)
    return out


def from_dicts(rows):
    """rows as {column: coefficient} dicts (oracle.ref_py's and synth's form) -> rows"""
    return [[(int(v), int(c) % R) for v, c in sorted(row.items())] for row in rows]


# ---- small systems with known shapes -------------------------------------------------------------------------------------------
def independent(nrows):
    """one level of nrows independent rows: out_j = (x + j) * (x + 2 j + 1), variables: one, x, out_0 ..; input {1}"""
    A = [[(1, 1), (0, j)] for j in range(nrows)]
    B = [[(1, 1), (0, 2 * j + 1)] for j in range(nrows)]
    C = [[(2 + j, 1)] for j in range(nrows)]
    return A, B, C, 2 + nrows, [1]


def chain(nrows, k=3):
    """a chain of nrows dependent rows, sqchain's shape: s_(j+1) = s_j * s_j + k written as s_j * s_j = {one: -k, s_(j+1): 1}"""
    A = [[(1 + j, 1)] for j in range(nrows)]
    B = [[(1 + j, 1)] for j in range(nrows)]
    C = [[(0, -k % R), (2 + j, 1)] for j in range(nrows)]
    return A, B, C, 2 + nrows, [1]


def widths(ws):
    """a circuit whose level widths are ws: every row of level l multiplies the input by the first signal of level l - 1"""
    A, B, C = [], [], []
    m, prev = 2, 1
    for wd in ws:
        first = m
        for i in range(wd):
            A.append([(1, 1), (0, i + 1)])
            B.append([(prev, 1)])
            C.append([(m, 1)])
            m += 1
        prev = first
    return A, B, C, m, [1]
