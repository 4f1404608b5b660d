"""Sparse R1CS matrices in the shapes real front ends emit, and an exact reference for them (test infrastructure).

The circuits of gosnark_amd.synth and tests/test_gpu_prove.py have rows of one to three sorted, distinct, canonical entries.  Here a
matrix is a raw CSR triple (row_ptr uint32 [nrows + 1], col uint32 [nnz], val uint64 [nnz, 4]) built entry by entry: rows of a
prescribed length (a `ladder` around the 256-thread tile and the 512-entry hand-off of the device product), column indices that
are unsorted in some rows and repeated in others, and values anywhere in [0, 2^256).  The meaning of such a matrix is the one
`times` states: every raw entry contributes val * x[col] mod r, so repeated indices add and every value counts mod r."""
import random
from operator import mul

import numpy as np

from oracle import ref_py as O

R = O.R
# lengths around every seam of the device product: empty, the short rows of the synthetic circuits, one tile of 256 threads and
# its neighbours, the hand-off threshold 512 / 513, and whole tiles plus or minus one beyond it
LADDER = (0, 1, 2, 3, 255, 256, 257, 511, 512, 513, 514, 767, 768, 769, 1023, 1024, 1025)
LONG_ROW = 512          # rows of MORE entries than this are summed by a workgroup each
NONCANONICAL_OF = {"canonical": 0, "mixed": 32, "noncanonical": 56}      # of the 64 palette values


def standard_lengths(total, ncols, seed, repeats=2, nlong=130, top=None):
    """The length ladder (with `ncols` as its last rung) `repeats` times, then `nlong` seeded lengths in 513..top (default ncols), then
    seeded short lengths 0..3 up to `total` rows -- shuffled, so that long and short rows sit in one workgroup of the short-row
    kernel.  130 long rows are two full rounds of the 64 workgroups of the long-row kernel and a ragged third."""
    rng = random.Random(seed)
    top = ncols if top is None else top
    out = list(LADDER + (ncols,)) * repeats + [rng.randint(LONG_ROW + 1, top) for _ in range(nlong)]
    assert len(out) <= total, "the ladder alone has %d rows" % len(out)
    out += [rng.randint(0, 3) for _ in range(total - len(out))]
    rng.shuffle(out)
    return out


def palette(classes, seed):
    """64 values: the canonical ones 0, 1, 2, r - 1 and uniform elements of [0, r); for `mixed` / `noncanonical` 32 / 56 of them are
    replaced by r, r + 1, 2r - 1, 2^256 - 1 and uniform elements of [r, 2^256)."""
    rng = random.Random(seed)
    nnc = NONCANONICAL_OF[classes]
    non = [R, R + 1, 2 * R - 1, (1 << 256) - 1] + [rng.randrange(R, 1 << 256) for _ in range(60)]
    can = [0, 1, 2, R - 1] + [rng.randrange(R) for _ in range(60)]
    return non[:nnc] + can[:64 - nnc]


def ints_to_rows(vals):
    return np.frombuffer(b"".join(int(v).to_bytes(32, "little") for v in vals), dtype="<u8").reshape(len(vals), 4).astype(np.uint64)


def rows_to_ints(a):
    raw = np.ascontiguousarray(a, dtype="<u8").tobytes()
    return [int.from_bytes(raw[i:i + 32], "little") for i in range(0, len(raw), 32)]


def ladder_csr(nrows, ncols, lengths, seed, classes, avail=None, colmap=None):
    """Raw CSR triple with lengths[j] entries in row j.  Row j draws its columns from the first avail[j] columns (default: all);
    a row longer than that necessarily repeats indices.  About half of the rows keep a shuffled column order, about a third repeat
    a column index (up to four times over; the first row of five or more entries carries one index four times).  colmap, if given,
    renames the drawn column k to colmap[k].  Values come from palette(classes)."""
    assert len(lengths) == nrows
    rng = np.random.Generator(np.random.PCG64(seed))
    row_ptr = np.zeros(nrows + 1, dtype=np.uint32)
    row_ptr[1:] = np.cumsum(np.asarray(lengths, dtype=np.int64))
    nnz = int(row_ptr[nrows])
    col = np.zeros(nnz, dtype=np.uint32)
    deep = False
    for j in range(nrows):
        n = int(lengths[j])
        if n == 0:
            continue
        a = ncols if avail is None else int(avail[j])
        assert 1 <= a <= ncols
        if n <= a:
            c = rng.choice(a, size=n, replace=False)
            if rng.random() < 0.5:
                c.sort()
            if n >= 5 and not deep:
                c[[0, 2, 4]] = c[1]
                deep = True
            elif n >= 2 and rng.random() < 0.3:
                c[rng.choice(n, size=min(n - 1, int(rng.integers(1, 5))), replace=False)] = c[int(rng.integers(n))]
        else:
            c = rng.integers(0, a, size=n)
        col[int(row_ptr[j]):int(row_ptr[j + 1])] = c
    if colmap is not None:
        col = np.asarray(colmap, dtype=np.uint32)[col]
    val = ints_to_rows(palette(classes, seed))[rng.integers(0, 64, size=nnz)] if nnz else np.zeros((0, 4), dtype=np.uint64)
    return row_ptr, col, np.ascontiguousarray(val)


def transpose_ladder(nrows, ncols, lengths, seed, classes):
    """The same construction with the lengths applied to the COLUMNS: column i of the nrows x ncols matrix has lengths[i] entries
    (how many constraints variable i sits in).  Returned as a raw CSR triple whose rows hold their entries in a seeded order, so
    unsorted and repeated column indices survive the transposition."""
    cp, ri, cv = ladder_csr(ncols, nrows, lengths, seed, classes)
    nnz = int(cp[ncols])
    ci = np.repeat(np.arange(ncols, dtype=np.uint32), np.diff(cp.astype(np.int64)))
    perm = np.random.Generator(np.random.PCG64(seed + 1)).permutation(nnz)
    order = perm[np.argsort(ri[perm], kind="stable")]
    row_ptr = np.zeros(nrows + 1, dtype=np.uint32)
    row_ptr[1:] = np.cumsum(np.bincount(ri, minlength=nrows))
    return row_ptr, np.ascontiguousarray(ci[order]), np.ascontiguousarray(cv[order])


def times(csr, w):
    """The reference: (M w)_j = sum over the raw entries of row j of val * w[col] mod r, in Python integers."""
    row_ptr, col, val = csr
    v = rows_to_ints(val)
    wr = [int(x) % R for x in w]
    c, p = col.tolist(), row_ptr.tolist()
    return [sum(map(mul, v[lo:hi], map(wr.__getitem__, c[lo:hi]))) % R for lo, hi in zip(p, p[1:])]


def times_transposed(csr, ncols, x):
    """(M^T x)_i = sum over the raw entries (j, i) of val * x[j] mod r: what the trusted setup evaluates per variable."""
    row_ptr, col, val = csr
    v = rows_to_ints(val)
    c, p = col.tolist(), row_ptr.tolist()
    out = [0] * ncols
    for j, (lo, hi) in enumerate(zip(p, p[1:])):
        xj = int(x[j]) % R
        for k in range(lo, hi):
            out[c[k]] += v[k] * xj
    return [t % R for t in out]


def dense(csr, ncols):
    """nrows x ncols list of canonical ints: repeated entries summed, values reduced (the matrix the reference would be handed)."""
    row_ptr, col, val = csr
    v = rows_to_ints(val)
    out = [[0] * ncols for _ in range(len(row_ptr) - 1)]
    for j in range(len(row_ptr) - 1):
        for k in range(int(row_ptr[j]), int(row_ptr[j + 1])):
            out[j][int(col[k])] = (out[j][int(col[k])] + v[k]) % R
    return out


def satisfied_system(n, lengths_a, lengths_b, lengths_c, seed, extra=0, leaves=()):
    """A satisfied R1CS over m = n + 1 + extra variables [one, v_1 .. v_n, free ...].  Constraint j introduces v_j: its A and B rows
    are ladder rows over earlier variables, its C row is a ladder row over earlier variables plus {v_j: 1}, and
    w[v_j] = (A w)_j (B w)_j - (rest of the C row) w.  The variables v_j, j in `leaves`, appear in no other constraint: changing one
    of them breaks constraint j alone.  The `extra` free variables appear in no constraint.  -> ((A, B, C) raw CSR triples, w)."""
    m = n + 1 + extra
    allowed = np.array([i for i in range(n + 1) if i not in set(leaves)], dtype=np.uint32)
    assert allowed[0] == 0
    avail = np.searchsorted(allowed, np.arange(1, n + 1))          # variables before v_j that a row may use
    a = ladder_csr(n, m, lengths_a, seed, "mixed", avail, allowed)
    b = ladder_csr(n, m, lengths_b, seed + 1, "canonical", avail, allowed)
    rp, col, val = ladder_csr(n, m, lengths_c, seed + 2, "noncanonical", avail, allowed)
    rng = np.random.Generator(np.random.PCG64(seed + 3))
    at = rp[:-1].astype(np.int64) + rng.integers(0, np.diff(rp.astype(np.int64)) + 1)       # v_j anywhere in its row
    col = np.insert(col, at, np.arange(1, n + 1, dtype=np.uint32))
    val = np.insert(val, at, np.array([1, 0, 0, 0], dtype=np.uint64), axis=0)
    c = ((rp.astype(np.int64) + np.arange(n + 1)).astype(np.uint32), np.ascontiguousarray(col), np.ascontiguousarray(val))
    py = random.Random(seed + 4)
    w = [1] + [0] * n + [py.randrange(R) for _ in range(extra)]
    rows = [(m_[0].tolist(), m_[1].tolist(), [x % R for x in rows_to_ints(m_[2])]) for m_ in (a, b, c)]
    for j in range(1, n + 1):
        dot = []
        for p, cl, v in rows:
            lo, hi = p[j - 1], p[j]
            dot.append(sum(map(mul, v[lo:hi], map(w.__getitem__, cl[lo:hi]))) % R)
        w[j] = (dot[0] * dot[1] - dot[2]) % R            # w[j] is still 0 here, so dot[2] is the rest of the C row
    return (a, b, c), w


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


def horner(coeffs, x):
    acc = 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % R
    return acc
