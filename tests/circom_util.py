"""Shared by the tests of the power-of-two domain QAP (snarkjs / circom keys): the fixture, the conventions of csrc/domain.h in
Python integers, and a synthetic generator -- a random sparse system over the domain 2^k with a satisfying witness, whose key is
built from toxic values (scalars in Python, points by gs_g1_fixed_base / gs_g2_fixed_base) and whose proofs therefore have closed
forms in the generators.  Test infrastructure (no test in here)."""
import json
import os
import random

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "golden", "circom_multiplier")
R = 21888242871839275222246405745257275088548364400416034343698204186575808495617


def omega(k):
    return pow(5, (R - 1) >> k, R)


def coset_gen(k):
    return pow(5, (R - 1) >> (k + 1), R)


def fixture_json(name):
    with open(os.path.join(FIXTURE, name + ".json")) as f:
        return json.load(f)


def batch_inverse(xs):
    pre, acc = [], 1
    for x in xs:
        pre.append(acc)
        acc = acc * x % R
    inv = pow(acc, -1, R)
    out = [0] * len(xs)
    for i in range(len(xs) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * xs[i] % R
    return out


def lagrange_at(k, tau, shift=1):
    """L_j(tau), j < m, over the nodes shift * omega^j:  (tau^m - shift^m) x_j / (m shift^m (tau - x_j))."""
    m, w = 1 << k, omega(k)
    xs, x = [], shift % R
    for _ in range(m):
        xs.append(x)
        x = x * w % R
    sm = pow(shift, m, R)
    num = (pow(tau, m, R) - sm) * pow(m * sm, -1, R) % R
    inv = batch_inverse([(tau - x) % R for x in xs])
    return [num * x % R * i % R for x, i in zip(xs, inv)]


def mat_vec(rows, w):
    return [sum(v * w[s] for s, v in row.items()) % R for row in rows]


def interpolate_naive(vals, k):
    """coefficients of the interpolant of vals (v_c at omega^c), O(m^2): small domains only"""
    m, wi = 1 << k, pow(omega(k), -1, R)
    minv = pow(m, -1, R)
    return [sum(v * pow(wi, i * c, R) for c, v in enumerate(vals)) * minv % R for i in range(m)]


def px_naive(rows_a, rows_b, rows_c, w, k):
    """px = a b - c (2m - 1 coefficients) for a small domain, schoolbook"""
    m = 1 << k
    pad = lambda v: v + [0] * (m - len(v))            # noqa: E731
    a, b, c = (interpolate_naive(pad(mat_vec(rows, w)), k) for rows in (rows_a, rows_b, rows_c))
    px = [0] * (2 * m - 1)
    for i, x in enumerate(a):
        for j, y in enumerate(b):
            px[i + j] = (px[i + j] + x * y) % R
    for i, x in enumerate(c):
        px[i] = (px[i] - x) % R
    return px


class Instance:
    """A synthetic domain instance: rows_a/b/c (n rows of {variable: coefficient}), a satisfying witness w, the toxic values, and the
    key scalars (at, bt, ct per variable, hExps).  Variable 0 is the constant 1, variable 1 the public input, variable 2 + c the
    product of row c."""

    def __init__(self, k, n, seed, tau=None, fan=2):
        rng = random.Random(seed)
        self.k, self.m, self.n = k, 1 << k, n
        self.nvars, self.npublic = n + 2, 1
        w = [1, rng.randrange(2, R)]
        self.rows_a, self.rows_b, self.rows_c = [], [], []
        for c in range(n):
            ra = {rng.randrange(len(w)): rng.randrange(1, R) for _ in range(fan)}
            rb = {rng.randrange(len(w)): rng.randrange(1, R) for _ in range(fan)}
            self.rows_a.append(ra)
            self.rows_b.append(rb)
            self.rows_c.append({2 + c: 1})
            w.append(sum(v * w[s] for s, v in ra.items()) * sum(v * w[s] for s, v in rb.items()) % R)
        self.w = w
        self.tau = rng.randrange(2, R) if tau is None else tau % R
        self.alpha, self.beta, self.gamma, self.delta = (rng.randrange(2, R) for _ in range(4))
        self.L = lagrange_at(k, self.tau)
        self.zt = (pow(self.tau, self.m, R) - 1) % R
        self.at, self.bt, self.ct = ([0] * self.nvars for _ in range(3))
        for rows, out in ((self.rows_a, self.at), (self.rows_b, self.bt), (self.rows_c, self.ct)):
            for c, row in enumerate(rows):
                for s, v in row.items():
                    out[s] = (out[s] + v * self.L[c]) % R
        dinv = pow(self.delta, -1, R)
        self.hexps = [pow(self.tau, i, R) * self.zt % R * dinv % R for i in range(self.m + 1)]
        self.cd = [0 if s <= self.npublic else (self.beta * self.at[s] + self.alpha * self.bt[s] + self.ct[s]) * dinv % R
                   for s in range(self.nvars)]

    def csr(self):
        from gosnark_amd import r1csqap
        return tuple(r1csqap.csr_from_rows(rows) for rows in (self.rows_a, self.rows_b, self.rows_c))

    def upload(self, n_hexps=None):
        """-> (groth16.DevicePk, circom.DeviceDomainR1CS)"""
        from gosnark_amd import capi, circom, groth16
        from oracle import ref_py as O
        g1 = lambda ks: capi.g1_fixed_base(capi.ints_to_u64(ks))            # noqa: E731
        pt = self.hexps if n_hexps is None else self.hexps[:n_hexps]
        mul1 = lambda kk: O.G1.MulScalar(O.G1_GEN, kk)                      # noqa: E731
        dev = groth16.device_pk_from_handles(g1(self.at), g1(self.bt), capi.g2_fixed_base(capi.ints_to_u64(self.bt)), g1(self.cd), g1(pt),
                                             mul1(self.alpha), mul1(self.beta), mul1(self.delta), O.G2.MulScalar(O.G2_GEN, self.beta),
                                             O.G2.MulScalar(O.G2_GEN, self.delta), capi.ints_to_u64([R - 1] + [0] * (self.m - 1) + [1]),
                                             self.nvars, self.npublic)
        a, b, c = self.csr()
        return dev, circom.DeviceDomainR1CS(self.k, a, b, c, self.nvars)

    def expected_scalars(self, w, r, s):
        """(a, b, c): PiA = a G1, PiB = b G2, PiC = c G1 for a witness that satisfies the system"""
        dot = lambda ks: sum(x * y for x, y in zip(ks, w)) % R              # noqa: E731
        at, bt, ct = dot(self.at), dot(self.bt), dot(self.ct)
        a = (self.alpha + at + r * self.delta) % R
        b = (self.beta + bt + s * self.delta) % R
        h = (at * bt - ct) * pow(self.delta, -1, R) % R                     # H(tau) Z(tau) / delta
        c = (dot(self.cd) + h + s * a + r * b - r * s % R * self.delta) % R
        return a, b, c

    def eval_basis_scalars(self):
        """E_j = e_j G with e_j = -L^coset_j(tau) (tau^m - 1) / (2 delta), L^coset the Lagrange basis over g omega^j"""
        lc = lagrange_at(self.k, self.tau, coset_gen(self.k))
        f = (-self.zt) * pow(2 * self.delta, -1, R) % R
        return [x * f % R for x in lc]


def assert_closed_form(proof, scalars):
    from oracle import c_oracle as C
    from oracle import ref_py as O
    a, b, c = scalars
    assert (proof.PiA[0], proof.PiA[1]) == C.g1_affine(C.g1_mul_scalar(O.G1_GEN, a))
    wb = C.g2_affine(C.g2_mul_scalar(O.G2_GEN, b))
    assert (proof.PiB[0], proof.PiB[1]) == (wb[0], wb[1])
    assert (proof.PiC[0], proof.PiC[1]) == C.g1_affine(C.g1_mul_scalar(O.G1_GEN, c))


def words(proof):
    """the three elements as one comparable tuple"""
    return (proof.PiA, proof.PiB, proof.PiC)


def u64(vals):
    from gosnark_amd import capi
    return capi.ints_to_u64([v % R for v in vals]) if len(vals) else np.zeros((0, 4), dtype=np.uint64)
