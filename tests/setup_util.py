"""Shared by the tests of the setup from a transcript: a synthetic circuit with a satisfying witness and toxic values, whose key has
closed forms in the generators.  Test infrastructure (no test in here)."""
import random

from gosnark_amd import circom
import circom_util as CU

R = CU.R


class Circuit:
    """Wires: 0 = one, 1 .. nPublic public inputs, one private input, then one product per constraint: (A w)(B w) = w_new."""

    def __init__(self, k, npub, nc, seed, fan=2):
        rng = random.Random(seed)
        self.k, self.m, self.npub, self.nc = k, 1 << k, npub, nc
        assert max(1, (nc + npub).bit_length()) == k
        coef = lambda: rng.choice([1, 1, R - 1, 2, R - 3, rng.randrange(R)])      # noqa: E731
        w = [1] + [rng.randrange(R) for _ in range(npub + 1)]
        self.constraints = []
        dot = lambda lc: sum(v * w[s] for s, v in lc) % R                       # noqa: E731
        for _ in range(nc):
            la = [(rng.randrange(len(w)), coef()) for _ in range(fan)]
            lb = [(rng.randrange(len(w)), coef()) for _ in range(fan)]
            w.append(dot(la) * dot(lb) % R)
            self.constraints.append((la, lb, [(len(w) - 1, 1)]))
        self.w, self.nvars = w, len(w)
        self.tau, self.alpha, self.beta = (rng.randrange(2, R) for _ in range(3))
        L = CU.lagrange_at(k, self.tau)
        self.at, self.bt, self.ct = ([0] * self.nvars for _ in range(3))
        for j, lcs in enumerate(self.constraints):
            for lc, out in zip(lcs, (self.at, self.bt, self.ct)):
                for s, v in lc:
                    out[s] = (out[s] + v * L[j]) % R
        for s in range(npub + 1):                                              # the public rows: (signal s, 1) in A at row nc + s
            self.at[s] = (self.at[s] + L[nc + s]) % R
        self.kk = [(self.beta * a + self.alpha * b + c) % R for a, b, c in zip(self.at, self.bt, self.ct)]

    def write_r1cs(self, path):
        circom.WriteR1cs(path, self.nvars, 0, self.npub, 1, self.constraints)

    def h_scalars(self, with_last):
        """H_j = (1/2m) sum_{i < 2m (- 1)} y_j^(-i) tau^i, y_j = v^(2j+1): the geometric series (y_j^(2m) = 1), less the last term"""
        m2 = 2 * self.m
        v = CU.omega(self.k + 1)
        ys = [pow(v, 2 * j + 1, R) for j in range(self.m)]
        inv2m = pow(m2, -1, R)
        top = (pow(self.tau, m2, R) - 1) % R
        den = CU.batch_inverse([(self.tau - y) % R for y in ys])
        out = [top * y % R * d % R * inv2m % R for y, d in zip(ys, den)]       # (t^2m - 1) / (t / y - 1) / 2m
        if not with_last:
            last = pow(self.tau, m2 - 1, R)
            out = [(h - inv2m * last % R * y) % R for h, y in zip(out, ys)]     # y^(-(2m-1)) = y
        return out

    def h_scalars_by_definition(self, with_last):
        m2 = 2 * self.m
        vi = pow(CU.omega(self.k + 1), -1, R)
        n = m2 if with_last else m2 - 1
        return [sum(pow(vi, (2 * j + 1) * i % m2, R) * pow(self.tau, i, R) for i in range(n)) * pow(m2, -1, R) % R for j in range(self.m)]

    def expected_records(self):
        sh = pow(2, 512, R)
        out = []
        for j, (la, lb, _) in enumerate(self.constraints):
            out += [(0, j, s, v * sh % R) for s, v in la] + [(1, j, s, v * sh % R) for s, v in lb]
        return out + [(0, self.nc + s, s, sh) for s in range(self.npub + 1)]

    def proof_scalars(self, w, r, s, delta=1):
        dot = lambda ks: sum(x * y for x, y in zip(ks, w)) % R                  # noqa: E731
        dinv = pow(delta, -1, R)
        at, bt, ct = dot(self.at), dot(self.bt), dot(self.ct)
        a = (self.alpha + at + r * delta) % R
        b = (self.beta + bt + s * delta) % R
        cd = sum(self.kk[i] * w[i] for i in range(self.npub + 1, self.nvars)) * dinv % R
        return a, b, (cd + (at * bt - ct) * dinv + s * a + r * b - r * s % R * delta) % R

    def system_rows(self):
        """the three matrices as lists of (column, value) rows, A with the public rows appended"""
        a = [list(la) for la, _, _ in self.constraints] + [[(s, 1)] for s in range(self.npub + 1)]
        b = [list(lb) for _, lb, _ in self.constraints] + [[] for _ in range(self.npub + 1)]
        c = [list(lc) for _, _, lc in self.constraints] + [[] for _ in range(self.npub + 1)]
        return a, b, c
