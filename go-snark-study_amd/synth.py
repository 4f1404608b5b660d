"""Deterministic synthetic Groth16 instances for bench.py and the large-size parity tests
(SURVEY.md 8d).  Everything heavy is produced on the device through the C ABI (fixed-base batch
multiplication = the hot loop of groth16.GenerateTrustedSetup, groth16.go:139-175)."""
import numpy as np

from . import capi, groth16

R = groth16.R
_R_LIMBS = [(R >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]


def scalars_u64(n, seed):
    """n uniform elements of [0, r) as an [n, 4] uint64 array (vectorised rejection sampling)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    out = np.zeros((n, 4), dtype=np.uint64)
    todo = np.arange(n)
    while todo.size:
        cand = rng.integers(0, 2**64, size=(todo.size, 4), dtype=np.uint64)
        cand[:, 3] &= np.uint64(0x3FFFFFFFFFFFFFFF)
        lt = np.zeros(todo.size, dtype=bool)
        eq = np.ones(todo.size, dtype=bool)
        for i in (3, 2, 1, 0):
            lt |= eq & (cand[:, i] < np.uint64(_R_LIMBS[i]))
            eq &= cand[:, i] == np.uint64(_R_LIMBS[i])
        out[todo[lt]] = cand[lt]
        todo = todo[~lt]
    return out


def field_elems(n, seed, modulus=R):
    return [int(x) % modulus for x in capi.u64_to_ints(scalars_u64(n, seed))]


def _jac_g1(row):
    v = capi.u64_to_ints(row)
    return (v[0], v[1], v[2])


def _jac_g2(row):
    v = capi.u64_to_ints(row)
    return ((v[0], v[1]), (v[2], v[3]), (v[4], v[5]))


class RandomInstance:
    """A Groth16 instance of the reference's shape (m = n + 1, NPublic = 1, len(Z) = len(hx) = n =
    len(PowersTauDelta), len(px) = 2n - 1) whose key points are k_i * G for seeded
    uniform k_i and whose w / px are seeded uniform field elements.  The arithmetic the prover performs
    is that of a real instance of this size (px / Z leaves a remainder, which groth16.go:266 discards)."""

    def __init__(self, n, seed):
        self.n, self.m, self.seed = n, n + 1, seed
        m = self.m
        self.g1 = {
            "at": capi.g1_fixed_base(scalars_u64(m, seed + 1)),
            "bacgamma": capi.g1_fixed_base(scalars_u64(m, seed + 2)),
            "bacdelta": capi.g1_fixed_base(scalars_u64(m, seed + 3)),
            "ptd": capi.g1_fixed_base(scalars_u64(n, seed + 4)),
        }
        self.g2_bacgamma = capi.g2_fixed_base(scalars_u64(m, seed + 5))
        singles1 = capi.g1_download(capi.g1_fixed_base(scalars_u64(3, seed + 6)))
        singles2 = capi.g2_download(capi.g2_fixed_base(scalars_u64(2, seed + 7)))
        self.alpha, self.beta, self.delta = (_jac_g1(singles1[i]) for i in range(3))
        self.beta2, self.delta2 = (_jac_g2(singles2[i]) for i in range(2))
        self.w_host = scalars_u64(m, seed + 8)
        self.w_host[0] = (1, 0, 0, 0)
        self.px_host = scalars_u64(2 * n - 1, seed + 9)
        self.z_host = self._z()
        self.w = capi.scalars_upload(self.w_host)
        self.px = capi.scalars_upload(self.px_host)
        self._pk = None

    def _z(self):
        """Z(x) = prod_{i=1}^{m-2} (x - i) (groth16.go:122-131): n coefficients."""
        return capi.zpoly(self.m - 2)

    def device_pk(self):
        if self._pk is None:
            self._pk = groth16.device_pk_from_handles(
                self.g1["at"], self.g1["bacgamma"], self.g2_bacgamma, self.g1["bacdelta"], self.g1["ptd"],
                self.alpha, self.beta, self.delta, self.beta2, self.delta2, self.z_host, self.m, 1)
        return self._pk

    def describe(self):
        return ("key points k_i*G (seeded uniform k_i), w and px seeded uniform in [0,r), "
                "Z = prod_{i=1..m-2}(x-i); seed 0x%X" % self.seed)


def random_instance(n, seed):
    return RandomInstance(n, seed)


class QuotientInstance(RandomInstance):
    """RandomInstance's key and witness with a px whose quotient is KNOWN: px = hx * Z + rem for seeded uniform hx (n coefficients)
    and rem (n - 2 coefficients, degree below Z's), built here with the library's own gs_poly_mul / gs_poly_add.  The golden generator
    (oracle/gen_golden_large.py prove20) builds the same px by an unrelated exact product (oracle/crt_ntt.py) and records its SHA-256,
    so a test can pin the device product at 2^20 and then the whole proof, whose fifth sum is sum_i hx_i PTD_i for that known hx."""

    def __init__(self, n, seed):
        import hashlib
        super().__init__(n, seed)
        self.hx_host = scalars_u64(n, seed + 11)
        self.px_host = px = _quotient_px(self.hx_host, self.z_host, scalars_u64(n - 2, seed + 12))
        self.px_sha256 = hashlib.sha256(np.ascontiguousarray(px, dtype="<u8").tobytes()).hexdigest()
        self.px.free()
        self.px = capi.scalars_upload(px)


def _quotient_px(hx, z, rem):
    """hx * z + rem as [2 n - 1, 4] uint64 for n = len(hx), len(z) = n: the library's own gs_poly_mul / gs_poly_add."""
    n = hx.shape[0]
    prod, px = np.zeros((2 * n - 1, 4), dtype=np.uint64), np.zeros((2 * n - 1, 4), dtype=np.uint64)
    capi.call("gs_poly_mul", capi.ptr64(hx), n, capi.ptr64(z), z.shape[0], capi.ptr64(prod))
    capi.call("gs_poly_add", capi.ptr64(prod), 2 * n - 1, capi.ptr64(rem), rem.shape[0], capi.ptr64(px))
    return px


def quotient_instance(n, seed):
    return QuotientInstance(n, seed)


def sqchain_witness(n, x, extra_vars=0):
    """The satisfying assignment of sqchain_r1cs(n, x) alone ([m, 4] uint64): another proof of the same circuit."""
    wit = [1, x % R]
    for k in range(1, n):
        wit.append((wit[k] * wit[k] + k) % R)
    for e in range(extra_vars):
        wit.append((x * 31337 + e + 5) % R)
    return capi.ints_to_u64(wit)


def sqchain_r1cs(n, x, extra_vars=0):
    """SURVEY 8d's synthetic circuit: variables [one, s_1 = x (public), s_2 .. s_n] (m = n + 1, NPublic = 1);
    constraint k = 1..n-1:  s_k * s_k = s_{k+1} - k * one;  constraint n:  one * one = one.
    Returns (a_csr, b_csr, c_csr, w [m,4] uint64); nnz: A = n, B = n, C = 2n - 1 (k = 0 entries are dropped).
    extra_vars = 1 appends an unconstrained variable: the m = n + 2 shape the reference also accepts (snark_test.go:280-290)."""
    m = n + 1 + extra_vars
    wit = [1, x % R]
    for k in range(1, n):
        wit.append((wit[k] * wit[k] + k) % R)
    for e in range(extra_vars):
        wit.append((x * 31337 + e + 5) % R)
    idx = np.arange(n, dtype=np.uint32)
    one = np.zeros((n, 4), dtype=np.uint64)
    one[:, 0] = 1
    rowptr = np.arange(n + 1, dtype=np.uint32)
    a_col = idx + 1
    a_col[n - 1] = 0                                  # last constraint: one * one = one
    a = (rowptr, a_col.copy(), one)
    b = (rowptr, a_col.copy(), one.copy())
    # C rows: k = 1..n-1 -> {s_{k+1}: 1, one: -k}; row n -> {one: 1}
    c_rowptr = np.zeros(n + 1, dtype=np.uint32)
    c_rowptr[1:n] = 2 * np.arange(1, n, dtype=np.uint32)
    c_rowptr[n] = 2 * (n - 1) + 1
    c_col = np.zeros(2 * (n - 1) + 1, dtype=np.uint32)
    c_val = np.zeros((2 * (n - 1) + 1, 4), dtype=np.uint64)
    ks = np.arange(1, n, dtype=np.uint64)
    c_col[0:2 * (n - 1):2] = 0                        # the `one` entry first (columns sorted)
    c_col[1:2 * (n - 1):2] = np.arange(2, n + 1, dtype=np.uint32)
    negk = capi.ints_to_u64([(R - int(k)) % R for k in ks]) if n > 1 else np.zeros((0, 4), dtype=np.uint64)
    c_val[0:2 * (n - 1):2] = negk
    c_val[1:2 * (n - 1):2, 0] = 1
    c_col[2 * (n - 1)] = 0
    c_val[2 * (n - 1), 0] = 1
    c = (c_rowptr, c_col, c_val)
    return a, b, c, capi.ints_to_u64(wit)


class SqchainInstance(RandomInstance):
    """RandomInstance whose w / px come from a SATISFIED R1CS (the sqchain circuit): px is produced on the device from
    the sparse system (gs_r1cs_to_px) and is exactly divisible by Z, as in a real proof.  The key points remain
    k_i * G for seeded k_i (a structured trusted setup is SURVEY 8f item 1)."""

    def __init__(self, n, seed):
        from . import r1csqap
        super().__init__(n, seed)
        x = field_elems(1, seed + 10)[0]
        a, b, c, w = sqchain_r1cs(n, x)
        self.r1cs = (a, b, c)
        self.w_host = w
        self.ax_host, self.bx_host, self.cx_host, self.px_host = r1csqap.ComputePx(a, b, c, w, self.m)
        self.w = capi.scalars_upload(self.w_host)
        self.px = capi.scalars_upload(self.px_host)

    def describe(self):
        return ("sqchain(n) R1CS (s_k^2 = s_{k+1} - k), satisfying witness, px = A(x)B(x) - C(x) from the sparse system on the "
                "device (exactly divisible by Z); key points k_i*G for seeded uniform k_i; seed 0x%X" % self.seed)


def sqchain_instance(n, seed):
    return SqchainInstance(n, seed)


class SqchainSetupInstance:
    """A COMPLETE synthetic Groth16 instance: the sqchain(n) R1CS, a satisfying witness, a structured
    trusted setup built on the device from seeded toxic values (gs_groth16_setup = groth16.go:94-222), and px from the
    sparse system.  Because the toxic values are known, the proof the prover must emit is known in closed form
    (expected_proof_scalars) -- an end-to-end check at sizes no reference implementation can replay."""

    def __init__(self, n, seed, extra_vars=0):
        from . import r1csqap
        self.n, self.m, self.seed = n, n + 1 + extra_vars, seed
        self.toxic = field_elems(5, seed + 20)
        x = field_elems(1, seed + 10)[0]
        a, b, c, w = sqchain_r1cs(n, x, extra_vars)
        self.r1cs = (a, b, c)
        self.w_host = w
        self._pk, self.vk = groth16.GenerateTrustedSetupSparse(n, self.m, 1, a, b, c, self.toxic)
        self.ax_host, self.bx_host, self.cx_host, self.px_host = r1csqap.ComputePx(a, b, c, w, self.m)
        self.w = capi.scalars_upload(self.w_host)
        self.px = capi.scalars_upload(self.px_host)

    def device_pk(self):
        return self._pk

    def describe(self):
        return ("sqchain(n) R1CS (s_k^2 = s_{k+1} - k), satisfying witness, structured trusted setup on the device from seeded "
                "toxic values (gs_groth16_setup), px = A(x)B(x) - C(x) from the sparse system; seed 0x%X" % self.seed)

    def _closed_form_tables(self):
        """What the closed form needs of the circuit and the setup alone (cached: bench.py checks several witnesses of one instance):
        L_j(tau) over the nodes 1..n, the CSR matrices as Python ints, and a_i(tau), b_i(tau), c_i(tau) for the public i <= 1."""
        if getattr(self, "_cf", None) is not None:
            return self._cf
        n = self.n
        T = self.toxic[0]
        # L_j(tau) = M(tau) / ((tau - j) M'(j)),  M'(j) = (-1)^(n-j) (j-1)! (n-j)!
        fact = [1] * (n + 1)
        for k in range(1, n + 1):
            fact[k] = fact[k - 1] * k % R
        den = []
        mt = 1
        for j in range(1, n + 1):
            mt = mt * (T - j) % R
            d = (T - j) * fact[j - 1] % R * fact[n - j] % R
            den.append(d if (n - j) % 2 == 0 else R - d)
        pre = [1] * (n + 1)
        for i, d in enumerate(den):
            pre[i + 1] = pre[i] * d % R
        inv = pow(pre[n], R - 2, R)
        lag = [0] * n
        for i in range(n - 1, -1, -1):
            lag[i] = mt * (inv * pre[i] % R) % R
            inv = inv * den[i] % R
        mats, lows = [], []
        for rp, cl, vl in self.r1cs:
            rp, cl, vals = [int(x) for x in rp], [int(x) for x in cl], capi.u64_to_ints(vl)
            low = [0, 0]
            for j in range(n):
                for e in range(rp[j], rp[j + 1]):
                    if cl[e] <= 1:
                        low[cl[e]] = (low[cl[e]] + vals[e] * lag[j]) % R       # a_i(tau) for i <= NPublic
            mats.append((rp, cl, vals))
            lows.append(low)
        self._cf = (lag, mats, lows)
        return self._cf

    def expected_proof_scalars(self, r, s, w_host=None):
        """Discrete logs (to the base G1 / G2 generators) of the proof elements groth16.go:243-275 must produce:
           a = A(tau) + Kalpha + r Kdelta,  b = B(tau) + Kbeta + s Kdelta,
           c = [ sum_{i>l} w_i (Kbeta a_i + Kalpha b_i + c_i)(tau) + A(tau) B(tau) - C(tau) ] / Kdelta + s a + r b - r s Kdelta
        with A(tau) = sum_j (A w)_j L_j(tau) over the nodes 1..n (H Z = A B - C because the witness satisfies the R1CS).
        w_host: another satisfying witness of the same circuit ([m, 4] uint64; default: the instance's own)."""
        n = self.n
        T, Ka, Kb, Kg, Kd = self.toxic
        w = capi.u64_to_ints(self.w_host if w_host is None else w_host)
        lag, mats, lows = self._closed_form_tables()
        sums = []
        for rp, cl, vals in mats:
            tot = 0
            for j in range(n):
                acc = 0
                for e in range(rp[j], rp[j + 1]):
                    acc += vals[e] * w[cl[e]]
                tot += acc % R * lag[j]
            sums.append(tot % R)
        At, Bt, Ct = sums
        a = (At + Ka + r * Kd) % R
        b = (Bt + Kb + s * Kd) % R
        priv = (Kb * At + Ka * Bt + Ct) % R
        for i in (0, 1):                                              # subtract the public part (i <= NPublic = 1)
            priv = (priv - w[i] * (Kb * lows[0][i] + Ka * lows[1][i] + lows[2][i])) % R
        c = ((priv + At * Bt - Ct) * pow(Kd, R - 2, R) + s * a + r * b - r * s % R * Kd) % R
        return a, b, c


def sqchain_setup_instance(n, seed, extra_vars=0):
    return SqchainSetupInstance(n, seed, extra_vars)


def realistic_r1cs(n, seed):
    """A satisfiable R1CS whose WITNESS has the shape the reference's CalculateWitness produces (circuitcompiler/circuit.go:158-182:
    flags, selectors and small intermediate values dominate; few wires are full-width field elements) -- VERDICT r3 next #6.
    Variables [one, x (public), v_2 .. v_n] (m = n + 1, NPublic = 1); constraint j = 1..n-1 introduces variable j + 1 as one of
      bit   (~50 %)  v * v = v,          v in {0, 1}
      small (~40 %)  v * one = v,        v < 2^32            (stand-in for a range-checked value)
      chain (~10 %)  p * p = v - j one,  p the previous chain variable (x at first): full-width values, as in sqchain_r1cs
    and constraint n is one * one = one.  Returns (a_csr, b_csr, c_csr, w [m,4] uint64, counts)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = field_elems(1, seed + 10)[0]
    kind = rng.random(n - 1)                                   # constraint j = 1..n-1 <-> kind[j - 1]
    is_bit, is_chain = kind < 0.5, kind >= 0.9
    is_small = ~is_bit & ~is_chain
    j = np.arange(1, n, dtype=np.int64)
    var = j + 1
    # previous chain variable of every constraint (1 = x before the first chain constraint)
    last = np.where(is_chain, var, 0)
    prev = np.concatenate(([1], np.maximum.accumulate(np.maximum(last, 1))[:-1]))
    a_col = np.where(is_chain, prev, var)
    b_col = np.where(is_chain, prev, np.where(is_small, 0, var))
    one = np.zeros((n, 4), dtype=np.uint64)
    one[:, 0] = 1
    rowptr = np.arange(n + 1, dtype=np.uint32)
    a = (rowptr, np.concatenate((a_col, [0])).astype(np.uint32), one)
    b = (rowptr, np.concatenate((b_col, [0])).astype(np.uint32), one.copy())
    # C: one entry {v: 1}, chain rows two entries {one: -j, v: 1} (columns sorted); last row {one: 1}
    per_row = np.concatenate((np.where(is_chain, 2, 1), [1])).astype(np.uint32)
    c_rowptr = np.zeros(n + 1, dtype=np.uint32)
    c_rowptr[1:] = np.cumsum(per_row)
    nnz = int(c_rowptr[n])
    c_col = np.zeros(nnz, dtype=np.uint32)
    c_val = np.zeros((nnz, 4), dtype=np.uint64)
    first = c_rowptr[:-1][:n - 1]
    c_col[first[~is_chain]] = var[~is_chain]
    c_val[first[~is_chain], 0] = 1
    ch = np.nonzero(is_chain)[0]
    c_col[first[ch]] = 0
    c_val[first[ch]] = capi.ints_to_u64([(R - int(k)) % R for k in j[ch]]) if ch.size else np.zeros((0, 4), dtype=np.uint64)
    c_col[first[ch] + 1] = var[ch]
    c_val[first[ch] + 1, 0] = 1
    c_col[nnz - 1] = 0
    c_val[nnz - 1, 0] = 1
    c = (c_rowptr, c_col, c_val)
    # witness
    w = np.zeros((n + 1, 4), dtype=np.uint64)
    w[0, 0] = 1
    w[1] = capi.ints_to_u64([x])[0]
    w[var[is_bit], 0] = rng.integers(0, 2, size=int(is_bit.sum()), dtype=np.uint64)
    w[var[is_small], 0] = rng.integers(0, 2**32, size=int(is_small.sum()), dtype=np.uint64)
    cur, vals = x, []
    for k in j[ch]:
        cur = (cur * cur + int(k)) % R
        vals.append(cur)
    if vals:
        w[var[ch]] = capi.ints_to_u64(vals)
    counts = {"bit": int(is_bit.sum()), "small": int(is_small.sum()), "full_width": int(is_chain.sum()) + 1}
    counts["zeros"] = int(((w == 0).all(axis=1)).sum())
    counts["ones"] = int(((w[:, 0] == 1) & (w[:, 1:] == 0).all(axis=1)).sum())
    return a, b, c, w, counts


class RealisticSetupInstance(SqchainSetupInstance):
    """SqchainSetupInstance's machinery (device trusted setup from seeded toxic values, px from the sparse system, the closed-form
    proof) on realistic_r1cs: the heavy-bucket / zero-digit paths of the MSM plan under load instead of uniform 254-bit scalars."""

    def __init__(self, n, seed):
        from . import r1csqap
        self.n, self.m, self.seed = n, n + 1, seed
        self.toxic = field_elems(5, seed + 20)
        a, b, c, w, self.counts = realistic_r1cs(n, seed)
        self.r1cs = (a, b, c)
        self.w_host = w
        self._pk, self.vk = groth16.GenerateTrustedSetupSparse(n, self.m, 1, a, b, c, self.toxic)
        self.ax_host, self.bx_host, self.cx_host, self.px_host = r1csqap.ComputePx(a, b, c, w, self.m)
        self.w = capi.scalars_upload(self.w_host)
        self.px = capi.scalars_upload(self.px_host)

    def describe(self):
        return ("realistic-witness R1CS (%(bit)d bit constraints v^2 = v, %(small)d small values < 2^32, %(full_width)d full-width chain values: "
                "%(zeros)d zeros and %(ones)d ones among the witness entries), structured trusted setup on the device, px from the sparse system"
                % self.counts) + "; seed 0x%X" % self.seed


def realistic_setup_instance(n, seed):
    return RealisticSetupInstance(n, seed)


def gates_r1cs(n, seed, mul_share=0.5):
    """A satisfiable R1CS of the shape the reference's circuit compiler emits (circuitcompiler/circuit.go:84-139, GenerateR1CS): every
    constraint is ONE flattened gate  out = u (op) v  over earlier signals, and
        `*`:   A = [u],     B = [v],    C = [out]
        `+`:   A = [u, v],  B = [one],  C = [out]
    so a signal enters B only as the second operand of a multiplication: with half the gates additions, ~60 % of the variables have
    b_i(x) = 0 and their G1.BACGamma / G2.BACGamma points are the point at infinity (what ProverKey::b_index is for).
    Variables [one, x (public), v_2 .. v_n] (m = n + 1, NPublic = 1); constraint j = 1..n-1 defines v_{j+1} from two uniformly chosen
    earlier variables (index 1..j); constraint n is one * one = one.  The values are full-width field elements after a few products.
    Returns (a_csr, b_csr, c_csr, w [m,4] uint64, counts)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    x = field_elems(1, seed + 10)[0]
    j = np.arange(1, n, dtype=np.int64)
    u = 1 + (rng.random(n - 1) * j).astype(np.int64)           # operands among variables 1 .. j
    v = 1 + (rng.random(n - 1) * j).astype(np.int64)
    is_mul = rng.random(n - 1) < mul_share
    is_mul[: min(8, n - 1)] = True                             # a few products first: the values become full-width at once
    var = j + 1
    same = (~is_mul) & (u == v)
    two = (~is_mul) & (u != v)
    lo, hi = np.minimum(u, v), np.maximum(u, v)
    # A: one entry for products (u) and for u + u (value 2), two sorted entries for u + v; last row {one: 1}
    a_per = np.concatenate((np.where(two, 2, 1), [1])).astype(np.uint32)
    a_rowptr = np.zeros(n + 1, dtype=np.uint32)
    a_rowptr[1:] = np.cumsum(a_per)
    nnz_a = int(a_rowptr[n])
    a_col = np.zeros(nnz_a, dtype=np.uint32)
    a_val = np.zeros((nnz_a, 4), dtype=np.uint64)
    first = a_rowptr[:-1][:n - 1].astype(np.int64)
    a_col[first] = np.where(two, lo, u)
    a_val[first, 0] = np.where(same, 2, 1)
    a_col[first[two] + 1] = hi[two]
    a_val[first[two] + 1, 0] = 1
    a_col[nnz_a - 1] = 0
    a_val[nnz_a - 1, 0] = 1
    one = np.zeros((n, 4), dtype=np.uint64)
    one[:, 0] = 1
    rowptr = np.arange(n + 1, dtype=np.uint32)
    b = (rowptr, np.concatenate((np.where(is_mul, v, 0), [0])).astype(np.uint32), one)
    c = (rowptr, np.concatenate((var, [0])).astype(np.uint32), one.copy())
    wit = [1, x % R] + [0] * (n - 1)
    ul, vl, ml = u.tolist(), v.tolist(), is_mul.tolist()
    for k in range(n - 1):
        wit[k + 2] = (wit[ul[k]] * wit[vl[k]] if ml[k] else wit[ul[k]] + wit[vl[k]]) % R
    in_b = np.zeros(n + 1, dtype=bool)
    in_b[0] = True
    in_b[v[is_mul]] = True
    counts = {"mul_gates": int(is_mul.sum()), "add_gates": int((~is_mul).sum()), "variables_in_B": int(in_b.sum()), "variables": n + 1}
    return (a_rowptr, a_col, a_val), b, c, capi.ints_to_u64(wit), counts


class GatesSetupInstance(SqchainSetupInstance):
    """SqchainSetupInstance's machinery (device trusted setup from seeded toxic values, px from the sparse system, the closed-form
    proof) on gates_r1cs: a circuit of the reference's own shape, whose key has most of its B points at infinity."""

    def __init__(self, n, seed, mul_share=0.5):
        from . import r1csqap
        self.n, self.m, self.seed = n, n + 1, seed
        self.toxic = field_elems(5, seed + 20)
        a, b, c, w, self.counts = gates_r1cs(n, seed, mul_share)
        self.r1cs = (a, b, c)
        self.w_host = w
        self._pk, self.vk = groth16.GenerateTrustedSetupSparse(n, self.m, 1, a, b, c, self.toxic)
        self.ax_host, self.bx_host, self.cx_host, self.px_host = r1csqap.ComputePx(a, b, c, w, self.m)
        self.w = capi.scalars_upload(self.w_host)
        self.px = capi.scalars_upload(self.px_host)

    def describe(self):
        return ("flattened-gate R1CS in the shape of the reference's circuit compiler (%(mul_gates)d `*` gates A=[u] B=[v], %(add_gates)d `+` gates "
                "A=[u,v] B=[one]; %(variables_in_B)d of %(variables)d variables appear in B), full-width witness, structured trusted setup on the device, "
                "px from the sparse system" % self.counts) + "; seed 0x%X" % self.seed


def gates_setup_instance(n, seed, mul_share=0.5):
    return GatesSetupInstance(n, seed, mul_share)


class SqchainPinocchioInstance:
    """The same sqchain(n) system under the Pinocchio protocol (snark.go): device trusted setup from 8 seeded toxic values
    (gs_pinocchio_setup = snark.go:98-251), resident witness and px.  The verifier (snark.VerifyProof, five pairing
    equations) is the end-to-end check at sizes the reference cannot replay."""

    def __init__(self, n, seed, extra_vars=0):
        from . import r1csqap, snark
        self.n, self.m, self.seed = n, n + 1 + extra_vars, seed
        self.toxic = field_elems(8, seed + 30)
        x = field_elems(1, seed + 10)[0]
        a, b, c, w = sqchain_r1cs(n, x, extra_vars)
        self.r1cs = (a, b, c)
        self.w_host = w
        self._pk, self.vk = snark.GenerateTrustedSetupSparse(n, self.m, 1, a, b, c, self.toxic)
        _, _, _, self.px_host = r1csqap.ComputePx(a, b, c, w, self.m)
        self.w = capi.scalars_upload(self.w_host)
        self.px = capi.scalars_upload(self.px_host)
        self.public = capi.u64_to_ints(self.w_host[1:2])

    def device_pk(self):
        return self._pk

    def describe(self):
        return ("sqchain(n) R1CS, satisfying witness, Pinocchio trusted setup on the device from seeded toxic values "
                "(gs_pinocchio_setup), px from the sparse system; seed 0x%X" % self.seed)


class GatesPinocchioInstance(SqchainPinocchioInstance):
    """gates_r1cs under the Pinocchio protocol: B (G2) and B' of its key are mostly the point at infinity (ProverKey::b_index)."""

    def __init__(self, n, seed, mul_share=0.5):
        from . import r1csqap, snark
        self.n, self.m, self.seed = n, n + 1, seed
        self.toxic = field_elems(8, seed + 30)
        a, b, c, w, self.counts = gates_r1cs(n, seed, mul_share)
        self.r1cs = (a, b, c)
        self.w_host = w
        self._pk, self.vk = snark.GenerateTrustedSetupSparse(n, self.m, 1, a, b, c, self.toxic)
        _, _, _, self.px_host = r1csqap.ComputePx(a, b, c, w, self.m)
        self.w = capi.scalars_upload(self.w_host)
        self.px = capi.scalars_upload(self.px_host)
        self.public = capi.u64_to_ints(self.w_host[1:2])

    def describe(self):
        return ("flattened * / + gates in the shape of the reference's circuit compiler (%d of %d variables in B), satisfying witness, "
                "Pinocchio trusted setup on the device from seeded toxic values, px from the sparse system; seed 0x%X"
                % (self.counts["variables_in_B"], self.counts["variables"], self.seed))


def gates_pinocchio_instance(n, seed, mul_share=0.5):
    return GatesPinocchioInstance(n, seed, mul_share)


class RandomPinocchioInstance:
    """A Pinocchio instance of the reference's shape (m = n + 1, NPublic = 1, len(Z) = len(hx) = n = len(G1T)) whose key points are
    k_i * G for seeded uniform k_i and whose w / px are seeded uniform field elements: what snark.GenerateProofs (snark.go:254-289)
    computes on it is pinned by a golden from the naive loops (oracle/gen_golden_large.py pinocchio)."""
    G1_ARRAYS = ("A", "Ap", "Bp", "C", "Cp", "Kp")

    def __init__(self, n, seed):
        from . import snark
        self.n, self.m, self.seed = n, n + 1, seed
        m = self.m
        g1 = {k: capi.g1_fixed_base(scalars_u64(m, seed + 1 + i)) for i, k in enumerate(self.G1_ARRAYS)}
        g1t = capi.g1_fixed_base(scalars_u64(n, seed + 7))
        b2 = capi.g2_fixed_base(scalars_u64(m, seed + 8))
        self.w_host = scalars_u64(m, seed + 9)
        self.w_host[0] = (1, 0, 0, 0)
        self.px_host = scalars_u64(2 * n - 1, seed + 10)
        self._pk = snark.device_pk_from_handles(B=b2, G1T=g1t, z_u64=capi.zpoly(m - 2), nvars=m, npublic=1, **g1)
        for x in list(g1.values()) + [g1t, b2]:
            x.free()
        self.w = capi.scalars_upload(self.w_host)
        self.px = capi.scalars_upload(self.px_host)

    def device_pk(self):
        return self._pk


def random_pinocchio_instance(n, seed):
    return RandomPinocchioInstance(n, seed)


class QuotientPinocchioInstance(RandomPinocchioInstance):
    """RandomPinocchioInstance with px = hx * Z + rem for seeded hx / rem (see QuotientInstance): the quotient snark.go:280 takes is
    known, so a complete golden proof can be computed outside the library at sizes where the schoolbook Div cannot."""

    def __init__(self, n, seed):
        import hashlib
        super().__init__(n, seed)
        self.hx_host = scalars_u64(n, seed + 11)
        self.px_host = px = _quotient_px(self.hx_host, capi.zpoly(self.m - 2), scalars_u64(n - 2, seed + 12))
        self.px_sha256 = hashlib.sha256(np.ascontiguousarray(px, dtype="<u8").tobytes()).hexdigest()
        self.px.free()
        self.px = capi.scalars_upload(px)


def quotient_pinocchio_instance(n, seed):
    return QuotientPinocchioInstance(n, seed)


def sqchain_pinocchio_instance(n, seed, extra_vars=0):
    return SqchainPinocchioInstance(n, seed, extra_vars)

