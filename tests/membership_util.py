"""Points of the twist E'(Fq2) inside and outside G2 for the membership tests, all from oracle/ref_py: random twist points (the
construction of test_verifier.py), their cofactor-cleared images, a point S of order 10069 (the smallest prime factor of the cofactor
2q - r) and mixed points G + S.  Also the oracle-side psi, from the definition of its two constants.  Test infrastructure."""
import functools

from oracle import ref_py as O

Q, R = O.Q, O.R
F2, G2 = O.FQ2, O.G2
COFACTOR = 2 * Q - R
SMALL = 10069
BN_X = 4965661367192848881
assert COFACTOR % SMALL == 0 and (COFACTOR // SMALL) % SMALL != 0


def complete_add(a, b):
    """The oracle's Add has no P == Q branch."""
    if G2.IsZero(a):
        return b
    if G2.IsZero(b):
        return a
    if G2.Equal(a, b):
        return G2.Double(a)
    return G2.Add(a, b)


def affine(p):
    """(x, y) with x, y pairs of ints, or None for infinity."""
    return G2.Affine(p)


def jac(a):
    return O.G2_ZERO if a is None else (a[0], a[1], (1, 0))


def in_subgroup(p):
    """The definition: [r] P = O."""
    return G2.IsZero(p) or G2.Affine(G2.MulScalar(p, R)) is None


def twist_points(count, start=1):
    """The first `count` twist points with x = (k, 1), k >= start: outside G2 with overwhelming probability."""
    b_twist = F2.Mul(F2.Inverse((9, 1)), (3, 0))
    out, k = [], start
    while len(out) < count:
        x = (k, 1)
        a0, a1 = F2.Add(F2.Mul(F2.Square(x), x), b_twist)
        norm = (a0 * a0 + a1 * a1) % Q
        s = pow(norm, (Q + 1) // 4, Q)                  # square root in Fq2 via the norm (q = 3 mod 4)
        if s * s % Q == norm:
            for sgn in (s, Q - s):
                t = (a0 + sgn) * pow(2, Q - 2, Q) % Q
                y0 = pow(t, (Q + 1) // 4, Q)
                if y0 * y0 % Q == t and y0:
                    y1 = a1 * pow(2 * y0, Q - 2, Q) % Q
                    if F2.Square((y0, y1)) == (a0, a1):
                        out.append((x, (y0, y1), (1, 0)))
                        break
        k += 1
    return out


@functools.lru_cache(maxsize=None)
def small_order_point(which=0):
    """S = [r (2q - r) / 10069] T for the which-th twist point T whose image is not infinity: a point of order exactly 10069."""
    found = -1
    for t in twist_points(8 + which):
        s = G2.MulScalar(t, R * (COFACTOR // SMALL))
        if not G2.IsZero(s) and G2.Affine(s) is not None:
            found += 1
            if found == which:
                assert G2.Affine(G2.MulScalar(s, SMALL)) is None
                return jac(G2.Affine(s))
    raise AssertionError("no point of order 10069 among the first twist points")


def subgroup_multiples(n, first=1):
    """first * G2, (first + 1) * G2, ... by repeated addition: n subgroup points without long scalar multiplications."""
    p = G2.MulScalar(O.G2_GEN, first)
    out = []
    for _ in range(n):
        out.append(jac(G2.Affine(p)))
        p = complete_add(p, O.G2_GEN)
    return out


def _f2_pow(a, e):
    r = (1, 0)
    while e:
        if e & 1:
            r = F2.Mul(r, a)
        a = F2.Square(a)
        e >>= 1
    return r


PSI_GX = _f2_pow((9, 1), (Q - 1) // 3)
PSI_GY = _f2_pow((9, 1), (Q - 1) // 2)


def psi(p):
    """(conj(x) xi^((q-1)/3), conj(y) xi^((q-1)/2)) on the affine form."""
    a = G2.Affine(p)
    if a is None:
        return O.G2_ZERO
    conj = lambda v: (v[0], (-v[1]) % Q)   # noqa: E731
    return (F2.Mul(conj(a[0]), PSI_GX), F2.Mul(conj(a[1]), PSI_GY), (1, 0))
