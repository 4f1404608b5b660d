"""Compressed points with Python integers, for the point-codec tests: square roots in Fq and Fq2 (checked by squaring), the sign rule,
and the (x, flag) encoding of the oracle's points.  Test infrastructure."""
from oracle import ref_py as O

Q = O.Q
F2 = O.FQ2
TWIST_B = F2.Mul(F2.Inverse((9, 1)), (3, 0))
LARGEST, INFINITY = 1, 2


def fq_sqrt(a):
    """A root of a in Fq, or None."""
    y = pow(a, (Q + 1) // 4, Q)
    return y if y * y % Q == a % Q else None


def fq2_sqrt(a):
    """A root of a = (a0, a1) in Fq2, or None: the complex method with an inversion, every candidate checked by squaring."""
    a0, a1 = a[0] % Q, a[1] % Q
    if (a0, a1) == (0, 0):
        return (0, 0)
    if a1 == 0:
        y = fq_sqrt(a0)
        if y is not None:
            return (y, 0)
        y = fq_sqrt(Q - a0)
        assert y is not None                                   # -1 is a non-residue: one of a0, -a0 has a root
        return (0, y)
    s = fq_sqrt((a0 * a0 + a1 * a1) % Q)
    if s is None:
        return None
    for sgn in (s, Q - s):
        y0 = fq_sqrt((a0 + sgn) * pow(2, Q - 2, Q) % Q)
        if y0:
            y = (y0, a1 * pow(2 * y0, Q - 2, Q) % Q)
            if F2.Square(y) == (a0, a1):
                return y
    raise AssertionError("a residue norm without a root")


def fq_larger(y):
    return y > Q - y


def fq2_larger(y):
    return fq_larger(y[1]) if y[1] else fq_larger(y[0])


def g1_rhs(x):
    return (pow(x, 3, Q) + 3) % Q


def g2_rhs(x):
    return F2.Add(F2.Mul(F2.Square(x), x), TWIST_B)


def g1_point(x, largest):
    """The affine point (x, y) with the root the flag asks for, or None when x^3 + 3 has no root."""
    y = fq_sqrt(g1_rhs(x))
    if y is None:
        return None
    return (x, y if fq_larger(y) == bool(largest) else Q - y)


def g2_point(x, largest):
    y = fq2_sqrt(g2_rhs(x))
    if y is None:
        return None
    return (x, y if fq2_larger(y) == bool(largest) else ((-y[0]) % Q, (-y[1]) % Q))


def g1_encoding(p):
    """A Jacobian triple of the oracle -> (x, flag)."""
    a = O.G1.Affine(p)
    return (0, INFINITY) if a is None else (a[0], LARGEST if fq_larger(a[1]) else 0)


def g2_encoding(p):
    a = O.G2.Affine(p)
    return ((0, 0), INFINITY) if a is None else (a[0], LARGEST if fq2_larger(a[1]) else 0)
