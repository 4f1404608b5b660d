"""The scaling-table index and exponent functions of the power-of-two domain QAP (csrc/domain.h), instantiated on the HOST
(tests/host/domain_host_test.hip) and compared with Python's pow: which frequency a slot of the engine's bit-reversed spectrum holds,
which power of g = 5^((r-1)/(2m)) multiplies it in the coset extension (g^((-f) mod m) / m) and in the evaluation-basis derivation
(g^((-i) mod 2m)), and where coefficient i of an interpolant sits.  No GPU."""
import pytest

import hostbuild
import circom_util as CU

R = CU.R


@pytest.fixture(scope="module")
def exe():
    return hostbuild.build("domain_host_test")


def bitrev(k, p):
    return int(format(p, "0%db" % k)[::-1], 2)


@pytest.mark.parametrize("k", [1, 2, 3, 7, 11])
def test_table_function_matches_python_pow(exe, k):
    m = 1 << k
    g = CU.coset_gen(k)
    assert pow(g, 2, R) == CU.omega(k) and pow(g, m, R) == R - 1
    (line,) = hostbuild.run_lines(exe, [str(k)])
    recs = line.split(" ")
    assert len(recs) == m
    minv = pow(m, -1, R)
    seen = set()
    for p, rec in enumerate(recs):
        slot, f, e, d, cs, val = rec.split(":")
        assert int(slot) == p and int(f) == bitrev(k, p)
        f = int(f)
        assert int(e) == (-f) % m and int(d) == (-f) % (2 * m)
        assert int(val, 16) == pow(g, (-f) % m, R) * minv % R
        assert pow(g, int(d), R) == pow(g, -f, R)                              # the derivation's g^(-i)
        assert int(cs) == bitrev(k, (-p) % m)                                  # coefficient p = frequency (-p) mod m
        seen.add(f)
    assert seen == set(range(m))
