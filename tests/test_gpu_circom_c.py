"""-m gpu: tests/c/circom_prove.c -- upload, prove, verify with a key over a power-of-two domain from a process without Python: the C
call sequence of go/gosnarkhip/domain.go, on a k = 3 instance this test writes out."""
import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi
import c_util
import circom_util as CU
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = CU.R


def test_circom_prove_c_sequence_proves_and_verifies(tmp_path):
    k, m = 3, 8
    inst = CU.Instance(k, m - 1, 11)
    r, s = 0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321fedcba0987654321
    px = CU.px_naive(inst.rows_a, inst.rows_b, inst.rows_c, inst.w, k)
    dense = [[[row.get(v, 0) for v in range(inst.nvars)] for row in rows] for rows in (inst.rows_a, inst.rows_b, inst.rows_c)]
    r1cs = c_util.write_r1cs(tmp_path, dense, inst.npublic, [])
    g1 = lambda ks: [O.G1.MulScalar(O.G1_GEN, x) if x else (0, 1, 0) for x in ks]                       # noqa: E731
    g2 = lambda ks: [O.G2.MulScalar(O.G2_GEN, x) if x else ((0, 0), (1, 0), (0, 0)) for x in ks]      # noqa: E731
    ginv = pow(inst.gamma, -1, R)
    ic = [(inst.beta * inst.at[i] + inst.alpha * inst.bt[i] + inst.ct[i]) * ginv % R for i in range(inst.npublic + 1)]
    public = inst.w[1:1 + inst.npublic]
    parts = [np.array([inst.nvars, len(px), m + 1, m + 1, len(ic), inst.npublic], dtype=np.uint64),
             capi.g1_points_to_u64(g1(inst.at)), capi.g1_points_to_u64(g1(inst.bt)), capi.g2_points_to_u64(g2(inst.bt)),
             capi.g1_points_to_u64(g1(inst.cd)), capi.g1_points_to_u64(g1(inst.hexps)),
             capi.g1_points_to_u64(g1([inst.alpha, inst.beta, inst.delta])), capi.g2_points_to_u64(g2([inst.beta, inst.delta])),
             capi.ints_to_u64([R - 1] + [0] * (m - 1) + [1]), CU.u64(inst.w), CU.u64(px), capi.ints_to_u64([r, s]),
             capi.g1_points_to_u64(g1([inst.alpha])), capi.g2_points_to_u64(g2([inst.beta, inst.gamma, inst.delta])),
             capi.g1_points_to_u64(g1(ic)), CU.u64(public)]
    blob = c_util._blob(str(tmp_path / "circom_instance.bin"), parts)
    out = tmp_path / "proof.bin"
    assert c_util.build_and_run("circom_prove.c", [str(r1cs), str(blob), str(k), str(out)], tmp_path).strip() == "OK"
    v = capi.u64_to_ints(c_util.read_words(out))
    a, b, c = inst.expected_scalars(inst.w, r, s)
    wb = C.g2_affine(C.g2_mul_scalar(O.G2_GEN, b))
    assert (v[0], v[1]) == C.g1_affine(C.g1_mul_scalar(O.G1_GEN, a))
    assert ((v[2], v[3]), (v[4], v[5])) == wb
    assert (v[6], v[7]) == C.g1_affine(C.g1_mul_scalar(O.G1_GEN, c))
