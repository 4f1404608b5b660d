"""-m gpu: the sort plan (k_digits -> k_hist -> k_colscan -> k_scatter, msm_kernels.h) at the seams of its workgroup map and of its
digit format, against the oracle's naive loop `acc = Add(acc, MulScalar(base_i, k_i))` (oracle/gs_oracle.c), as tests/test_gpu_msm.py.

The workgroup map gives window w the ids with id % 8 == w % 8 and pads W to a multiple of 8; the digit matrix keeps 16-bit bucket
numbers (up to c = 17) beside a skip and a sign bit plane, read 8 terms at a time over rows padded to 64 terms.  So: widths whose
window count is and is not a multiple of 8, one and two bucket ranges, one slice, several slices, a ragged last slice, term counts
that are no multiple of 8 or 64, the table-free route, a plan over a term list, and the digits at the ends of the code."""
import numpy as np
import pytest

import gosnark_amd
from gosnark_amd import capi, groth16
import gpu_util as U
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu

N_MAX = (1 << 17) + 3
CUTS = [1, 63, 5000, 16385, 40000, N_MAX]
_shared = {}


@pytest.fixture(scope="module", autouse=True, params=["always", "never"])
def _init(request):
    """every test on window tables and table-free (a forced width is clamped to 9..16 there: W = 16 windows, one range)"""
    capi.init()
    capi.set_table_policy(request.param)
    yield request.param
    capi.set_window_bits(0)
    capi.set_table_policy("auto")
    bases = _shared.pop("bases", None)          # with its window table: nothing of this module stays resident for the tests that follow
    if bases is not None:
        bases.free()


def _reference():
    """One pass of the naive loop over N_MAX seeded terms, cut at every term count the tests use: want[n] = the sum of the first n terms."""
    if "bases" not in _shared:
        _shared["bases"] = capi.g1_fixed_base(U.rand_scalars_u64(N_MAX, 0x5018))      # uniform random group elements
    if "want" not in _shared:
        ks = U.rand_scalars_u64(N_MAX, 0x5017)
        pts = capi.g1_download(_shared["bases"])
        want, acc, lo = {}, O.G1_ZERO, 0
        for hi in CUTS:
            part = C.g1_affine(C.g1_msm_naive(pts[lo:hi], ks[lo:hi], threads=8))
            acc = O.G1.Add(acc, (part[0], part[1], 1))
            want[hi] = O.G1.Affine(acc)
            lo = hi
        _shared.update(ks=ks, want=want)
    return _shared["bases"], _shared["ks"], _shared["want"]


def _msm_at(c, bases, ks):
    capi.set_window_bits(c)
    try:
        return capi.msm(bases, ks)
    finally:
        capi.set_window_bits(0)


@pytest.mark.parametrize("n", [1, 63, 16385, 40000, N_MAX])
def test_width_17_fifteen_windows_two_ranges(n):
    """c = 17: W = 15 windows (padded to 16 by the map), R = 2 bucket ranges; one slice (n <= 16384), several, a ragged last one."""
    bases, ks, want = _reference()
    assert _msm_at(17, bases, ks[:n]) == want[n]


@pytest.mark.parametrize("c", [16, 15])
def test_neighbouring_widths(c):
    """c = 16 (W = 16, a multiple of 8, R = 1) and c = 15 (W = 17: three rounds of 8 windows, seven padded)."""
    bases, ks, want = _reference()
    assert _msm_at(c, bases, ks[:40000]) == want[40000]


def test_table_free_route_width_13(_init):
    """Per-window bucket sets (W = 20 windows, padded to 24 by the map), under either policy of the module."""
    bases, ks, want = _reference()
    capi.set_table_policy("never")
    try:
        assert _msm_at(13, bases, ks[:5000]) == want[5000]
    finally:
        capi.set_table_policy(_init)


def test_digits_at_the_ends_of_the_code():
    """0 (every digit skipped), 1, r - 1, values >= r (reduced mod r), and scalars whose c = 17 digits are all +65536 (the largest bucket,
    0xffff in the 16-bit row; -65536 does not occur: digits lie in [-B + 1, B]), all -65535, all +1 and all -1 (the sign plane set in
    every window, everything in bucket 0: the heaviest bucket), among random ones; 203 terms, so the last group of 8 and the last plane
    word are ragged."""
    c, top = 17, 14
    every = lambda lo, rest, last: lo + sum(rest << (c * w) for w in range(1, top)) + (last << (c * top))      # noqa: E731
    special = [0, 1, O.R - 1, O.R, O.R + 5, 2 * O.R + 1, (1 << 256) - 1,
               every(1 << 16, 1 << 16, 1),                    # digits +65536 x 14, then +1
               every((1 << 16) + 1, 1 << 16, 0),              # 65537 -> -65535 and a carry, then 65536 + 1 likewise x 13; the carry ends as +1
               every(1, 1, 1),                                # digits +1
               every((1 << c) - 1, (1 << c) - 2, 0)]          # digits -1 x 14, the carry ends as +1
    assert all(k < O.R for k in special[7:])
    rnd = U.u64_rows_to_ints(U.rand_scalars_u64(203, 0x5019))
    ks = [special[i % len(special)] if i % 3 else rnd[i] for i in range(203)]
    ks[200:203] = [special[7], special[10], 0]
    bases = capi.g1_fixed_base(U.rand_scalars_u64(203, 0x501A))
    sc = capi.ints_to_u64(ks)
    want = C.g1_affine(C.g1_msm_naive(capi.g1_download(bases), sc, threads=8))
    assert _msm_at(17, bases, sc) == want
    assert _msm_at(16, bases, sc) == want


def test_width_17_plan_over_a_term_list():
    """A key whose B arrays are mostly the point at infinity: B1 and B2 are summed over a second plan of w that lists only the terms with
    a finite B point (ProverKey::b_index; about a third of 90 000 variables), here at c = 17.  The proof is pinned by the closed form of
    the setup's toxic values, as tests/test_gpu_prove.py pins such keys."""
    from gosnark_amd import synth
    n = 90000
    inst = synth.gates_setup_instance(n, 0x9517)
    listed = inst.counts["variables_in_B"]
    assert 22000 < listed < 41000, inst.counts
    r, s = synth.field_elems(2, 0x9518)
    capi.set_window_bits(17)
    try:
        got = groth16.prove_resident(inst.device_pk(), inst.w, inst.px, r, s)
        tm = capi.last_timing()
    finally:
        capi.set_window_bits(0)
    a, b, c = inst.expected_proof_scalars(r, s)
    assert (got.PiA[0], got.PiA[1]) == C.g1_affine(C.g1_mul_scalar(O.G1_GEN, a))
    assert (got.PiB[0], got.PiB[1]) == C.g2_affine(C.g2_mul_scalar(O.G2_GEN, b))
    assert (got.PiC[0], got.PiC[1]) == C.g1_affine(C.g1_mul_scalar(O.G1_GEN, c))
    windows = 254 // tm["window_bits"] + 1
    assert tm["acc_g2_adds"] < 0.5 * windows * n, (tm["acc_g2_adds"], windows * n)      # the G2 sum ran over the listed terms only


def test_flagship_slices_with_a_ragged_tail():
    """2^20 + 4097 terms at c = 17: the flagship's eight slices per window and range, 131 648 terms each (whole plane words), the last
    one short and ending inside a group of 8.  Too many terms for the naive loop: with bases P_i = k_i G the sum is
    (sum_i s_i k_i mod r) G, as tests/test_gpu_msm.py checks its full-size MSMs."""
    n = (1 << 20) + 4097
    k, s = U.rand_scalars_u64(n, 0x501B), U.rand_scalars_u64(n, 0x501C)
    bases = capi.g1_fixed_base(k)
    dot = sum(a * b for a, b in zip(U.u64_rows_to_ints(k), U.u64_rows_to_ints(s))) % O.R
    assert _msm_at(17, bases, s) == O.G1.Affine(O.G1.MulScalar(O.G1_GEN, dot))
    bases.free()
