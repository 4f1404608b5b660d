"""-m gpu: gs_pinocchio_verify_each / snark.VerifyProofsEach / snark.VerifyProofsEachChecks -- the verdict and the first failing equation
per Pinocchio proof of a batch under one key, on the device.

Proofs of the committed x^3 + x + 5 key (wasm_pinocchio_x3_setup.json) from the device prover, one witness x = 3 + i per proof, as
test_gpu_verify_each.py builds its batch.  The yardstick is always the host verifier, one proof at a time: snark.VerifyProof's verdict
and gs_pinocchio_verify's failed_check.  Every changed position must get the host's answers, every other position (True, 0).  Sizes 1,
2, 65, 130: both sides of the one-wave workgroup seam, and the smallest at which the two-dimensional grid's workspace index can go
wrong.  Keys with 0 and 3 public inputs are made from known discrete logs (pinocchio_each_util.py)."""
import ctypes
import random

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, snark, utils
import golden_util as GU
import membership_util as M
import pinocchio_each_util as P
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R, Q = O.R, O.Q
NMAX = 130
SIZES = [1, 2, 65, 130]


@pytest.fixture(autouse=True)
def _init():
    capi.init()


@pytest.fixture(scope="module")
def batch():
    """(vk, proofs, public signal lists): NMAX valid proofs, each accepted by the host verifier for its own public input."""
    capi.init()
    rec = GU.load("pinocchio_x3_setup")
    opk = GU.pinocchio_pk(rec["setup"])
    _, vk = utils.SetupFromString(rec["setup"])
    circ = snark.Circuit(rec["circuit"]["NVars"], rec["circuit"]["NPublic"])
    pk = snark.Pk(G1T=opk.G1T, A=opk.A, B=opk.B, C=opk.C, Kp=opk.Kp, Ap=opk.Ap, Bp=opk.Bp, Cp=opk.Cp, Z=opk.Z)
    al, be, ga, _ = O.PF.R1CSToQAP(O.X3_R1CS_A, O.X3_R1CS_B, O.X3_R1CS_C)
    proofs, pubs = [], []
    for i in range(NMAX):
        x = 3 + i
        out = x ** 3 + x + 5
        w = [1, out, x, x * x, x ** 3, x ** 3 + x, out, 1]
        px = O.PF.CombinePolynomials(w, al, be, ga)[3]
        proofs.append(snark.GenerateProofs(circ, pk, w, px))
        pubs.append([out])
    assert all(snark.VerifyProof(vk, p, s) for p, s in zip(proofs[:3], pubs[:3]))
    assert not snark.VerifyProof(vk, proofs[0], pubs[1])
    return vk, proofs, pubs


def _key_args(vk):
    g1 = capi.g1_points_to_u64([vk.Vkb, vk.G1Kbg])
    g2 = capi.g2_points_to_u64([vk.Vka, vk.Vkc, vk.G2Kbg, vk.G2Kg, vk.Vkz])
    ic = capi.g1_points_to_u64(vk.IC)
    return (g1, g2, ic), (capi.ptr64(g2[0]), capi.ptr64(g1[0]), capi.ptr64(g2[1]), capi.ptr64(g1[1]), capi.ptr64(g2[2]), capi.ptr64(g2[3]),
                          capi.ptr64(g2[4]), capi.ptr64(ic), len(vk.IC))


def host(vk, proof, signals):
    """gs_pinocchio_verify on the signals as they are (no reduction) -> (ok, failed_check)."""
    keep, key = _key_args(vk)
    pub = capi.ints_to_u64(list(signals)) if signals else np.zeros((1, 4), dtype=np.uint64)
    words = snark._proof_words(proof)
    ok, bad = ctypes.c_int(7), ctypes.c_int(7)
    capi.check(capi.load_library().gs_pinocchio_verify(*key, capi.ptr64(pub), len(signals), capi.ptr64(words), ctypes.byref(ok), ctypes.byref(bad)))
    return bool(ok.value), bad.value


def raw_call(vk, proofs, pubs, nbad=True, failed=True):
    """gs_pinocchio_verify_each on the signals as they are -> rc, verdicts, failed equations, *nbad"""
    keep, key = _key_args(vk)
    npublic = len(pubs[0]) if pubs else 0
    flat = [x for s in pubs for x in s]
    pub = capi.ints_to_u64(flat) if flat else np.zeros((1, 4), dtype=np.uint64)
    words = np.ascontiguousarray(np.concatenate([snark._proof_words(p) for p in proofs]))
    ok, bad, count = np.full(len(proofs), 7, dtype=np.intc), np.full(len(proofs), 7, dtype=np.intc), ctypes.c_uint64(77)
    rc = capi.load_library().gs_pinocchio_verify_each(*key, capi.ptr64(pub), npublic, capi.ptr64(words), len(proofs), ok.ctypes.data_as(capi.intp),
                                                      bad.ctypes.data_as(capi.intp) if failed else None, ctypes.byref(count) if nbad else None)
    return rc, [int(x) for x in ok], [int(x) for x in bad], count.value


def agree(vk, proofs, pubs, changed, expect_false=True):
    """The device's answers against the host's at the changed positions and (True, 0) everywhere else; returns the failed equations."""
    got = snark.VerifyProofsEach(vk, proofs, pubs)
    checks = snark.VerifyProofsEachChecks(vk, proofs, pubs)
    assert len(got) == len(checks) == len(proofs)
    for i in range(len(proofs)):
        if i in changed:
            ok, bad = host(vk, proofs[i], [int(x) % R for x in pubs[i]])
            assert ok == snark.VerifyProof(vk, proofs[i], pubs[i])
            assert (got[i], checks[i]) == (ok, bad), i
            if expect_false:
                assert got[i] is False and 1 <= bad <= 5, i
        else:
            assert got[i] is True and checks[i] == 0, i
    return checks


def with_point(p, **kw):
    return snark.Proof(**{f: kw.get(f, getattr(p, f)) for f in snark.Proof.FIELDS})


@pytest.mark.parametrize("n", SIZES)
def test_valid_batches_get_true_and_no_failed_equation_everywhere(batch, n):
    vk, base, pubs = batch
    assert snark.VerifyProofsEach(vk, base[:n], pubs[:n]) == [True] * n
    assert snark.VerifyProofsEachChecks(vk, base[:n], pubs[:n]) == [0] * n


KINDS = ("PiA", "PiAp", "PiB", "PiBp", "PiC", "PiCp", "PiH", "PiKp", "public")


@pytest.mark.parametrize("n", SIZES)
def test_exactly_the_tampered_positions_get_the_hosts_verdict_and_equation(batch, n):
    vk, base, pubs = batch
    other_b = O.G2.MulScalar(O.G2_GEN, 12345)
    spots = sorted({0, n // 2, n - 1})
    seen = set()
    for shift in range(len(KINDS)):                                     # every kind of change visits every position
        proofs, signals = list(base[:n]), [list(s) for s in pubs[:n]]
        for k, at in enumerate(spots):
            p, what = base[at], KINDS[(k + shift) % len(KINDS)]
            if what == "public":
                signals[at][0] += 1
            elif what == "PiB":
                proofs[at] = with_point(p, PiB=other_b)
            else:
                proofs[at] = with_point(p, **{what: O.G1.Add(getattr(p, what), O.G1_GEN)})
        checks = agree(vk, proofs, signals, set(spots))
        seen.update(checks[at] for at in spots)
    assert seen == {1, 2, 3, 4, 5}, seen                                # every kind visited position 0: all five loops were reached


def test_special_points_and_several_bad_proofs(batch):
    vk, base, pubs = batch
    n = 130
    proofs, signals = list(base[:n]), [list(s) for s in pubs[:n]]
    proofs[7] = with_point(base[7], PiA=O.G1_ZERO)                                             # an infinite PiA
    proofs[8] = with_point(base[8], PiB=O.G2_ZERO)                                             # an infinite PiB
    proofs[66] = with_point(base[66], PiH=O.G1_ZERO)                                           # an infinite PiH
    x, y, z = base[64].PiC
    proofs[64] = with_point(base[64], PiC=(x, (y + 1) % Q, z))                                 # a PiC off the curve: a verdict, not an error
    outside = (M.twist_points(1)[0], M.complete_add(M.jac(O.G2.Affine(base[65].PiB)), M.small_order_point()),
               M.complete_add(M.jac(O.G2.Affine(base[100].PiB)), M.small_order_point()))
    assert not any(M.in_subgroup(b) for b in outside)
    proofs[0] = with_point(base[0], PiB=outside[0])                                            # a PiB on the twist outside G2
    proofs[65] = with_point(base[65], PiB=outside[1])
    proofs[100] = with_point(base[100], PiB=outside[2], PiAp=O.G1.Add(base[100].PiAp, O.G1_GEN))   # ... where equation 1 fails too
    proofs[20] = with_point(base[20], PiA=base[21].PiA)                                        # two more in the first workgroup
    proofs[21] = with_point(base[21], PiKp=base[20].PiKp)
    signals[3], signals[129] = signals[129], signals[3]                                       # swapped publics
    checks = agree(vk, proofs, signals, {7, 8, 66, 64, 0, 65, 100, 20, 21, 3, 129})
    assert checks[0] == 2 and checks[65] == 2 and checks[100] == 1
    assert checks[64] == 3 and checks[21] == 5 and checks[3] == 4


def test_debug_prints_the_line_of_the_failing_check(batch, capsys):
    vk, base, pubs = batch
    proofs = [base[0], with_point(base[1], PiCp=O.G1.Add(base[1].PiCp, O.G1_GEN)), base[2]]
    capsys.readouterr()
    assert not snark.VerifyProof(vk, proofs[1], pubs[1], debug=True)
    want = [line for line in capsys.readouterr().out.splitlines() if line.startswith("❌")]
    assert len(want) == 1
    assert snark.VerifyProofsEach(vk, proofs, pubs[:3], debug=True) == [True, False, True]
    lines = capsys.readouterr().out.splitlines()
    assert len(lines) == 1 and lines[0].endswith(want[0]) and lines[0].startswith("proof 1:")


def test_strict_mode_the_count_and_balanced_allocations(batch):
    vk, base, pubs = batch
    n = 65
    lib = capi.load_library()
    assert raw_call(vk, base[:n], pubs[:n]) == (0, [1] * n, [0] * n, 0)
    before = capi.alloc_counters()
    x, y, z = base[9].PiH
    aliased = list(base[:n])
    aliased[9] = with_point(base[9], PiH=(x + Q, y, z))
    noncanon = [list(s) for s in pubs[:n]]
    noncanon[64][0] += R
    assert raw_call(vk, aliased, noncanon) == (0, [1] * n, [0] * n, 0)  # the reference's big.Int behaviour: X + q names the same point
    assert host(vk, aliased[9], pubs[9]) == (True, 0) and host(vk, base[64], noncanon[64]) == (True, 0)
    try:
        assert lib.gs_verify_set_strict(1) == 0
        assert raw_call(vk, base[:n], pubs[:n]) == (0, [1] * n, [0] * n, 0)
        want = [0 if i in (9, 64) else 1 for i in range(n)]
        assert raw_call(vk, aliased, noncanon) == (0, want, [0] * n, 2)  # refused for the encoding: (False, 0)
        assert host(vk, aliased[9], pubs[9]) == (False, 0) and host(vk, base[64], noncanon[64]) == (False, 0)
    finally:
        lib.gs_verify_set_strict(0)
    rc, ok, bad, _ = raw_call(vk, aliased, noncanon, nbad=False, failed=False)
    assert rc == 0 and ok == [1] * n and bad == [7] * n
    after = capi.alloc_counters()
    assert after[0] - before[0] == after[1] - before[1]                 # every temporary array is freed on every path


def test_a_key_point_off_its_curve_gives_what_the_host_gives(batch):
    vk, base, pubs = batch
    n = 4
    tampered = with_point(base[1], PiA=O.G1.Add(base[1].PiA, O.G1_GEN))  # fails equation 1 before the key point is used
    proofs = [base[0], tampered, base[2], with_point(base[3], PiH=O.G1_ZERO)]
    before = capi.alloc_counters()
    (zx, zy, zz) = vk.Vkz
    keys = {"Vkz": snark.Vk(IC=vk.IC, **{f: (getattr(vk, f) if f != "Vkz" else (zx, ((zy[0] + 1) % Q, zy[1]), zz)) for f in snark.Vk.FIELDS})}
    bx, by, bz = vk.Vkb
    keys["Vkb"] = snark.Vk(IC=vk.IC, **{f: (getattr(vk, f) if f != "Vkb" else (bx, (by + 1) % Q, bz)) for f in snark.Vk.FIELDS})
    ix, iy, iz = vk.IC[1]
    keys["IC"] = snark.Vk(IC=[vk.IC[0], (ix, (iy + 1) % Q, iz)], **{f: getattr(vk, f) for f in snark.Vk.FIELDS})
    firsts = {"Vkz": 4, "Vkb": 2, "IC": 4}
    for name, bad_key in keys.items():
        want = [host(bad_key, p, s) for p, s in zip(proofs, pubs[:n])]
        assert [w[1] for w in want] == [firsts[name], 1, firsts[name], firsts[name]], name
        rc, ok, bad, count = raw_call(bad_key, proofs, pubs[:n])
        assert (rc, count) == (0, n) and list(zip(map(bool, ok), bad)) == want, name
    after = capi.alloc_counters()
    assert after[0] - before[0] == after[1] - before[1]


def dlog_batch(npublic, n, seed):
    """A key with npublic inputs and n proofs from known discrete logs; every odd proof has one exponent moved.  Proof 0 has a = -vkx, so
    vkx + PiA is infinite; with inputs, proof 2 carries a 256-bit signal at or above r.  -> vk, proofs, signals"""
    rng = random.Random(seed)
    key = P.dlog_key(npublic, rng)
    vk = snark.Vk(**P.vk_points(key))
    proofs, signals = [], []
    for i in range(n):
        sig = [rng.choice((0, 1, R - 1, rng.randrange(R))) for _ in range(npublic)]
        if i == 2 and npublic:
            sig[0] = R + rng.randrange(2 ** 256 - R)
        e = P.dlog_proof(key, sig, rng, a=-P.vkx_of(key, sig) if i == 0 else None)
        if i % 2:
            moved = P.NAMES[(i // 2) % len(P.NAMES)]
            e[moved] = (e[moved] + 1) % R
        proofs.append(snark.Proof(**P.proof_points(e)))
        signals.append(sig)
    return vk, proofs, signals


@pytest.mark.parametrize("npublic", [0, 3])
def test_keys_with_0_and_3_public_inputs_from_known_discrete_logs(npublic):
    n = 18
    vk, proofs, signals = dlog_batch(npublic, n, 700 + npublic)
    want = [host(vk, p, s) for p, s in zip(proofs, signals)]
    assert [w[0] for w in want] == [i % 2 == 0 for i in range(n)]       # the construction accepts, the moved exponent does not
    assert {w[1] for w in want} == {0, 1, 2, 3, 4, 5}
    rc, ok, bad, count = raw_call(vk, proofs, signals)
    assert (rc, count) == (0, n // 2) and list(zip(map(bool, ok), bad)) == want


def test_ragged_input_raises(batch):
    vk, base, pubs = batch
    with pytest.raises(ValueError):
        snark.VerifyProofsEach(vk, base[:2], pubs[:1])
    with pytest.raises(ValueError):
        snark.VerifyProofsEachChecks(vk, base[:2], [pubs[0], []])
    assert snark.VerifyProofsEach(vk, [], []) == [] and snark.VerifyProofsEachChecks(vk, [], []) == []
