"""-m gpu: circom.VerifyZkey -- a circuit.zkey checked against circuit.r1cs and a powers-of-tau file on the device
(gs_groth16_key_check).

The circuits and transcripts are those of test_gpu_setup_ptau.py (setup_util.Circuit: toxic values known), so both points of every
check are generator multiples with a closed form in Python integers: sum_i rho_i at[i], bt, kk over the public / private signals,
sum_j sigma_j H_j, each divided by delta on the key's side; rho_i = sigma_i = s^(i+1).  Points are compared bit for bit with the C
oracle's scalar multiplication.  Every tampering must fail exactly the checks it touches and pass all the others.  Seeds are fixed."""
import random

import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom
import circom_util as CU
from setup_util import Circuit
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R, Q = CU.R, circom.Q
SHAPES = {"k1": (1, 0, 1), "k3_full": (3, 3, 4), "k3": (3, 1, 3), "k10": (10, 1, 600)}      # name -> (k, nPublic, nConstraints)
SEED = 20261019
ALL = ["header", "delta"] + list(capi.KEY_CHECKS)


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    yield
    capi.set_table_policy("auto")


_BUILT = {}


def built(name, extra_power, tmp_path_factory):
    """-> (Circuit, paths); one setup per (shape, power) and session"""
    key = (name, extra_power)
    if key not in _BUILT:
        k, npub, nc = SHAPES[name]
        c = Circuit(k, npub, nc, 1000 + 10 * k + npub)
        d = tmp_path_factory.mktemp("check_%s_%d" % key)
        paths = {n: str(d / n) for n in ("c.r1cs", "t.ptau", "c.zkey")}
        c.write_r1cs(paths["c.r1cs"])
        circom.WritePtau(paths["t.ptau"], k + extra_power, c.tau, c.alpha, c.beta)
        circom.SetupFromPtau(paths["c.r1cs"], paths["t.ptau"], paths["c.zkey"])
        _BUILT[key] = (c, paths)
    return _BUILT[key]


def g1_affine(k):
    return tuple(C.g1_affine(C.g1_mul_scalar(O.G1_GEN, k % R))) if k % R else None


def g2_affine(k):
    p = C.g2_affine(C.g2_mul_scalar(O.G2_GEN, k % R))
    return (tuple(p[0]), tuple(p[1]))


def closed_forms(c, s, with_last, delta=1):
    """check name -> (lhs scalar, rhs scalar) of the generator"""
    rho = [pow(s, i + 1, R) for i in range(max(c.nvars, c.m))]
    dot = lambda xs, lo, hi: sum(rho[i] * xs[i] for i in range(lo, hi)) % R      # noqa: E731
    dinv = pow(delta, -1, R)
    h = sum(rho[j] * x for j, x in enumerate(c.h_scalars(with_last))) % R
    kc = dot(c.kk, c.npub + 1, c.nvars)
    return {"A": (dot(c.at, 0, c.nvars),) * 2, "B1": (dot(c.bt, 0, c.nvars),) * 2, "B2": (dot(c.bt, 0, c.nvars),) * 2,
            "IC": (dot(c.kk, 0, c.npub + 1),) * 2, "C": (kc * dinv % R, kc), "H": (h * dinv % R, h)}


def assert_closed_forms(rep, c, with_last, delta=1):
    for name, (lhs, rhs) in closed_forms(c, rep.seed, with_last, delta).items():
        pt = g2_affine if name == "B2" else g1_affine
        assert rep.points[name] == (pt(lhs), pt(rhs)), name
    assert rep.points["coefs A"][0] == 0 and rep.points["coefs B"][0] == 0


def sections(path):
    return circom._read_sections(path, b"zkey", 1, circom._ZKEY_NAMES, range(1, 10))[1]


def patched(src, dst, edits):
    """a copy of the file with (offset, bytes) written over it"""
    data = bytearray(open(src, "rb").read())
    for off, b in edits:
        data[off:off + len(b)] = b
    with open(dst, "wb") as f:
        f.write(bytes(data))
    return dst


def some_g1(k):
    x, y = g1_affine(k)
    return circom.G1ToZkey((x, y, 1))


def expect(rep, failed):
    assert [n for n, _, _, _ in rep.checks] == ALL
    assert sorted(rep.failed) == sorted(failed), rep
    assert bool(rep) == (not failed)


@pytest.mark.parametrize("extra_power", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_a_key_is_accepted_with_the_closed_forms_of_every_check(name, extra_power, tmp_path_factory):
    c, paths = built(name, extra_power, tmp_path_factory)
    rep = circom.VerifyZkey(paths["c.r1cs"], paths["t.ptau"], paths["c.zkey"], seed=SEED + extra_power)
    expect(rep, [])
    assert isinstance(rep, circom.ZkeyReport)
    assert_closed_forms(rep, c, with_last=extra_power > 0)


@pytest.mark.parametrize("name,extra_power", [("k3", 1), ("k3_full", 0)])
def test_a_contributed_key_is_accepted(name, extra_power, tmp_path_factory):
    c, paths = built(name, extra_power, tmp_path_factory)
    delta = random.Random(9).randrange(2, R)
    out = paths["c.zkey"] + ".contributed"
    circom.ContributeDelta(paths["c.zkey"], out, delta)
    rep = circom.VerifyZkey(paths["c.r1cs"], paths["t.ptau"], out, seed=SEED)
    expect(rep, [])
    assert_closed_forms(rep, c, with_last=extra_power > 0, delta=delta)
    # ... and with the H section of the key before the contribution copied back it is not
    sec = sections(out)
    h0 = open(paths["c.zkey"], "rb").read()[sec[9][0]:sec[9][0] + sec[9][1]]
    expect(circom.VerifyZkey(paths["c.r1cs"], paths["t.ptau"], patched(out, out + ".h", [(sec[9][0], h0)]), seed=SEED), ["H"])


def test_a_random_challenge_is_drawn_when_no_seed_is_given(tmp_path_factory):
    c, paths = built("k3", 0, tmp_path_factory)
    a, b = (circom.VerifyZkey(paths["c.r1cs"], paths["t.ptau"], paths["c.zkey"]) for _ in range(2))
    assert a and b and a.seed != b.seed and 0 < a.seed < R


def _tamperings(c, paths, tmp):
    """name -> (zkey path, the checks that must fail)"""
    src, sec = paths["c.zkey"], sections(paths["c.zkey"])
    data = open(src, "rb").read()
    pt = lambda sid, i, size=64: data[sec[sid][0] + i * size:sec[sid][0] + (i + 1) * size]      # noqa: E731
    out = {}
    i, j = next((i, j) for i in range(c.nvars) for j in range(i + 1, c.nvars) if c.at[i] != c.at[j])
    out["A swapped"] = ([(sec[5][0] + i * 64, pt(5, j)), (sec[5][0] + j * 64, pt(5, i))], ["A"])
    out["B1 replaced"] = ([(sec[6][0] + (c.nvars - 1) * 64, some_g1(77))], ["B1"])
    out["B2 replaced"] = ([(sec[7][0] + 128, pt(7, 0, 128) if c.bt[0] != c.bt[1] else pt(7, 2, 128))], ["B2"])
    out["IC[0] replaced"] = ([(sec[3][0], some_g1(78))], ["IC"])
    last = c.nvars - c.npub - 2                                # the last product wire: it stands in C's matrix, so its point is finite
    x, y, _ = circom.G1FromZkey(pt(8, last))
    out["C negated"] = ([(sec[8][0] + last * 64, circom.G1ToZkey((x, Q - y, 1)))], ["C"])
    out["H[m-1] replaced"] = ([(sec[9][0] + (c.m - 1) * 64, some_g1(79))], ["H"])
    d1 = sec[2][0] + sec[2][1] - 192
    out["delta1 replaced"] = ([(d1, some_g1(80))], ["delta"])
    rec = sec[4][0] + 4 + 12                                    # the value of the first record of section 4: a term of A
    out["coefficient changed"] = ([(rec, bytes([data[rec] ^ 1]))], ["coefs A"])
    return {n: (patched(src, str(tmp / ("t%d.zkey" % k)), e), f) for k, (n, (e, f)) in enumerate(out.items())}


@pytest.mark.parametrize("name,extra_power", [("k3", 0), ("k3_full", 1)])
def test_a_tampered_key_fails_exactly_the_checks_it_touches(name, extra_power, tmp_path_factory, tmp_path):
    c, paths = built(name, extra_power, tmp_path_factory)
    for what, (zkey, failed) in _tamperings(c, paths, tmp_path).items():
        rep = circom.VerifyZkey(paths["c.r1cs"], paths["t.ptau"], zkey, seed=SEED)
        assert sorted(rep.failed) == sorted(failed), (what, rep)
        assert not rep


def test_a_tampered_point_among_many_is_found(tmp_path_factory, tmp_path):
    c, paths = built("k10", 0, tmp_path_factory)
    sec = sections(paths["c.zkey"])
    zkey = patched(paths["c.zkey"], str(tmp_path / "t.zkey"), [(sec[6][0] + 333 * 64, some_g1(81))])
    expect(circom.VerifyZkey(paths["c.r1cs"], paths["t.ptau"], zkey, seed=SEED), ["B1"])


@pytest.mark.parametrize("name", ["k3", "k3_full"])
def test_the_last_power_rule_of_h(name, tmp_path_factory):
    """a key set up from the transcript of 2m - 1 tauG1 points against the transcript of the same toxic values that holds 2m, and back"""
    _, p0 = built(name, 0, tmp_path_factory)
    _, p1 = built(name, 1, tmp_path_factory)
    expect(circom.VerifyZkey(p0["c.r1cs"], p1["t.ptau"], p0["c.zkey"], seed=SEED), ["H"])
    expect(circom.VerifyZkey(p0["c.r1cs"], p0["t.ptau"], p1["c.zkey"], seed=SEED), ["H"])


def test_a_transcript_of_another_tau_fails_everything_but_the_coefficients(tmp_path_factory, tmp_path):
    c, paths = built("k3", 0, tmp_path_factory)
    other = str(tmp_path / "other.ptau")
    circom.WritePtau(other, c.k, c.tau + 1, c.alpha, c.beta)
    expect(circom.VerifyZkey(paths["c.r1cs"], other, paths["c.zkey"], seed=SEED), ["A", "B1", "B2", "IC", "C", "H"])


@pytest.mark.parametrize("name", ["k3", "k3_full"])
def test_a_changed_circuit_fails_the_checks_that_hold_the_signal(name, tmp_path_factory, tmp_path):
    c, paths = built(name, 0, tmp_path_factory)
    write = lambda cons: circom.WriteR1cs(str(tmp_path / "x.r1cs"), c.nvars, 0, c.npub, 1, cons)      # noqa: E731
    # one C coefficient of a private signal
    cons = [tuple(list(lc) for lc in con) for con in c.constraints]
    wire, v = cons[1][2][0]
    assert wire > c.npub
    cons[1][2][0] = (wire, (v + 1) % R)
    write(cons)
    expect(circom.VerifyZkey(str(tmp_path / "x.r1cs"), paths["t.ptau"], paths["c.zkey"], seed=SEED), ["C"])
    # one A coefficient: the key's own rows differ, A differs, and IC or C -- whichever holds the signal
    for j in range(c.nc):
        cons = [tuple(list(lc) for lc in con) for con in c.constraints]
        wire, v = cons[j][0][0]
        cons[j][0][0] = (wire, (v + 1) % R)
        write(cons)
        rep = circom.VerifyZkey(str(tmp_path / "x.r1cs"), paths["t.ptau"], paths["c.zkey"], seed=SEED)
        expect(rep, ["coefs A", "A", "IC" if wire <= c.npub else "C"])
        assert rep.points["coefs A"][0] == 1


def test_files_that_do_not_fit_are_value_errors_that_name_the_section(tmp_path_factory, tmp_path):
    c, paths = built("k3", 0, tmp_path_factory)
    x = str(tmp_path / "x.r1cs")
    circom.WriteR1cs(x, c.nvars, 0, c.npub + 1, 0, c.constraints)
    with pytest.raises(ValueError, match=r"section 2 \(header\): nPublic = 1.*needs 2"):
        circom.VerifyZkey(x, paths["t.ptau"], paths["c.zkey"])
    circom.WriteR1cs(x, c.nvars, 0, c.npub, 1, c.constraints * 3)
    with pytest.raises(ValueError, match=r"section 2 \(header\): domainSize = 8.*needs 16"):
        circom.VerifyZkey(x, paths["t.ptau"], paths["c.zkey"])
    small = str(tmp_path / "small.ptau")
    circom.WritePtau(small, c.k - 1, c.tau, c.alpha, c.beta)
    with pytest.raises(ValueError, match=r"small.ptau: section 1 \(header\): power = 2"):
        circom.VerifyZkey(paths["c.r1cs"], small, paths["c.zkey"])


def _upload_all(paths):
    r1cs, ptau, z = circom.ReadR1cs(paths["c.r1cs"]), circom.ReadPtau(paths["t.ptau"]), circom.ReadZkey(paths["c.zkey"])
    k, m = z.domainBits, z.domainSize
    up1, up2 = capi.g1_upload_affine_mont, capi.g2_upload_affine_mont
    handles = [up1(z.A), up1(z.B1), up2(z.B2), up1(z.IC), up1(z.C), up1(z.H), circom.DeviceZkeyR1CS(k, z.nVars, z.coefs), circom._setup_system(r1cs, k),
               up1(ptau.tauG1[:min(2 * m, (2 << ptau.power) - 1) * 64]), up2(ptau.tauG2[:m * 128]), up1(ptau.alphaTauG1[:m * 64]), up1(ptau.betaTauG1[:m * 64])]
    return handles, z


def test_no_tables_and_no_memory_left_behind(tmp_path_factory):
    c, paths = built("k10", 1, tmp_path_factory)
    capi.trim()
    before = capi.memory_query()["library_bytes"]
    capi.set_table_policy("always")
    handles, z = _upload_all(paths)
    checks = capi.groth16_key_check(*handles, circom._g2(z.delta2), z.domainBits, z.nPublic, 12345)
    assert all(ok for _, ok, _, _ in checks)
    for h in handles:
        assert capi.handle_bytes(h)[1] == 0
    # an array that owned a table loses it to the check
    capi.build_tables(handles[0])
    assert capi.handle_bytes(handles[0])[1] > 0
    assert all(ok for _, ok, _, _ in capi.groth16_key_check(*handles, circom._g2(z.delta2), z.domainBits, z.nPublic, 54321))
    assert capi.handle_bytes(handles[0])[1] == 0
    for h in handles:
        (h.handle if hasattr(h, "handle") else h).free()
    capi.trim()
    assert capi.memory_query()["library_bytes"] == before


def test_handles_that_do_not_fit_and_a_zero_challenge(tmp_path_factory):
    c, paths = built("k3", 0, tmp_path_factory)
    handles, z = _upload_all(paths)
    args = (circom._g2(z.delta2), z.domainBits, z.nPublic)
    with pytest.raises(capi.GosnarkHipError, match="challenge is 0 mod r") as e:
        capi.groth16_key_check(*handles, *args, R)
    assert e.value.code == -3
    swapped = list(handles)
    swapped[3], swapped[4] = swapped[4], swapped[3]              # IC <-> C
    with pytest.raises(capi.GosnarkHipError, match="ic holds") as e:
        capi.groth16_key_check(*swapped, *args, 7)
    assert e.value.code == -4
    short = list(handles)
    short[8] = capi.g1_upload_affine_mont(circom.ReadPtau(paths["t.ptau"]).tauG1[:(2 * c.m - 2) * 64])
    with pytest.raises(capi.GosnarkHipError, match="tau_g1 holds 14 points") as e:
        capi.groth16_key_check(*short, *args, 7)
    assert e.value.code == -4
    with pytest.raises(capi.GosnarkHipError, match="bad handle") as e:
        capi.groth16_key_check(handles[2], *handles[1:], *args, 7)     # a G2 array in A's place
    assert e.value.code == -3
    with pytest.raises(capi.GosnarkHipError, match="product system") as e:
        capi.groth16_key_check(*handles[:6], handles[7], handles[7], *handles[8:], *args, 7)
    assert e.value.code == -4
