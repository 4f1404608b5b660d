"""-m gpu: membership=True on circom.VerifyPtau, VerifyPtauPrepared and VerifyZkey -- the G2 arrays the verifiers upload are tested for the
order-r subgroup point by point (gs_g2_subgroup_check).

Transcripts at power 3 and 7 (128 tauG2 points: the 64-thread workgroup seam lies inside the section), prepared on the device; the key
of the small circuit of test_gpu_zkey_check.py over the power-3 transcript.  A tampered file has ONE G2 point replaced by point + S,
ord(S) = 10069: still on the twist, so every upload accepts it, and the random linear combination of its section lets it through once in
about 10069 challenges -- what those checks say about such a file is therefore not asserted here; the membership check must name it."""
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom
import membership_util as M
from setup_util import Circuit

pytestmark = pytest.mark.gpu
SEED = 20261021
APPENDED = {"ptau": ["tauG2 membership"], "prepared": ["tauG2 Lagrange membership"], "zkey": ["tauG2 membership", "B2 membership"]}


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    yield
    capi.set_table_policy("auto")


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The circuit, and name -> path: t3 / t7 (prepared transcripts of power 3 and 7), c.r1cs, c.zkey (over t3)"""
    capi.init()
    k, npub, nc = 3, 1, 3
    c = Circuit(k, npub, nc, 1000 + 10 * k + npub)
    d = tmp_path_factory.mktemp("membership")
    p = {n: str(d / n) for n in ("raw3.ptau", "raw7.ptau", "t3", "t7", "c.r1cs", "c.zkey")}
    c.write_r1cs(p["c.r1cs"])
    for power in (3, 7):
        circom.WritePtau(p["raw%d.ptau" % power], power, c.tau, c.alpha, c.beta)
        circom.PreparePtau(p["raw%d.ptau" % power], p["t%d" % power])
    circom.SetupFromPtau(p["c.r1cs"], p["t3"], p["c.zkey"])
    return c, p


def names(rep):
    return [c[0] for c in rep.checks]


def plus_s(src, dst, offset):
    """A copy of the file whose G2 point at byte `offset` is replaced by point + S."""
    data = bytearray(open(src, "rb").read())
    moved = M.complete_add(circom._g2(circom.G2FromZkey(data[offset:offset + 128])), M.small_order_point())
    assert not M.in_subgroup(moved)
    data[offset:offset + 128] = circom.G2ToZkey(moved)
    with open(dst, "wb") as f:
        f.write(bytes(data))
    return dst


def ptau_sections(path):
    return circom._read_sections(path, b"ptau", 1, circom._PTAU_PREPARED_NAMES, (3, 13))[1]


def only_failed_membership(rep, name, index):
    member = {c[0]: c for c in rep.checks if c[0].endswith("membership")}
    assert member[name] == (name, False, 1, index), rep
    assert all(ok for n, ok, _, _ in member.values() if n != name), rep
    assert name in rep.failed and not rep


@pytest.mark.parametrize("power", [3, 7])
def test_untouched_transcripts_pass_and_the_default_reports_are_unchanged(files, power):
    path = files[1]["t%d" % power]
    timing = {}
    rep = circom.VerifyPtau(path, seed=SEED, membership=True, timing=timing)
    assert rep and names(rep) == list(capi.PTAU_CHECKS) + APPENDED["ptau"]
    assert rep.checks[-1] == ("tauG2 membership", True, 0, None) and timing["membership_ms"] > 0.0
    assert names(circom.VerifyPtau(path, seed=SEED)) == list(capi.PTAU_CHECKS)
    timing = {}
    rep = circom.VerifyPtauPrepared(path, seed=SEED, membership=True, timing=timing)
    assert rep and names(rep) == list(circom.PTAU_PREPARED_CHECKS) + APPENDED["prepared"]
    assert rep.checks[-1] == ("tauG2 Lagrange membership", True, 0, None) and timing["membership_ms"] > 0.0
    timing = {}
    assert names(circom.VerifyPtauPrepared(path, seed=SEED, timing=timing)) == list(circom.PTAU_PREPARED_CHECKS)
    assert "membership_ms" not in timing


def test_an_untouched_key_passes_and_the_default_report_is_unchanged(files):
    _, p = files
    timing = {}
    rep = circom.VerifyZkey(p["c.r1cs"], p["t3"], p["c.zkey"], seed=SEED, membership=True, timing=timing)
    assert rep and names(rep) == ["header", "delta"] + list(capi.KEY_CHECKS) + APPENDED["zkey"]
    assert rep.checks[-2:] == [("tauG2 membership", True, 0, None), ("B2 membership", True, 0, None)] and timing["membership_ms"] > 0.0
    timing = {}
    rep = circom.VerifyZkey(p["c.r1cs"], p["t3"], p["c.zkey"], seed=SEED, timing=timing)
    assert rep and names(rep) == ["header", "delta"] + list(capi.KEY_CHECKS) and "membership_ms" not in timing


@pytest.mark.parametrize("power", [3, 7])
def test_a_tau_g2_point_off_the_subgroup_is_named(files, power, tmp_path):
    c, p = files
    src = p["t%d" % power]
    sec = ptau_sections(src)
    for index in (1, (1 << power) - 1):
        bad = plus_s(src, str(tmp_path / ("bad%d.ptau" % index)), sec[3][0] + 128 * index)
        only_failed_membership(circom.VerifyPtau(bad, seed=SEED, membership=True), "tauG2 membership", index)
        # the prepared sections of that file are untouched
        rep = circom.VerifyPtauPrepared(bad, seed=SEED, membership=True)
        assert rep.checks[-1] == ("tauG2 Lagrange membership", True, 0, None)
        if power == 3:                                       # the key check reads the same eight points
            only_failed_membership(circom.VerifyZkey(p["c.r1cs"], bad, p["c.zkey"], seed=SEED, membership=True), "tauG2 membership", index)


@pytest.mark.parametrize("power", [3, 7])
def test_a_level_point_off_the_subgroup_is_named(files, power, tmp_path):
    src = files[1]["t%d" % power]
    sec = ptau_sections(src)
    index = (1 << power) - 1 + 2                             # point 2 of the top level: behind the seam at power 7
    bad = plus_s(src, str(tmp_path / "bad.ptau"), sec[13][0] + 128 * index)
    only_failed_membership(circom.VerifyPtauPrepared(bad, seed=SEED, membership=True), "tauG2 Lagrange membership", index)
    assert circom.VerifyPtau(bad, seed=SEED, membership=True)          # sections 2 - 5 are untouched


def test_a_b2_point_off_the_subgroup_is_named(files, tmp_path):
    c, p = files
    sec = circom._read_sections(p["c.zkey"], b"zkey", 1, circom._ZKEY_NAMES, (7,))[1]
    assert sec[7][1] == c.nvars * 128
    for index in (0, c.nvars - 1):
        bad = plus_s(p["c.zkey"], str(tmp_path / ("bad%d.zkey" % index)), sec[7][0] + 128 * index)
        only_failed_membership(circom.VerifyZkey(p["c.r1cs"], p["t3"], bad, seed=SEED, membership=True), "B2 membership", index)
