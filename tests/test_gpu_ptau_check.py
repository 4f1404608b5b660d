"""-m gpu: circom.VerifyPtau -- a powers-of-tau file checked against itself on the device (gs_ptau_check).

The transcripts are written from toxic values (circom.WritePtau), so the combination points have closed forms: with rho_i = s^(i+1),
sum_i rho_i tau^i times the generator (times alpha, beta), and tau times that on the shifted side.  Every tampering must fail exactly the
checks whose points it touches: tauG1[1] and tauG2[1] stand in several equations, so at power 1 -- where the last tauG2 point IS
tauG2[1] -- more checks are affected than at the larger powers."""
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom
import circom_util as CU
from oracle import c_oracle as C
from oracle import ref_py as O

pytestmark = pytest.mark.gpu
R = CU.R
TAU, ALPHA, BETA = 0x1234567890abcdef1234567890abcdef, 0xfedcba0987654321, 0x0f1e2d3c4b5a6978
SEED = 20261020
NAMES = list(capi.PTAU_CHECKS)
USES_TAU2_1 = ["tau", "tauG1", "alphaTauG1", "betaTauG1"]          # the equations tauG2[1] stands in


@pytest.fixture(autouse=True)
def _init():
    capi.init()


_FILES = {}


def transcript(power, tmp_path_factory, tau=TAU, alpha=ALPHA, beta=BETA):
    key = (power, tau, alpha, beta)
    if key not in _FILES:
        path = str(tmp_path_factory.mktemp("ptau_%d" % power) / "t.ptau")
        circom.WritePtau(path, power, tau, alpha, beta)
        _FILES[key] = path
    return _FILES[key]


def sections(path):
    return circom._read_sections(path, b"ptau", 1, circom._PTAU_NAMES, range(1, 7))


def patched(src, dst, edits):
    data = bytearray(open(src, "rb").read())
    for off, b in edits:
        data[off:off + len(b)] = b
    with open(dst, "wb") as f:
        f.write(bytes(data))
    return dst


def g1_affine(k):
    return tuple(C.g1_affine(C.g1_mul_scalar(O.G1_GEN, k % R)))


def g2_affine(k):
    p = C.g2_affine(C.g2_mul_scalar(O.G2_GEN, k % R))
    return (tuple(p[0]), tuple(p[1]))


def expect(rep, failed):
    assert [n for n, _, _, _ in rep.checks] == NAMES
    assert sorted(rep.failed) == sorted(failed), rep
    assert bool(rep) == (not failed)


@pytest.mark.parametrize("power", [1, 3, 10])
def test_a_transcript_is_accepted_with_the_closed_forms_of_every_check(power, tmp_path_factory):
    rep = circom.VerifyPtau(transcript(power, tmp_path_factory), seed=SEED + power)
    expect(rep, [])
    assert isinstance(rep, circom.PtauReport)
    n, s = 1 << power, rep.seed
    comb = lambda count: sum(pow(s, i + 1, R) * pow(TAU, i, R) for i in range(count)) % R      # noqa: E731
    long_, short = comb(2 * n - 2), comb(n - 1)
    want = {"g1": (g1_affine(1), g1_affine(1)), "g2": (g2_affine(1), g2_affine(1)), "tau": (g1_affine(TAU), g2_affine(TAU)),
            "tauG1": (g1_affine(long_), g1_affine(long_ * TAU)), "tauG2": (g2_affine(short), g2_affine(short * TAU)),
            "alphaTauG1": (g1_affine(ALPHA * short), g1_affine(ALPHA * short * TAU)),
            "betaTauG1": (g1_affine(BETA * short), g1_affine(BETA * short * TAU)), "betaG2": (g1_affine(BETA), g2_affine(BETA))}
    for name in NAMES:
        assert rep.points[name] == want[name], name


def test_a_prefix_of_a_transcript_is_checked_on_request(tmp_path_factory):
    path = transcript(3, tmp_path_factory)
    rep = circom.VerifyPtau(path, power=2, seed=SEED)
    expect(rep, [])
    comb = sum(pow(rep.seed, i + 1, R) * pow(TAU, i, R) for i in range(6)) % R
    assert rep.points["tauG1"] == (g1_affine(comb), g1_affine(comb * TAU))
    with pytest.raises(ValueError, match=r"section 1 \(header\): power = 3"):
        circom.VerifyPtau(path, power=4)
    a, b = circom.VerifyPtau(path), circom.VerifyPtau(path)
    assert a and b and a.seed != b.seed


@pytest.mark.parametrize("power", [1, 3, 10])
def test_a_tampered_transcript_fails_exactly_the_checks_it_touches(power, tmp_path_factory, tmp_path):
    good = transcript(power, tmp_path_factory)
    other = transcript(power, tmp_path_factory, tau=TAU + 1, alpha=ALPHA + 1, beta=BETA + 1)
    n = 1 << power
    data, sec = sections(good)
    odata, osec = sections(other)
    data, odata = bytes(data), bytes(odata)
    g1 = lambda sid, i, d=data, s=sec: d[s[sid][0] + 64 * i:s[sid][0] + 64 * (i + 1)]      # noqa: E731
    g2 = lambda sid, i, d=data, s=sec: d[s[sid][0] + 128 * i:s[sid][0] + 128 * (i + 1)]    # noqa: E731
    i = 1 if power == 1 else n - 1                                 # the middle of tauG1; at power 1 the pair holds tauG1[1]
    cases = {
        "a swapped pair in tauG1": ([(sec[2][0] + 64 * i, g1(2, i + 1)), (sec[2][0] + 64 * (i + 1), g1(2, i))], ["tau", "tauG1", "tauG2"] if i == 1 else ["tauG1"]),
        "the last tauG1 point": ([(sec[2][0] + 64 * (2 * n - 2), g1(2, 0))], ["tauG1"]),
        "the last tauG2 point": ([(sec[3][0] + 128 * (n - 1), g2(3, 0))], USES_TAU2_1 + ["tauG2"] if n == 2 else ["tauG2"]),
        "an alphaTauG1 point of another alpha": ([(sec[4][0] + 64 * (n - 1), g1(4, n - 1, odata, osec))], ["alphaTauG1"]),
        "another betaG2": ([(sec[6][0], g2(6, 0, odata, osec))], ["betaG2"]),
        "the tauG2 section of another tau": ([(sec[3][0], odata[osec[3][0]:osec[3][0] + osec[3][1]])], USES_TAU2_1 + ["tauG2"]),
    }
    for k, (what, (edits, failed)) in enumerate(cases.items()):
        rep = circom.VerifyPtau(patched(good, str(tmp_path / ("t%d.ptau" % k)), edits), seed=SEED)
        assert sorted(rep.failed) == sorted(failed), (what, rep)


def test_handles_that_do_not_fit_and_a_zero_challenge(tmp_path_factory):
    p = circom.ReadPtau(transcript(3, tmp_path_factory))
    up1, up2 = capi.g1_upload_affine_mont, capi.g2_upload_affine_mont
    t1, t2, ta, tb = up1(p.tauG1), up2(p.tauG2), up1(p.alphaTauG1), up1(p.betaTauG1)
    bg2 = circom._g2(circom.G2FromZkey(p.betaG2))
    assert all(ok for _, ok, _, _ in capi.ptau_check(t1, t2, ta, tb, bg2, 3, 5))
    for args, code, text in (((t1, t2, ta, tb, bg2, 3, 0), -3, "challenge is 0 mod r"), ((t1, t2, ta, tb, bg2, 4, 5), -4, "tau_g1 holds 15 points"),
                             ((t1, t2, ta, up1(p.betaTauG1[:7 * 64]), bg2, 3, 5), -4, "need N = 8"), ((t2, t2, ta, tb, bg2, 3, 5), -3, "bad handle"),
                             ((t1, t2, ta, tb, bg2, 0, 5), -3, "log2_n = 0")):
        with pytest.raises(capi.GosnarkHipError, match=text) as e:
            capi.ptau_check(*args)
        assert e.value.code == code
    for h in (t1, t2, ta, tb):
        assert capi.handle_bytes(h)[1] == 0
