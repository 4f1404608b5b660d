"""-m gpu: circom.PreparePtau / VerifyPtauPrepared / SetupFromPtau(prepared=True) -- the prepared sections 12 - 15 of a powers-of-tau
file on the device.

The transcripts are written from toxic values (circom.WritePtau), so every point of every level has a closed form: level p of a section
with the factor c is c L_j^(p)(tau) G, the Lagrange basis of the domain 2^p at tau (circom_util.lagrange_at), and the padded level
power + 1 of tauG1 is the O(n^2) inverse transform of its 2^(power+1) - 1 scalars and a zero.  Scalars in Python integers, points by
gs_g*_fixed_base; every comparison is bit for bit on affine points or on the bytes of a file."""
import random
import struct

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom
import c_util
import circom_util as CU
from setup_util import Circuit

pytestmark = pytest.mark.gpu
R = CU.R
G1B, G2B = circom.G1_BYTES, circom.G2_BYTES
PREPARED = (12, 13, 14, 15)
NAMES = {12: "tauG1 Lagrange", 13: "tauG2 Lagrange", 14: "alphaTauG1 Lagrange", 15: "betaTauG1 Lagrange"}
SHAPES = {"k1": (1, 0, 1), "k3_full": (3, 3, 4), "k3": (3, 1, 3)}      # name -> (k, nPublic, nConstraints), as test_gpu_setup_ptau.py
EXTRA = [(7, b"a contribution record that is copied as found"), (12, b"\x01" * (3 * G1B)), (99, b"unknown")]


@pytest.fixture(autouse=True)
def _init():
    capi.init()
    capi.set_table_policy("auto")
    capi.set_eval_basis(True)
    yield
    capi.set_table_policy("auto")


def toxic(seed):
    rng = random.Random(seed)
    return tuple(rng.randrange(2, R) for _ in range(3))


_FILES = {}


def files(power, tmp_path_factory, seed=0):
    """-> (plain path, prepared path, (tau, alpha, beta)); the plain file carries section 7, a stale section 12 and an unknown section"""
    key = (power, seed)
    if key not in _FILES:
        d = tmp_path_factory.mktemp("prepare_%d_%d" % key)
        src, dst = str(d / "t.ptau"), str(d / "prepared.ptau")
        tox = toxic(900 + 10 * power + seed)
        circom.WritePtau(src, power, *tox, extra_sections=EXTRA)
        timing = {}
        circom.PreparePtau(src, dst, timing=timing)
        assert timing["power"] == power and timing["calls"] == 4 and timing["device_ms"] > 0 and timing["wall_ms"] > 0
        assert {"parse_ms", "upload_ms", "download_ms", "write_ms", "library_bytes_max"} <= set(timing)
        _FILES[key] = (src, dst, tox)
    return _FILES[key]


def sections(path):
    data = open(path, "rb").read()
    assert data[:4] == b"ptau" and struct.unpack("<I", data[4:8])[0] == 1
    nsec, pos, out = struct.unpack("<I", data[8:12])[0], 12, []
    for _ in range(nsec):
        sid, length = struct.unpack("<IQ", data[pos:pos + 12])
        out.append((sid, data[pos + 12:pos + 12 + length]))
        pos += 12 + length
    assert pos == len(data)
    return out


def write_sections(path, secs):
    with open(path, "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, len(secs)))
        for sid, payload in secs:
            f.write(struct.pack("<IQ", sid, len(payload)) + payload)


def section_rows(buf, g2=False):
    return capi.g2_download(capi.g2_upload_affine_mont(buf)) if g2 else capi.g1_download(capi.g1_upload_affine_mont(buf))


def fixed_rows(scalars, g2=False):
    f = capi.g2_fixed_base if g2 else capi.g1_fixed_base
    return (capi.g2_download if g2 else capi.g1_download)(f(CU.u64(scalars)))


def padded_level(tau, power):
    """the inverse transform of size 2^(power+1) of tau^0 .. tau^(2^(power+1) - 2) and one zero, by definition"""
    k, n = power + 1, 2 << power
    s, t = [], 1
    for _ in range(n - 1):
        s.append(t)
        t = t * tau % R
    s.append(0)
    wi = pow(CU.omega(k), -1, R)
    pw = [pow(wi, e, R) for e in range(n)]
    ninv = pow(n, -1, R)
    return [sum(s[i] * pw[i * j % n] for i in range(n)) * ninv % R for j in range(n)]


def expected_levels(sid, power, tox):
    tau, alpha, beta = tox
    c = {12: 1, 13: 1, 14: alpha, 15: beta}[sid]
    out = []
    for p in range(power + 1):
        out += [c * v % R for v in CU.lagrange_at(p, tau)]
    if sid == 12:
        out += padded_level(tau, power)
    return out


@pytest.mark.parametrize("power", [0, 1, 3, 5])
def test_prepare_ptau_levels_have_their_closed_forms_and_the_rest_is_copied(power, tmp_path_factory):
    src, dst, tox = files(power, tmp_path_factory)
    before, after = sections(src), sections(dst)
    kept = [s for s in before if s[0] not in PREPARED]
    assert [sid for sid, _ in before] == [1, 2, 3, 4, 5, 6, 7, 12, 99]
    assert [sid for sid, _ in after] == [1, 2, 3, 4, 5, 6, 7, 99, 12, 13, 14, 15]
    assert after[:len(kept)] == kept                                   # sections 1 - 7 and the unknown one byte for byte
    p = circom.ReadPtauPrepared(dst)                                   # the stale section 12 is gone: the lengths are the layout's
    n = 1 << power
    assert [p.lagrange[sid].size for sid in PREPARED] == [(4 * n - 1) * G1B, (2 * n - 1) * G2B, (2 * n - 1) * G1B, (2 * n - 1) * G1B]
    for sid in PREPARED:
        g2 = sid == 13
        assert np.array_equal(section_rows(p.lagrange[sid], g2), fixed_rows(expected_levels(sid, power, tox), g2)), NAMES[sid]
    # the padded level is not the full one: a transcript one power longer has the full level power + 1
    if power == 3:
        tau = tox[0]
        got = section_rows(p.level(12, power + 1))
        assert not np.array_equal(got, fixed_rows(CU.lagrange_at(power + 1, tau)))
        assert np.array_equal(got, fixed_rows(padded_level(tau, power)))


@pytest.mark.parametrize("power", [1, 3])
def test_prepare_ptau_batch_seam_gives_identical_files(power, tmp_path_factory, tmp_path):
    """batch_log2 = 0: level 0 batched, every other level a single call (the padded one through an appended infinity); 2: the seam in the
    middle; 27: everything batched, as the default"""
    src, dst, _ = files(power, tmp_path_factory)
    want = open(dst, "rb").read()
    for batch, calls in ((0, 4 + 4 * power + 1), (2, 4 + 4 * max(power - 2, 0) + (1 if power >= 2 else 0)), (27, 4)):
        out, timing = str(tmp_path / ("b%d.ptau" % batch)), {}
        circom.PreparePtau(src, out, batch_log2=batch, timing=timing)
        assert open(out, "rb").read() == want, batch
        assert timing["calls"] == calls
    # preparing a prepared file drops its sections 12 - 15 and gives the same file again
    again = str(tmp_path / "again.ptau")
    circom.PreparePtau(dst, again)
    assert open(again, "rb").read() == want


@pytest.mark.parametrize("extra_power", [0, 1])
@pytest.mark.parametrize("name", list(SHAPES))
def test_setup_from_prepared_sections_writes_the_same_zkey(name, extra_power, tmp_path):
    """transcript power k: H comes from the padded level k + 1; power k + 1: from the full one -- SetupFromPtau's two H rules"""
    k, npub, nc = SHAPES[name]
    c = Circuit(k, npub, nc, 1000 + 10 * k + npub)
    paths = {n: str(tmp_path / n) for n in ("c.r1cs", "t.ptau", "p.ptau", "a.zkey", "b.zkey")}
    c.write_r1cs(paths["c.r1cs"])
    circom.WritePtau(paths["t.ptau"], k + extra_power, c.tau, c.alpha, c.beta)
    circom.PreparePtau(paths["t.ptau"], paths["p.ptau"])
    ta, tb = {}, {}
    circom.SetupFromPtau(paths["c.r1cs"], paths["t.ptau"], paths["a.zkey"], timing=ta)
    key, prod, vk = circom.SetupFromPtau(paths["c.r1cs"], paths["p.ptau"], paths["b.zkey"], timing=tb, prepared=True)
    assert open(paths["a.zkey"], "rb").read() == open(paths["b.zkey"], "rb").read()
    assert ta["transforms_ms"] > 0 and tb["transforms_ms"] == 0 and tb["colsums_ms"] > 0
    assert circom.VerifyZkey(paths["c.r1cs"], paths["p.ptau"], paths["b.zkey"], seed=3)
    # the default path over the prepared file does not read its sections 12 - 15 either way
    circom.SetupFromPtau(paths["c.r1cs"], paths["p.ptau"], paths["a.zkey"])
    assert open(paths["a.zkey"], "rb").read() == open(paths["b.zkey"], "rb").read()
    # the objects it returns prove
    proof = circom.GenerateProofsWithRS(key, prod, c.w, 5, 6)
    CU.assert_closed_form(proof, c.proof_scalars(c.w, 5, 6))
    with pytest.raises(ValueError, match=r"section 12 \(tauG1 Lagrange\) is missing"):
        circom.SetupFromPtau(paths["c.r1cs"], paths["t.ptau"], paths["b.zkey"], prepared=True)


@pytest.mark.parametrize("power", [0, 3, 5])
def test_verify_ptau_prepared_accepts(power, tmp_path_factory):
    _, dst, _ = files(power, tmp_path_factory)
    timing = {}
    rep = circom.VerifyPtauPrepared(dst, seed=40 + power, timing=timing)
    assert rep and [name for name, _, _, _ in rep.checks] == list(NAMES.values()) and not rep.failed
    assert all(lhs == rhs for lhs, rhs in rep.points.values())
    assert timing["power"] == power and timing["device_ms"] > 0 and timing["wall_ms"] > 0
    assert circom.VerifyPtauPrepared(dst)                              # a challenge from the system's randomness


def altered(path, out, sid, index, donor):
    """the file with point `index` of section sid replaced by the section's point `donor`"""
    secs = sections(path)
    size = G2B if sid == 13 else G1B
    for i, (s, body) in enumerate(secs):
        if s == sid:
            body = bytearray(body)
            new = bytes(body[donor * size:(donor + 1) * size])
            assert new != bytes(body[index * size:(index + 1) * size])
            body[index * size:(index + 1) * size] = new
            secs[i] = (s, bytes(body))
    write_sections(out, secs)


@pytest.mark.parametrize("where", ["first", "last of the top level", "middle level"])
def test_verify_ptau_prepared_names_the_section_of_one_altered_point(where, tmp_path_factory, tmp_path):
    power = 3
    _, dst, _ = files(power, tmp_path_factory)
    out = str(tmp_path / "bad.ptau")
    for sid in PREPARED:
        count = (4 << power) - 1 if sid == 12 else (2 << power) - 1
        index, donor = {"first": (0, 1), "last of the top level": (count - 1, 0), "middle level": (4, 5)}[where]      # 4: level 2, point 1
        altered(dst, out, sid, index, donor)
        rep = circom.VerifyPtauPrepared(out, seed=50 + sid)
        assert not rep and rep.failed == [NAMES[sid]]
        lhs, rhs = rep.points[NAMES[sid]]
        assert lhs != rhs


def test_verify_ptau_prepared_refuses_the_sections_of_another_tau(tmp_path_factory, tmp_path):
    _, mine, tox = files(3, tmp_path_factory)
    other = (pow(tox[0], 2, R), tox[1], tox[2])
    a, b, out = str(tmp_path / "o.ptau"), str(tmp_path / "op.ptau"), str(tmp_path / "spliced.ptau")
    circom.WritePtau(a, 3, *other)
    circom.PreparePtau(a, b)
    theirs = dict(sections(b))
    write_sections(out, [(sid, theirs[sid] if sid in PREPARED else body) for sid, body in sections(mine)])
    rep = circom.VerifyPtauPrepared(out, seed=60)
    assert rep.failed == list(NAMES.values())
    assert circom.VerifyPtauPrepared(b, seed=60)


def test_verify_ptau_prepared_power_checks_a_prefix(tmp_path_factory, tmp_path):
    """the last point of every section's top level is wrong: the file's own power sees it, a smaller one does not -- and for tauG1 the
    smaller power's top level is the FULL level power + 1, not a padded one"""
    power = 3
    _, dst, _ = files(power, tmp_path_factory)
    out = str(tmp_path / "bad.ptau")
    secs = sections(dst)
    for i, (sid, body) in enumerate(secs):
        if sid in PREPARED:
            size = G2B if sid == 13 else G1B
            secs[i] = (sid, body[:-size] + body[:size])
    write_sections(out, secs)
    assert circom.VerifyPtauPrepared(out, seed=70).failed == list(NAMES.values())
    for p in (0, 1, 2):
        timing = {}
        assert circom.VerifyPtauPrepared(out, power=p, seed=70, timing=timing) and timing["power"] == p
    with pytest.raises(ValueError, match=r"the levels 0 \.\. 4 cannot be checked \(0 <= power <= 3"):
        circom.VerifyPtauPrepared(out, power=4)


def test_ptau_prepare_c_sequence_gives_the_python_routes_sections(tmp_path_factory, tmp_path):
    """tests/c/ptau_prepare.c, the call sequence of go/gosnarkhip/ptau.go (PreparePtauArrays + the four checks) from a process without
    Python"""
    src, dst, _ = files(3, tmp_path_factory)
    out = str(tmp_path / "sections.bin")
    stdout = c_util.build_and_run("ptau_prepare.c", [src, out], tmp_path)
    assert stdout.startswith("OK power 3"), stdout
    mine = dict(sections(dst))
    assert open(out, "rb").read() == b"".join(mine[sid] for sid in PREPARED)
