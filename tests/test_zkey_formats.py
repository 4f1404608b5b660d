"""circuit.zkey / witness.wtns as go-snark-study_amd/circom.py reads and writes them (host code, no GPU): round trips field by field, the committed
fixture against the JSON fixture it was converted from, every malformation a ValueError that names its section."""
import os
import random
import struct

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import capi, circom, groth16
import circom_util as CU
from oracle import c_oracle as C
from oracle import ref_py as O

R = CU.R
ZFIX = os.path.join(CU.HERE, "golden", "zkey_multiplier")


def g1(ks):
    out = []
    for k in ks:
        a = C.g1_affine(C.g1_mul_scalar(O.G1_GEN, k % R)) if k % R else None
        out.append(circom.G1_INF if a is None else (a[0], a[1], 1))
    return out


def g2(ks):
    out = []
    for k in ks:
        a = C.g2_affine(C.g2_mul_scalar(O.G2_GEN, k % R)) if k % R else None
        out.append(circom.G2_INF if a is None else (a[0], a[1], (1, 0)))
    return out


def multiplier():
    pkj = circom.ParseProvingKey(CU.fixture_json("proving_key"))
    vk = circom.ParseVerificationKey(CU.fixture_json("verification_key"))
    w = circom.ParseWitness(CU.fixture_json("witness"))
    return pkj, vk, w


def synthetic(k=3, seed=5):
    """A ProvingKey, its Vk and E from an Instance's toxic values (points by the oracle)."""
    inst = CU.Instance(k, (1 << k) - 1, seed)
    ginv = pow(inst.gamma, -1, R)
    ic = [(inst.beta * inst.at[i] + inst.alpha * inst.bt[i] + inst.ct[i]) * ginv % R for i in range(inst.npublic + 1)]
    one = lambda f, x: f([x])[0]                                          # noqa: E731
    pkj = circom.ProvingKey(inst.nvars, inst.npublic, k, inst.rows_a, inst.rows_b, inst.rows_c, g1(inst.at), g1(inst.bt), g2(inst.bt), g1(inst.cd),
                            g1(inst.hexps), one(g1, inst.alpha), one(g1, inst.beta), one(g1, inst.delta), one(g2, inst.beta), one(g2, inst.delta))
    vk = groth16.Vk(IC=g1(ic), G1_Alpha=pkj.alfa1, G2_Beta=pkj.beta2, G2_Gamma=one(g2, inst.gamma), G2_Delta=pkj.delta2)
    return pkj, vk, g1(inst.eval_basis_scalars()), inst


def padded(rows, m):
    return [dict(r) for r in rows] + [dict() for _ in range(m - len(rows))]


def assert_same_key(z, pkj, vk, e):
    assert (z.nVars, z.nPublic, z.domainSize, z.domainBits) == (pkj.nVars, pkj.nPublic, pkj.domainSize, pkj.domainBits)
    assert z.g1("A") == pkj.A and z.g1("B1") == pkj.B1 and z.g2("B2") == pkj.B2 and z.c_full() == pkj.C
    assert (z.alfa1, z.beta1, z.delta1, z.beta2, z.delta2) == (pkj.alfa1, pkj.beta1, pkj.delta1, pkj.beta2, pkj.delta2)
    assert z.gamma2 == vk.G2_Gamma and z.g1("IC") == vk.IC
    if e is not None:
        assert z.g1("H") == e
    ra, rb = z.rows()
    assert ra == padded(pkj.rows_a, pkj.domainSize) and rb == padded(pkj.rows_b, pkj.domainSize)
    v = circom.VerificationKeyFromZkey(z)
    assert (v.IC, v.G1_Alpha, v.G2_Beta, v.G2_Gamma, v.G2_Delta) == (vk.IC, vk.G1_Alpha, vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta)


@pytest.fixture(scope="module")
def synth():
    return synthetic()


def test_write_then_read_round_trips_field_by_field(tmp_path, synth):
    pkj, vk, _ = multiplier()
    fix = circom.ReadZkey(os.path.join(ZFIX, "circuit.zkey"))
    for name, (key, kvk, e) in {"multiplier": (pkj, vk, fix.g1("H")), "synthetic": synth[:3]}.items():
        path = str(tmp_path / (name + ".zkey"))
        circom.WriteZkey(path, key, kvk, e)
        z = circom.ReadZkey(path)
        assert_same_key(z, key, kvk, e)
        assert not z.A.flags.writeable and z.nCoefs == sum(len(r) for r in key.rows_a) + sum(len(r) for r in key.rows_b)
    inst = synth[3]
    for w in (inst.w, [0, 1, R - 1, 5]):
        path = str(tmp_path / "w.wtns")
        circom.WriteWtns(path, w)
        got = circom.ReadWtns(path)
        assert got.shape == (len(w), 4) and not got.flags.writeable
        assert capi.u64_to_ints(np.array(got)) == [x % R for x in w]
    raw = np.array([[2 ** 64 - 1] * 4, [1, 2, 3, 4]], dtype=np.uint64)        # any 256-bit word passes through as it is
    circom.WriteWtns(str(tmp_path / "raw.wtns"), raw)
    assert np.array_equal(np.array(circom.ReadWtns(str(tmp_path / "raw.wtns"))), raw)


def test_committed_fixture_is_the_json_fixture():
    pkj, vk, w = multiplier()
    z = circom.ReadZkey(os.path.join(ZFIX, "circuit.zkey"))
    assert_same_key(z, pkj, vk, None)
    assert len(z.g1("H")) == pkj.domainSize
    assert capi.u64_to_ints(np.array(circom.ReadWtns(os.path.join(ZFIX, "witness.wtns")))) == w
    # the fixture system is a product system on its witness: c = a o b at every point of the domain
    m = pkj.domainSize
    a, b, c = (CU.mat_vec(padded(rows, m), w) for rows in (pkj.rows_a, pkj.rows_b, pkj.rows_c))
    assert [x * y % R for x, y in zip(a, b)] == c


def test_repeated_and_shuffled_records_add_up(tmp_path, synth):
    pkj, vk, e, _ = synth
    rec = circom.CoefRecords(pkj.rows_a, pkj.rows_b)
    mat, row, sig = struct.unpack("<III", rec[0][:12])
    v = int.from_bytes(rec[0][12:], "little") * pow(pow(2, 512, R), -1, R) % R
    split = [struct.pack("<III", mat, row, sig) + (x * pow(2, 512, R) % R).to_bytes(32, "little") for x in (5, (v - 5) % R)]
    rec = split + rec[1:]
    random.Random(3).shuffle(rec)
    path = str(tmp_path / "shuffled.zkey")
    circom.WriteZkey(path, pkj, vk, e, records=rec)
    assert_same_key(circom.ReadZkey(path), pkj, vk, e)


def test_unknown_section_is_skipped_and_order_is_free(tmp_path, synth):
    pkj, vk, e, _ = synth
    path = str(tmp_path / "odd.zkey")
    circom.WriteZkey(path, pkj, vk, e, order=list(range(9, 0, -1)), extra_sections=[(77, b"not a section this reader knows"), (10, b"")])
    assert_same_key(circom.ReadZkey(path), pkj, vk, e)


# ---- malformed files -------------------------------------------------------------------------------------------------------------
def sections_of(path):
    data = open(path, "rb").read()
    nsec = struct.unpack("<I", data[8:12])[0]
    out, pos = [], 12
    for _ in range(nsec):
        sid, length = struct.unpack("<IQ", data[pos:pos + 12])
        out.append((sid, data[pos + 12:pos + 12 + length]))
        pos += 12 + length
    return data[:4], struct.unpack("<I", data[4:8])[0], out


def write_sections(path, magic, version, secs, cut=0):
    blob = magic + struct.pack("<II", version, len(secs)) + b"".join(struct.pack("<IQ", sid, len(p)) + p for sid, p in secs)
    with open(path, "wb") as f:
        f.write(blob[:len(blob) - cut])
    return path


def patched(secs, sid, fn):
    return [(i, fn(p) if i == sid else p) for i, p in secs]


FOREIGN = 2 ** 255 - 19
HEAD_Q, HEAD_R = 4, 36                     # offsets of q and of n8r inside section 2


def zkey_cases():
    u32 = lambda v: struct.pack("<I", v)                                   # noqa: E731
    return {
        "wrong magic": (lambda m, v, s: (b"zkex", v, s), "not a .zkey"),
        "wrong version": (lambda m, v, s: (m, 2, s), "version"),
        "protocol 2": (lambda m, v, s: (m, v, patched(s, 1, lambda p: u32(2))), "section 1 (protocol)"),
        "n8q = 48": (lambda m, v, s: (m, v, patched(s, 2, lambda p: u32(48) + p[4:])), "section 2 (header)"),
        "foreign prime": (lambda m, v, s: (m, v, patched(s, 2, lambda p: p[:HEAD_R + 4] + FOREIGN.to_bytes(32, "little") + p[HEAD_R + 36:])),
                          "section 2 (header)"),
        "foreign base prime": (lambda m, v, s: (m, v, patched(s, 2, lambda p: p[:HEAD_Q] + FOREIGN.to_bytes(32, "little") + p[HEAD_Q + 32:])),
                               "section 2 (header)"),
        "domainSize = 6": (lambda m, v, s: (m, v, patched(s, 2, lambda p: p[:80] + u32(6) + p[84:])), "section 2 (header)"),
        "duplicate section": (lambda m, v, s: (m, v, s + [s[4]]), "section 5 (A) appears twice"),
        "missing section 9": (lambda m, v, s: (m, v, [x for x in s if x[0] != 9]), "section 9 (H) is missing"),
        "section 5 one point short": (lambda m, v, s: (m, v, patched(s, 5, lambda p: p[:-64])), "section 5 (A)"),
        "coefficient count too large": (lambda m, v, s: (m, v, patched(s, 4, lambda p: u32(struct.unpack("<I", p[:4])[0] + 1) + p[4:])),
                                        "section 4 (coefficients)"),
    }


@pytest.mark.parametrize("case", sorted(zkey_cases()))
def test_malformed_zkey_is_a_value_error_that_names_the_section(tmp_path, synth, case):
    pkj, vk, e, _ = synth
    good = str(tmp_path / "good.zkey")
    circom.WriteZkey(good, pkj, vk, e)
    magic, version, secs = sections_of(good)
    assert [s[0] for s in secs] == list(range(1, 10))
    mutate, text = zkey_cases()[case]
    bad = write_sections(str(tmp_path / "bad.zkey"), *mutate(magic, version, secs))
    with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)")):
        circom.ReadZkey(bad)


def test_truncated_files_are_value_errors(tmp_path, synth):
    pkj, vk, e, inst = synth
    good = str(tmp_path / "good.zkey")
    circom.WriteZkey(good, pkj, vk, e)
    magic, version, secs = sections_of(good)
    with pytest.raises(ValueError, match=r"section 9 \(H\).*runs past the end"):
        circom.ReadZkey(write_sections(str(tmp_path / "cut.zkey"), magic, version, secs, cut=10))
    wgood = str(tmp_path / "good.wtns")
    circom.WriteWtns(wgood, inst.w)
    wm, wv, ws = sections_of(wgood)
    with pytest.raises(ValueError, match=r"section 2 \(witness\).*runs past the end"):
        circom.ReadWtns(write_sections(str(tmp_path / "cut.wtns"), wm, wv, ws, cut=1))


def wtns_cases():
    u32 = lambda v: struct.pack("<I", v)                                   # noqa: E731
    return {
        "wrong magic": (lambda m, v, s: (b"wtnz", v, s), "not a .wtns"),
        "wrong version": (lambda m, v, s: (m, 1, s), "version"),
        "n8 = 48": (lambda m, v, s: (m, v, patched(s, 1, lambda p: u32(48) + p[4:])), "section 1 (header)"),
        "foreign prime": (lambda m, v, s: (m, v, patched(s, 1, lambda p: p[:4] + FOREIGN.to_bytes(32, "little") + p[36:])), "section 1 (header)"),
        "one value short": (lambda m, v, s: (m, v, patched(s, 2, lambda p: p[:-32])), "section 2 (witness)"),
        "duplicate section": (lambda m, v, s: (m, v, s + [s[1]]), "section 2 (witness) appears twice"),
        "missing section 2": (lambda m, v, s: (m, v, s[:1]), "section 2 (witness) is missing"),
    }


@pytest.mark.parametrize("case", sorted(wtns_cases()))
def test_malformed_wtns_is_a_value_error_that_names_the_section(tmp_path, synth, case):
    good = str(tmp_path / "good.wtns")
    circom.WriteWtns(good, synth[3].w)
    mutate, text = wtns_cases()[case]
    bad = write_sections(str(tmp_path / "bad.wtns"), *mutate(*sections_of(good)))
    with pytest.raises(ValueError, match=text.replace("(", r"\(").replace(")", r"\)")):
        circom.ReadWtns(bad)
