"""circuit.r1cs and powers-of-tau files on the host (circom.ReadR1cs / WriteR1cs / ReadPtau): round trips, counts, and every
malformation a ValueError that names its section.  No device: the .ptau files here are packed by hand with all-zero points."""
import struct

import numpy as np
import pytest

import gosnark_amd  # noqa: F401
from gosnark_amd import circom

R, Q = circom.R, circom.Q


def _container(magic, sections, version=1):
    out = magic + struct.pack("<II", version, len(sections))
    for sid, payload in sections:
        out += struct.pack("<IQ", sid, len(payload)) + payload
    return out


def _ptau_sections(power, prime=Q, ceremony=None):
    n = 1 << power
    head = struct.pack("<I", 32) + prime.to_bytes(32, "little") + struct.pack("<II", power, power if ceremony is None else ceremony)
    return {1: head, 2: bytes((2 * n - 1) * 64), 3: bytes(n * 128), 4: bytes(n * 64), 5: bytes(n * 64), 6: bytes(128), 7: b"\x01\x02\x03",
            12: bytes(n * 64)}


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


CONSTRAINTS = [
    ([(1, 1), (2, R - 1)], [(0, 5)], [(3, 2)]),
    ([], [], []),                                                  # an empty constraint
    ([(1, 3), (1, 4), (1, R - 7)], [], [(2, 0), (0, R), (3, R + 1), (3, (1 << 256) - 1)]),      # repeated wires, an empty combination, 0 and >= r
    ([(4, 1)], [(4, R - 1)], [(0, 1)]),
]


def _r1cs_path(tmp_path, constraints=CONSTRAINTS, extra=()):
    p = str(tmp_path / "c.r1cs")
    circom.WriteR1cs(p, 5, 1, 1, 2, constraints, extra_sections=extra)
    return p


def _terms(csr):
    rp, col, val = csr
    return [[(int(col[e]), int.from_bytes(val[e].astype("<u8").tobytes(), "little")) for e in range(rp[j], rp[j + 1])] for j in range(len(rp) - 1)]


def test_r1cs_round_trip(tmp_path):
    r = circom.ReadR1cs(_r1cs_path(tmp_path))
    assert (r.nWires, r.nVars, r.nPubOut, r.nPubIn, r.nPrvIn, r.nPublic, r.nConstraints, r.nLabels) == (5, 5, 1, 1, 2, 2, 4, 5)
    for k, m in enumerate((r.a, r.b, r.c)):
        assert m[0].dtype == np.uint32 and m[1].dtype == np.uint32 and m[2].dtype == np.uint64 and m[2].shape == (m[1].size, 4)
        assert _terms(m) == [[(w, v) for w, v in c[k]] for c in CONSTRAINTS]


def test_r1cs_without_constraints(tmp_path):
    r = circom.ReadR1cs(_r1cs_path(tmp_path, []))
    assert r.nConstraints == 0 and all(m[0].tolist() == [0] and m[1].size == 0 and m[2].shape == (0, 4) for m in (r.a, r.b, r.c))


def test_setup_records_order_and_values(tmp_path):
    """Section 4 of the key: A's terms before B's per constraint, in file order, then the nPublic + 1 public rows; values * 2^512 mod r."""
    r = circom.ReadR1cs(_r1cs_path(tmp_path))
    rec = circom._setup_records(r)
    got = [(int(x["matrix"]), int(x["row"]), int(x["signal"]), int.from_bytes(x["value"].tobytes(), "little")) for x in rec]
    want = []
    for j, (a, b, _) in enumerate(CONSTRAINTS):
        want += [(0, j, w, v * pow(2, 512, R) % R) for w, v in a] + [(1, j, w, v * pow(2, 512, R) % R) for w, v in b]
    want += [(0, 4 + s, s, pow(2, 512, R)) for s in range(3)]
    assert got == want and rec.dtype.itemsize == 44
    assert circom._setup_domain_bits(r) == 3                        # 4 + 2 + 1 = 7 rows


def test_r1cs_malformations_name_their_section(tmp_path):
    good = open(_r1cs_path(tmp_path), "rb").read()
    data, sec = circom._read_sections(_r1cs_path(tmp_path), b"r1cs", 1, circom._R1CS_NAMES, (1, 2))
    payload = lambda sid: bytes(data[sec[sid][0]:sec[sid][0] + sec[sid][1]])      # noqa: E731
    head, body, wmap = payload(1), payload(2), payload(3)
    del data

    def fails(sections, what, version=1, magic=b"r1cs"):
        with pytest.raises(ValueError, match=what):
            circom.ReadR1cs(_write(tmp_path / "bad.r1cs", _container(magic, sections, version)))

    assert circom.ReadR1cs(_write(tmp_path / "ok.r1cs", good)).nConstraints == 4
    fails([(1, head[:4] + (R + 2).to_bytes(32, "little") + head[36:]), (2, body), (3, wmap)], r"section 1 \(header\).*prime")
    fails([(1, struct.pack("<I", 48) + head[4:]), (2, body)], r"section 1 \(header\).*n8")
    fails([(1, head + b"\0"), (2, body)], r"section 1 \(header\) has 65 bytes")
    fails([(1, head), (2, body[:-36])], r"section 2 \(constraints\)")
    fails([(1, head), (2, body + bytes(4))], r"section 2 \(constraints\)")
    fails([(1, head), (2, body + bytes(3))], r"section 2 \(constraints\)")
    fails([(1, head), (3, wmap)], r"section 2 \(constraints\) is missing")
    fails([(2, body), (3, wmap)], r"section 1 \(header\) is missing")
    fails([(1, head), (2, body), (4, b"\x01\0\0\0")], r"section 4 \(custom gates list\)")
    fails([(1, head), (2, body), (5, b"\x01")], r"section 5 \(custom gates application\)")
    fails([(1, head[:36] + struct.pack("<I", 3) + head[40:]), (2, body)], r"section 1 \(header\).*nWires")       # fewer wires than inputs
    wire9 = struct.pack("<I", 1) + struct.pack("<I", 9) + (1).to_bytes(32, "little") + bytes(8)
    fails([(1, head[:60] + struct.pack("<I", 1)), (2, wire9)], r"section 2 \(constraints\): wire 9")
    fails([(1, head), (2, body)], "version 2", version=2)
    fails([(1, head), (2, body)], "not a .r1cs file", magic=b"zkey")
    assert circom.ReadR1cs(_write(tmp_path / "ok2.r1cs", _container(b"r1cs", [(3, wmap), (2, body), (4, b""), (1, head)]))).nConstraints == 4


@pytest.mark.parametrize("power", [0, 1, 3])
def test_ptau_counts(tmp_path, power):
    s = _ptau_sections(power)
    p = circom.ReadPtau(_write(tmp_path / "t.ptau", _container(b"ptau", [(sid, s[sid]) for sid in (1, 7, 2, 12, 3, 4, 5, 6)])))
    n = 1 << power
    assert (p.power, p.ceremonyPower) == (power, power)
    assert (p.tauG1.size, p.tauG2.size, p.alphaTauG1.size, p.betaTauG1.size, p.betaG2.size) == ((2 * n - 1) * 64, n * 128, n * 64, n * 64, 128)
    assert not p.tauG1.flags.writeable and p.tauG1.dtype == np.uint8


def test_ptau_malformations_name_their_section(tmp_path):
    s = _ptau_sections(2)

    def fails(changed, what, drop=()):
        t = dict(s)
        t.update(changed)
        with pytest.raises(ValueError, match=what):
            circom.ReadPtau(_write(tmp_path / "bad.ptau", _container(b"ptau", [(sid, t[sid]) for sid in sorted(t) if sid not in drop])))

    fails({1: _ptau_sections(2, prime=R)[1]}, r"section 1 \(header\).*prime")
    fails({1: struct.pack("<I", 31) + s[1][4:]}, r"section 1 \(header\).*n8")
    fails({1: s[1] + b"\0"}, r"section 1 \(header\) has 45 bytes")
    fails({1: _ptau_sections(2, ceremony=1)[1]}, r"section 1 \(header\).*power")
    fails({2: s[2] + bytes(64)}, r"section 2 \(tauG1\) has 512 bytes, its counts need 448")
    fails({3: s[3][:-128]}, r"section 3 \(tauG2\)")
    fails({4: s[4] + bytes(1)}, r"section 4 \(alphaTauG1\)")
    fails({5: bytes(0)}, r"section 5 \(betaTauG1\)")
    fails({6: bytes(64)}, r"section 6 \(betaG2\)")
    for sid, name in ((2, "tauG1"), (3, "tauG2"), (4, "alphaTauG1"), (5, "betaTauG1"), (6, "betaG2")):
        fails({}, r"section %d \(%s\) is missing" % (sid, name), drop=(sid,))


def test_setup_refuses_a_transcript_too_small_for_the_circuit(tmp_path):
    """4 constraints + 2 public signals + 1 need a domain of 2^3; the check comes before anything touches a device."""
    s = _ptau_sections(2)
    ptau = _write(tmp_path / "small.ptau", _container(b"ptau", sorted(s.items())))
    with pytest.raises(ValueError, match=r"section 1 \(header\): power = 2.*2\^3"):
        circom.SetupFromPtau(_r1cs_path(tmp_path), ptau, str(tmp_path / "out.zkey"))
