"""snarkjs / circom Groth16 files on the HIP library: the prover half of the reference's externalVerif/ (which only verifies).

    pkj = circom.ParseProvingKey(utils.ReadJSON("proving_key.json"))
    key, r1cs = circom.UploadProvingKey(pkj)                     # resident key + resident sparse R1CS over the domain 2^k
    circom.DeriveEvalBasis(key, pkj.domainBits)                  # optional, once per key: the coset evaluation-basis array
    proof = circom.GenerateProofs(key, r1cs, circom.ParseWitness(utils.ReadJSON("witness.json")))
    utils.WriteJSON("proof.json", circom.ProofToJSON(proof))
    ok = circom.VerifyFromCircom(vk_json, proof_json, public_json)      # externalVerif/circomVerifier.go:26-90

A snarkjs proving key is a QAP over the domain of the m = 2^domainBits-th roots of unity with Z = x^m - 1 (csrc/domain.h holds the
conventions; confirmed against snarkjs for domainBits = 2, the reference's externalVerif/circom-test fixture, and the same formula
above that).  It maps onto the engine's Groth16 key one to one:

    G1.At <- A     G1.BACGamma <- B1     G2.BACGamma <- B2     BACDelta <- C (null entries = infinity)     PowersTauDelta <- hExps
    alpha, beta, delta, beta2, delta2 <- vk_alfa_1, vk_beta_1, vk_delta_1, vk_beta_2, vk_delta_2      Z <- x^m - 1      NPublic <- nPublic

polsA/B/C[s] = {row c: coefficient of signal s in row c} are transposed into the CSR rows the device multiplies the witness with.
Values are decimal strings; ["0", "1", "0"] (Z = 0) is the point at infinity.

The binary files circom and snarkjs write today, circuit.zkey and witness.wtns:

    key, r1cs = circom.UploadZkey("circuit.zkey")                # the sections go to the device as they lie in the file
    proof = circom.GenerateProofs(key, r1cs, circom.ReadWtns("witness.wtns"))
    ok = circom.VerifyFromCircom(circom.VerificationKeyFromZkey(circom.ReadZkey("circuit.zkey")), proof, public)

A zkey has no C matrix (c_j = a_j b_j on the domain: a product system, gs_r1cs_upload_zkey) and no hExps: its section 9 is the coset
evaluation basis, so the key is coset-only (gs_groth16_pk_create_domain) and proves on that route alone.  The layout read here (ReadZkey,
ReadWtns below) is written down from snarkjs's source; NO FILE WRITTEN BY snarkjs ITSELF HAS BEEN READ YET -- the files this module has
seen are the ones its own WriteZkey / WriteWtns produce.  Should a real file disagree, the parser is what changes: the library takes
sections, not files."""
import struct

import numpy as np

from . import _scheme, capi, groth16, r1csqap, utils

R = groth16.R
G1_INF = (0, 1, 0)
G2_INF = ((0, 0), (1, 0), (0, 0))


def _g1(p):
    return G1_INF if p is None else tuple(int(c) for c in p)


def _g2(p):
    return G2_INF if p is None else tuple((int(c[0]), int(c[1])) for c in p)


class ProvingKey:
    """The fields of a snarkjs proving_key.json, as integers; rows_a/b/c: one {signal: coefficient} dict per constraint row."""

    def __init__(self, nVars, nPublic, domainBits, rows_a, rows_b, rows_c, A, B1, B2, C, hExps, alfa1, beta1, delta1, beta2, delta2):
        self.nVars, self.nPublic, self.domainBits = nVars, nPublic, domainBits
        self.rows_a, self.rows_b, self.rows_c = rows_a, rows_b, rows_c
        self.A, self.B1, self.B2, self.C, self.hExps = A, B1, B2, C, hExps
        self.alfa1, self.beta1, self.delta1, self.beta2, self.delta2 = alfa1, beta1, delta1, beta2, delta2

    @property
    def domainSize(self):
        return 1 << self.domainBits

    def csr(self):
        """(a_csr, b_csr, c_csr): (row_ptr uint32, col uint32, val [nnz, 4] uint64) each, over len(rows) constraints x nVars signals."""
        return tuple(r1csqap.csr_from_rows(rows) for rows in (self.rows_a, self.rows_b, self.rows_c))

    def Z(self):
        """x^m - 1 as m + 1 coefficients."""
        return [R - 1] + [0] * (self.domainSize - 1) + [1]


def TransposePols(pols_a, pols_b, pols_c, domain_size):
    """polsX[s] = {row: coefficient} per signal -> per matrix the list of rows {signal: coefficient}, cut behind the last row any of
    the three uses (the rows above it are empty: the device pads them up to the domain)."""
    n = 0
    for pols in (pols_a, pols_b, pols_c):
        for sig in pols:
            for c in sig:
                if not 0 <= int(c) < domain_size:
                    raise ValueError("error parsing proving key: row %s outside the domain of %d points" % (c, domain_size))
                n = max(n, int(c) + 1)
    out = []
    for pols in (pols_a, pols_b, pols_c):
        rows = [dict() for _ in range(n)]
        for s, sig in enumerate(pols):
            for c, v in sig.items():
                rows[int(c)][s] = int(v) % R
        out.append(rows)
    return tuple(out)


def ParseProvingKey(j):
    if j.get("protocol") not in ("groth", "groth16"):
        raise ValueError("error parsing proving key: protocol %r is not Groth16" % j.get("protocol"))
    nvars, k = int(j["nVars"]), int(j["domainBits"])
    if int(j["domainSize"]) != 1 << k:
        raise ValueError("error parsing proving key: domainSize is not 2^domainBits")
    for name in ("polsA", "polsB", "polsC", "A", "B1", "B2", "C"):
        if len(j[name]) != nvars:
            raise ValueError("error parsing proving key: %s has %d entries, nVars = %d" % (name, len(j[name]), nvars))
    rows = TransposePols(j["polsA"], j["polsB"], j["polsC"], 1 << k)
    return ProvingKey(nvars, int(j["nPublic"]), k, rows[0], rows[1], rows[2], [_g1(p) for p in j["A"]], [_g1(p) for p in j["B1"]],
                      [_g2(p) for p in j["B2"]], [_g1(p) for p in j["C"]], [_g1(p) for p in j["hExps"]], _g1(j["vk_alfa_1"]),
                      _g1(j["vk_beta_1"]), _g1(j["vk_delta_1"]), _g2(j["vk_beta_2"]), _g2(j["vk_delta_2"]))


def ParseVerificationKey(j):
    """verification_key.json -> groth16.Vk (circomVerifier.go:38-47; vk_alfabeta_12 is not used, as there)."""
    return groth16.Vk(IC=[_g1(p) for p in j["IC"]], G1_Alpha=_g1(j["vk_alfa_1"]), G2_Beta=_g2(j["vk_beta_2"]),
                      G2_Gamma=_g2(j["vk_gamma_2"]), G2_Delta=_g2(j["vk_delta_2"]))


def ParseProof(j):
    return groth16.Proof(_g1(j["pi_a"]), _g2(j["pi_b"]), _g1(j["pi_c"]))


def ParsePublic(j):
    return [int(x) for x in j]


def ParseWitness(j):
    return [int(x) for x in j]


def ProofToJSON(proof):
    """groth16.Proof -> the dictionary snarkjs writes as proof.json."""
    s1 = lambda p: [str(c) for c in p]                     # noqa: E731
    return {"pi_a": s1(proof.PiA), "pi_b": [[str(c[0]), str(c[1])] for c in proof.PiB], "pi_c": s1(proof.PiC), "protocol": "groth"}


class DeviceDomainR1CS(r1csqap.DeviceR1CS):
    """A sparse R1CS resident on the device as a QAP over the domain 2^log2_domain (gs_r1cs_upload_domain)."""

    def __init__(self, log2_domain, a_csr, b_csr, c_csr, nvars):
        self.log2_domain = int(log2_domain)
        self._upload("gs_r1cs_upload_domain", (self.log2_domain,), (a_csr, b_csr, c_csr), nvars)


def UploadProvingKey(pkj):
    """ProvingKey -> (groth16.DevicePk, DeviceDomainR1CS), both resident."""
    at = capi.g1_upload(capi.g1_points_to_u64(pkj.A))
    b1 = capi.g1_upload(capi.g1_points_to_u64(pkj.B1))
    b2 = capi.g2_upload(capi.g2_points_to_u64(pkj.B2))
    cd = capi.g1_upload(capi.g1_points_to_u64(pkj.C))
    pt = capi.g1_upload(capi.g1_points_to_u64(pkj.hExps))
    dev = groth16.device_pk_from_handles(at, b1, b2, cd, pt, pkj.alfa1, pkj.beta1, pkj.delta1, pkj.beta2, pkj.delta2,
                                         capi.ints_to_u64(pkj.Z()), pkj.nVars, pkj.nPublic)
    a, b, c = pkj.csr()
    return dev, DeviceDomainR1CS(pkj.domainBits, a, b, c, pkj.nVars)


def DeriveEvalBasis(dev_pk, log2_domain):
    """Compute the coset evaluation-basis array of a resident domain key from its hExps alone and attach it
    (gs_groth16_pk_derive_eval_domain: one transform of size 2^log2_domain in the group, once per key)."""
    _scheme.derive_basis(groth16._S, "eval_domain", dev_pk, int(log2_domain))


def SetEvalBasis(dev_pk, points, log2_domain):
    """Attach a coset evaluation-basis array (2^log2_domain Jacobian int triples, natural order) read from a file
    (gs_groth16_pk_set_eval_domain)."""
    _scheme.set_basis(groth16._S, "eval_domain", dev_pk, capi.g1_points_to_u64(points), int(log2_domain))


def GenerateProofsWithRS(dev_pk, dev_r1cs, w, r, s):
    """Witness -> proof against the resident key and R1CS: a host-buffer ticket collected at once, as groth16.GenerateProofsFromWitnessWithRS
    (the coset evaluation-basis route when the key holds the array, else px and the quotient by x^m - 1; same proof either way)."""
    return groth16.GenerateProofsFromWitnessWithRS(None, dev_pk, dev_r1cs, w, r, s)


def GenerateProofs(dev_pk, dev_r1cs, w, r=None, s=None):
    return GenerateProofsWithRS(dev_pk, dev_r1cs, w, groth16.FqRRand() if r is None else r, groth16.FqRRand() if s is None else s)


def VerifyFromCircom(vk, proof, public):
    """externalVerif/circomVerifier.go:26-90 on parsed JSON (dictionaries / lists as json.load returns them, or the parsed objects)
    -> bool, over gs_groth16_verify (host side, needs no device)."""
    vk = ParseVerificationKey(vk) if isinstance(vk, dict) else vk
    proof = ParseProof(proof) if isinstance(proof, dict) else proof
    return groth16.VerifyProof(vk, proof, [int(x) for x in public])


# ---- the binary key container (utils.WriteBinary) for domain keys: the key's arrays, the three CSR matrices, optionally E --------
_SECTIONS_G1 = (("G1.At", "A"), ("G1.BACGamma", "B1"), ("BACDelta", "C"), ("PowersTauDelta", "hExps"))
EVAL_SECTION = "PowersTauDeltaCoset"        # optional: the coset evaluation-basis array, 2^domainBits G1 points, natural order


def ProvingKeyToBinary(path, pkj, eval_points=None):
    """Write a parsed snarkjs key -- and, when given, its coset evaluation-basis array (e.g. groth16.ExportPkArray(key,
    "PowersTauDeltaEval") after DeriveEvalBasis) -- into the limb container."""
    sec = {name: capi.g1_points_to_u64(getattr(pkj, attr)) for name, attr in _SECTIONS_G1}
    sec["G2.BACGamma"] = capi.g2_points_to_u64(pkj.B2)
    sec["G1.ABD"] = capi.g1_points_to_u64([pkj.alfa1, pkj.beta1, pkj.delta1])
    sec["G2.BD"] = capi.g2_points_to_u64([pkj.beta2, pkj.delta2])
    sec["Domain"] = np.array([[pkj.domainBits, len(pkj.rows_a), 0, 0]], dtype=np.uint64)
    for name, csr in zip("ABC", pkj.csr()):
        sec["R1CS.%s.rowptr" % name] = csr[0].astype(np.uint64).reshape(-1, 1)
        sec["R1CS.%s.col" % name] = csr[1].astype(np.uint64).reshape(-1, 1)
        sec["R1CS.%s.val" % name] = csr[2].reshape(-1, 4)
    if eval_points is not None:
        if len(eval_points) != pkj.domainSize:
            raise ValueError("the coset evaluation-basis array has %d points, the domain %d" % (len(eval_points), pkj.domainSize))
        sec[EVAL_SECTION] = capi.g1_points_to_u64(eval_points)
    utils.WriteBinary(path, utils.PROTO_GROTH16, pkj.nVars, pkj.nPublic, sec)


def UploadProvingKeyBinary(path):
    """file -> (groth16.DevicePk, DeviceDomainR1CS); an EVAL_SECTION inside is attached with gs_groth16_pk_set_eval_domain."""
    protocol, nvars, npublic, sec = utils.ReadBinary(path)
    if protocol != utils.PROTO_GROTH16 or "Domain" not in sec:
        raise ValueError("error parsing key file: not a Groth16 key over a power-of-two domain")
    k = int(sec["Domain"][0][0])
    up1 = lambda name: capi.g1_upload(np.ascontiguousarray(sec[name], dtype=np.uint64))     # noqa: E731
    b2 = capi.g2_upload(np.ascontiguousarray(sec["G2.BACGamma"], dtype=np.uint64))
    abd, bd = utils._g1_tuples(sec["G1.ABD"]), utils._g2_tuples(sec["G2.BD"])
    z = capi.ints_to_u64([R - 1] + [0] * ((1 << k) - 1) + [1])
    dev = groth16.device_pk_from_handles(up1("G1.At"), up1("G1.BACGamma"), b2, up1("BACDelta"), up1("PowersTauDelta"), abd[0], abd[1], abd[2],
                                         bd[0], bd[1], z, nvars, npublic)
    csr = [(np.ascontiguousarray(sec["R1CS.%s.rowptr" % n]).reshape(-1).astype(np.uint32),
            np.ascontiguousarray(sec["R1CS.%s.col" % n]).reshape(-1).astype(np.uint32),
            np.ascontiguousarray(sec["R1CS.%s.val" % n], dtype=np.uint64).reshape(-1, 4)) for n in "ABC"]
    if EVAL_SECTION in sec:
        _scheme.set_basis(groth16._S, "eval_domain", dev, sec[EVAL_SECTION], k)
    return dev, DeviceDomainR1CS(k, csr[0], csr[1], csr[2], nvars)


# ---- circuit.zkey / witness.wtns -------------------------------------------------------------------------------------------------
# Container (both, little-endian): 4 bytes of magic, u32 version, u32 nSections; then per section u32 id, u64 length, payload.  Sections
# come in any order; unknown ids are skipped.
#   .wtns  "wtns" v2    1: u32 n8 (32), n8 bytes of prime (r), u32 nWitness       2: nWitness x 32 bytes, standard form
#   .zkey  "zkey" v1    1: u32 protocol (1 = Groth16)
#                       2: u32 n8q, q, u32 n8r, r, u32 nVars, u32 nPublic, u32 domainSize, alpha1, beta1, beta2, gamma2, delta1, delta2
#                       3: IC, nPublic + 1 G1       4: u32 nCoefs, nCoefs x (u32 matrix, u32 row, u32 signal, 32 bytes of v * 2^512 mod r)
#                       5: A, nVars G1    6: B1, nVars G1    7: B2, nVars G2    8: C, nVars - nPublic - 1 G1 (signals nPublic + 1 ..)
#                       9: H, domainSize G1: the coset evaluation basis, natural order          10: contributions (ignored)
# Points are affine: G1 x | y, G2 x.c0 | x.c1 | y.c0 | y.c1, each coordinate 32 bytes of value * 2^256 mod q; all zero = infinity.
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
_MONT = 1 << 256
_MONT_INV_Q = pow(_MONT, -1, Q)
_COEF_SHIFT = pow(2, 512, R)
_COEF_UNSHIFT = pow(_COEF_SHIFT, -1, R)
G1_BYTES, G2_BYTES, COEF_BYTES = 64, 128, 44
_ZKEY_NAMES = {1: "1 (protocol)", 2: "2 (header)", 3: "3 (IC)", 4: "4 (coefficients)", 5: "5 (A)", 6: "6 (B1)", 7: "7 (B2)", 8: "8 (C)",
               9: "9 (H)", 10: "10 (contributions)"}
_WTNS_NAMES = {1: "1 (header)", 2: "2 (witness)"}


def _read_sections(path, magic, version, names, required):
    """-> (the file as a read-only uint8 memory map, {id: (offset, length)})."""
    data = np.memmap(path, dtype=np.uint8, mode="r")
    what = magic.decode()
    if data.size < 12 or bytes(data[:4]) != magic:
        raise ValueError("%s: not a .%s file (magic %r)" % (path, what, bytes(data[:4])))
    ver, nsec = struct.unpack("<II", bytes(data[4:12]))
    if ver != version:
        raise ValueError("%s: .%s version %d, this reader knows version %d" % (path, what, ver, version))
    sec, pos = {}, 12
    for _ in range(nsec):
        if pos + 12 > data.size:
            raise ValueError("%s: the section table runs past the end of the file" % path)
        sid, length = struct.unpack("<IQ", bytes(data[pos:pos + 12]))
        pos += 12
        label = names.get(sid, str(sid))
        if pos + length > data.size:
            raise ValueError("%s: section %s (%d bytes) runs past the end of the file" % (path, label, length))
        if sid in names:
            if sid in sec:
                raise ValueError("%s: section %s appears twice" % (path, label))
            sec[sid] = (pos, length)
        pos += length
    for sid in required:
        if sid not in sec:
            raise ValueError("%s: section %s is missing" % (path, names[sid]))
    return data, sec


def _expect_len(path, names, sid, sec, want):
    if sec[sid][1] != want:
        raise ValueError("%s: section %s has %d bytes, its counts need %d" % (path, names[sid], sec[sid][1], want))


def ReadWtns(path):
    """witness.wtns -> read-only [nWitness, 4] uint64 view of the file: the C ABI's `w` as it lies there (values are not range-checked:
    the device takes any 256-bit word)."""
    data, sec = _read_sections(path, b"wtns", 2, _WTNS_NAMES, (1, 2))
    off, length = sec[1]
    if length < 4:
        raise ValueError("%s: section %s is too short" % (path, _WTNS_NAMES[1]))
    n8 = struct.unpack("<I", bytes(data[off:off + 4]))[0]
    if n8 != 32:
        raise ValueError("%s: section %s: n8 = %d, BN128 needs 32" % (path, _WTNS_NAMES[1], n8))
    _expect_len(path, _WTNS_NAMES, 1, sec, 4 + 32 + 4)
    if int.from_bytes(bytes(data[off + 4:off + 36]), "little") != R:
        raise ValueError("%s: section %s: the prime is not BN128's r" % (path, _WTNS_NAMES[1]))
    n = struct.unpack("<I", bytes(data[off + 36:off + 40]))[0]
    _expect_len(path, _WTNS_NAMES, 2, sec, n * 32)
    return np.ndarray((n, 4), dtype="<u8", buffer=data, offset=sec[2][0])


def WriteWtns(path, w):
    """Integers (reduced mod r) or an [n, 4] uint64 array -> witness.wtns."""
    rows = capi.u64_rows(w)
    head = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<I", rows.shape[0])
    with open(path, "wb") as f:
        f.write(b"wtns" + struct.pack("<II", 2, 2))
        f.write(struct.pack("<IQ", 1, len(head)) + head)
        f.write(struct.pack("<IQ", 2, rows.nbytes) + rows.astype("<u8").tobytes())


def _fq_from_mont(b):
    return int.from_bytes(bytes(b), "little") * _MONT_INV_Q % Q


def _fq_to_mont(v):
    return (v % Q * _MONT % Q).to_bytes(32, "little")


def G1FromZkey(b):
    """64 bytes -> Jacobian int triple (x, y, 1) / (0, 1, 0)."""
    b = bytes(b)
    if not any(b):
        return G1_INF
    return (_fq_from_mont(b[:32]), _fq_from_mont(b[32:]), 1)


def G2FromZkey(b):
    b = bytes(b)
    if not any(b):
        return G2_INF
    c = [_fq_from_mont(b[32 * i:32 * i + 32]) for i in range(4)]
    return ((c[0], c[1]), (c[2], c[3]), (1, 0))


def _fq2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % Q, (a[0] * b[1] + a[1] * b[0]) % Q)


def _fq2_inv(a):
    d = pow(a[0] * a[0] + a[1] * a[1], -1, Q)
    return (a[0] * d % Q, -a[1] * d % Q)


def G1ToZkey(p):
    """Jacobian int triple (any Z) -> the 64 bytes of the affine point."""
    x, y, z = p
    if z % Q == 0:
        return bytes(G1_BYTES)
    if z != 1:
        zi = pow(z, -1, Q)
        x, y = x * zi * zi % Q, y * zi * zi * zi % Q
    return _fq_to_mont(x) + _fq_to_mont(y)


def G2ToZkey(p):
    x, y, z = ((int(c[0]) % Q, int(c[1]) % Q) for c in p)
    if z == (0, 0):
        return bytes(G2_BYTES)
    if z != (1, 0):
        zi = _fq2_inv(z)
        zi2 = _fq2_mul(zi, zi)
        x, y = _fq2_mul(x, zi2), _fq2_mul(y, _fq2_mul(zi2, zi))
    return b"".join(_fq_to_mont(c) for c in (x[0], x[1], y[0], y[1]))


class Zkey:
    """A parsed circuit.zkey: the header as integers (the six points as Jacobian int tuples) and the array sections as read-only uint8
    views of the memory-mapped file (IC, coefs, A, B1, B2, C, H), which go to the device as they are."""

    def __init__(self, nVars, nPublic, domainSize, alfa1, beta1, beta2, gamma2, delta1, delta2, IC, coefs, A, B1, B2, C, H):
        self.nVars, self.nPublic, self.domainSize, self.domainBits = nVars, nPublic, domainSize, domainSize.bit_length() - 1
        self.alfa1, self.beta1, self.beta2, self.gamma2, self.delta1, self.delta2 = alfa1, beta1, beta2, gamma2, delta1, delta2
        self.IC, self.coefs, self.A, self.B1, self.B2, self.C, self.H = IC, coefs, A, B1, B2, C, H

    @property
    def nCoefs(self):
        return self.coefs.size // COEF_BYTES

    def g1(self, name):
        """Section `name` (IC, A, B1, C, H) as Jacobian int triples (host work: tests and export, not the prover's path)."""
        b = getattr(self, name).reshape(-1, G1_BYTES)
        return [G1FromZkey(r) for r in b]

    def g2(self, name="B2"):
        return [G2FromZkey(r) for r in getattr(self, name).reshape(-1, G2_BYTES)]

    def c_full(self):
        """C over all nVars signals, as proving_key.json has it: infinity for the signals 0 .. nPublic."""
        return [G1_INF] * (self.nPublic + 1) + self.g1("C")

    def rows(self):
        """(rows_a, rows_b): per matrix one {signal: coefficient} dict per row of the domain, repeated records added up (host work)."""
        out = ([dict() for _ in range(self.domainSize)], [dict() for _ in range(self.domainSize)])
        rec = self.coefs.reshape(-1, COEF_BYTES)
        for r in rec:
            mat, row, sig = struct.unpack("<III", bytes(r[:12]))
            v = int.from_bytes(bytes(r[12:]), "little") * _COEF_UNSHIFT % R
            out[mat][row][sig] = (out[mat][row].get(sig, 0) + v) % R
        return out


def ReadZkey(path):
    """circuit.zkey -> Zkey.  Every malformation is a ValueError that names the section."""
    N = _ZKEY_NAMES
    data, sec = _read_sections(path, b"zkey", 1, N, (1, 2, 3, 4, 5, 6, 7, 8, 9))
    view = lambda sid, skip=0: data[sec[sid][0] + skip:sec[sid][0] + sec[sid][1]]      # noqa: E731
    _expect_len(path, N, 1, sec, 4)
    protocol = struct.unpack("<I", bytes(view(1)))[0]
    if protocol != 1:
        raise ValueError("%s: section %s: protocol %d is not Groth16 (1)" % (path, N[1], protocol))
    h = bytes(view(2))
    pos = 0
    for name, prime in (("n8q", Q), ("n8r", R)):
        if len(h) < pos + 4:
            raise ValueError("%s: section %s is too short" % (path, N[2]))
        n8 = struct.unpack_from("<I", h, pos)[0]
        if n8 != 32:
            raise ValueError("%s: section %s: %s = %d, BN128 needs 32" % (path, N[2], name, n8))
        if int.from_bytes(h[pos + 4:pos + 36], "little") != prime or len(h) < pos + 36:
            raise ValueError("%s: section %s: the prime behind %s is not BN128's" % (path, N[2], name))
        pos += 36
    _expect_len(path, N, 2, sec, pos + 12 + 3 * G1_BYTES + 3 * G2_BYTES)
    nvars, npublic, m = struct.unpack_from("<III", h, pos)
    pos += 12
    if m < 2 or m & (m - 1) or m > 1 << 27:
        raise ValueError("%s: section %s: domainSize = %d is not a power of two in 2 .. 2^27" % (path, N[2], m))
    if npublic + 1 > nvars:
        raise ValueError("%s: section %s: nPublic + 1 = %d exceeds nVars = %d" % (path, N[2], npublic + 1, nvars))
    pts = []
    for g2 in (False, False, True, True, False, True):                # alpha1, beta1, beta2, gamma2, delta1, delta2
        size = G2_BYTES if g2 else G1_BYTES
        pts.append((G2FromZkey if g2 else G1FromZkey)(h[pos:pos + size]))
        pos += size
    _expect_len(path, N, 3, sec, (npublic + 1) * G1_BYTES)
    if sec[4][1] < 4:
        raise ValueError("%s: section %s is too short" % (path, N[4]))
    ncoefs = struct.unpack("<I", bytes(view(4)[:4]))[0]
    _expect_len(path, N, 4, sec, 4 + ncoefs * COEF_BYTES)
    for sid, count, size in ((5, nvars, G1_BYTES), (6, nvars, G1_BYTES), (7, nvars, G2_BYTES), (8, nvars - npublic - 1, G1_BYTES), (9, m, G1_BYTES)):
        _expect_len(path, N, sid, sec, count * size)
    return Zkey(nvars, npublic, m, pts[0], pts[1], pts[2], pts[3], pts[4], pts[5], view(3), view(4, 4), view(5), view(6), view(7), view(8), view(9))


def CoefRecords(rows_a, rows_b):
    """Two lists of {signal: coefficient} rows -> the records of section 4 as bytes (A's rows, then B's)."""
    out = []
    for mat, rows in enumerate((rows_a, rows_b)):
        for row, entries in enumerate(rows):
            for sig, v in entries.items():
                out.append(struct.pack("<III", mat, row, sig) + (int(v) % R * _COEF_SHIFT % R).to_bytes(32, "little"))
    return out


def WriteZkey(path, pkj, vk, eval_points, order=None, records=None, extra_sections=()):
    """A parsed ProvingKey, its verification key (groth16.Vk: IC and gamma2 come from there) and the domainSize points of its coset
    evaluation basis E -> circuit.zkey.  Host code, for fixtures and for interoperability.  polsC is dropped: the file has no C matrix.
    `order`: the section ids in the order to write them (default 1 .. 9); `records`: the records of section 4 when not CoefRecords' own
    (tests: shuffled, repeated); `extra_sections`: (id, bytes) pairs written behind the others."""
    m = pkj.domainSize
    if len(eval_points) != m:
        raise ValueError("the coset evaluation-basis array has %d points, the domain %d" % (len(eval_points), m))
    if len(vk.IC) != pkj.nPublic + 1:
        raise ValueError("vk.IC has %d points, nPublic + 1 = %d" % (len(vk.IC), pkj.nPublic + 1))
    rec = CoefRecords(pkj.rows_a, pkj.rows_b) if records is None else list(records)
    g1s = lambda pts: b"".join(G1ToZkey(p) for p in pts)                  # noqa: E731
    head = struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<I", 32) + R.to_bytes(32, "little")
    head += struct.pack("<III", pkj.nVars, pkj.nPublic, m)
    head += G1ToZkey(pkj.alfa1) + G1ToZkey(pkj.beta1) + G2ToZkey(pkj.beta2) + G2ToZkey(vk.G2_Gamma) + G1ToZkey(pkj.delta1) + G2ToZkey(pkj.delta2)
    body = {1: struct.pack("<I", 1), 2: head, 3: g1s(vk.IC), 4: struct.pack("<I", len(rec)) + b"".join(rec), 5: g1s(pkj.A), 6: g1s(pkj.B1),
            7: b"".join(G2ToZkey(p) for p in pkj.B2), 8: g1s(pkj.C[pkj.nPublic + 1:]), 9: g1s(eval_points)}
    secs = [(sid, body[sid]) for sid in (order or range(1, 10))] + list(extra_sections)
    with open(path, "wb") as f:
        f.write(b"zkey" + struct.pack("<II", 1, len(secs)))
        for sid, payload in secs:
            f.write(struct.pack("<IQ", sid, len(payload)) + payload)


def VerificationKeyFromZkey(z):
    """Sections 2 and 3 of a parsed Zkey (or of the file at a path) -> groth16.Vk."""
    z = ReadZkey(z) if isinstance(z, str) else z
    return groth16.Vk(IC=z.g1("IC"), G1_Alpha=z.alfa1, G2_Beta=z.beta2, G2_Gamma=z.gamma2, G2_Delta=z.delta2)


class DeviceZkeyR1CS(DeviceDomainR1CS):
    """The A and B of a zkey resident as a product system (gs_r1cs_upload_zkey): built on the device from the records of section 4."""

    def __init__(self, log2_domain, nvars, coefs):
        capi.init()
        self.log2_domain, self.n, self.nvars = int(log2_domain), 1 << int(log2_domain), nvars
        p, keep = capi.byte_ptr(coefs)
        cell = capi.HandleCell()
        capi.call("gs_r1cs_upload_zkey", self.log2_domain, nvars, p, keep.size // COEF_BYTES, cell.ref)
        self.handle = cell.result()


def UploadZkey(path):
    """circuit.zkey -> (groth16.DevicePk, DeviceDomainR1CS): a coset-only key and a product system.  The array sections go to the device
    as memory-mapped bytes; only the six points of the header pass through Python integers."""
    z = ReadZkey(path) if isinstance(path, str) else path
    at = capi.g1_upload_affine_mont(z.A)
    b1 = capi.g1_upload_affine_mont(z.B1)
    b2 = capi.g2_upload_affine_mont(z.B2)
    cd = capi.g1_upload_affine_mont(np.concatenate([np.zeros((z.nPublic + 1) * G1_BYTES, dtype=np.uint8), z.C]))
    he = capi.g1_upload_affine_mont(z.H)
    dev = groth16.device_pk_domain_from_handles(at, b1, b2, cd, he, z.alfa1, z.beta1, z.delta1, z.beta2, z.delta2, z.domainBits, z.nVars, z.nPublic)
    return dev, DeviceZkeyR1CS(z.domainBits, z.nVars, z.coefs)


def ConvertProvingKey(pkj, vk_json, path):
    """An old proving_key.json (parsed) + its verification_key.json -> circuit.zkey at `path`.  E is derived on the device from hExps
    (DeriveEvalBasis) and read back; polsC is dropped."""
    vk = ParseVerificationKey(vk_json) if isinstance(vk_json, dict) else vk_json
    key, _ = UploadProvingKey(pkj)
    DeriveEvalBasis(key, pkj.domainBits)
    WriteZkey(path, pkj, vk, groth16.ExportPkArray(key, "PowersTauDeltaEval"))
