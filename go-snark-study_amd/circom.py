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
import shutil
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


def GenerateProofsChecked(dev_pk, dev_r1cs, w, check_r1cs=None, r=None, s=None):
    """GenerateProofs that refuses a witness which breaks a constraint (r1csqap.WitnessError, nothing proved).  check_r1cs: the system
    the witness is checked against, default dev_r1cs -- for a .zkey key, whose own system is a product system without C, the
    three-matrix system of circuit.r1cs (a DeviceDomainR1CS; CheckWtns builds the same one)."""
    return groth16.GenerateProofsChecked(None, dev_pk, dev_r1cs, w, r, s, check_r1cs)


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


# ---- circuit.r1cs / a powers-of-tau transcript -> circuit.zkey -------------------------------------------------------------------
# The container is the one of .zkey / .wtns (_read_sections).  Layouts as published by iden3 (r1cs binary format, snarkjs ptau files); as
# for .zkey, NO FILE WRITTEN BY circom / snarkjs ITSELF HAS BEEN READ YET: ReadR1cs and ReadPtau are the only places that know them.
#   .r1cs  "r1cs" v1    1: u32 n8 (32), r, u32 nWires, u32 nPubOut, u32 nPubIn, u32 nPrvIn, u64 nLabels, u32 nConstraints
#                       2: per constraint the linear combinations A, B, C: u32 nTerms, nTerms x (u32 wire, 32 bytes, standard form)
#                       3: wire -> label map (ignored)      4, 5: custom gates (must be empty)
#   .ptau  "ptau" v1    1: u32 n8 (32), q, u32 power, u32 ceremonyPower
#                       2: tauG1, 2^(power+1) - 1 G1     3: tauG2, 2^power G2     4: alphaTauG1, 2^power G1     5: betaTauG1, 2^power G1
#                       6: betaG2, one G2                7: contributions, 12 - 15: prepared Lagrange bases (ReadPtau ignores them)
#                       12: tauG1 Lagrange, levels 0 .. power+1, 2^(power+2) - 1 G1     13: tauG2 Lagrange, levels 0 .. power, 2^(power+1) - 1 G2
#                       14: alphaTauG1 Lagrange, 15: betaTauG1 Lagrange, levels 0 .. power, 2^(power+1) - 1 G1 each
#                       level p = the Lagrange basis of the domain 2^p over the section's first 2^p points, at point offset 2^p - 1; level
#                       power+1 of section 12 is the transform of the 2^(power+1) - 1 tauG1 points and one point at infinity.  This is the
#                       layout `snarkjs powersoftau prepare phase2` writes as far as its source is understood here: like the rest, it has
#                       not been checked against a file snarkjs wrote (ReadPtauPrepared is the only place that knows it).
# Points are in the .zkey encoding.
_R1CS_NAMES = {1: "1 (header)", 2: "2 (constraints)", 3: "3 (wire map)", 4: "4 (custom gates list)", 5: "5 (custom gates application)"}
_PTAU_NAMES = {1: "1 (header)", 2: "2 (tauG1)", 3: "3 (tauG2)", 4: "4 (alphaTauG1)", 5: "5 (betaTauG1)", 6: "6 (betaG2)"}
# ReadPtauPrepared's table: ReadPtau keeps the one above and with it its indifference to whatever sits in sections 12 - 15
_PTAU_PREPARED_NAMES = {**_PTAU_NAMES, 12: "12 (tauG1 Lagrange)", 13: "13 (tauG2 Lagrange)", 14: "14 (alphaTauG1 Lagrange)",
                        15: "15 (betaTauG1 Lagrange)"}
G1_GEN, G2_GEN = (1, 2, 1), ((10857046999023057135944570762232829481370756359578518086990519993285655852781,
                              11559732032986387107991004021392285783925812861821192530917403151452391805634),
                             (8495653923123431417604973247489272438418190587263600148770280649306958101930,
                              4082367875863433681332203403145435568316851327593401208105741076214120093531), (1, 0))


class R1cs:
    """A parsed circuit.r1cs: the counts of its header and the three matrices as CSR triples (row_ptr uint32 [nConstraints + 1], col uint32
    [nnz], val uint64 [nnz, 4], as they stand in the file: unsorted, repeated wires stay separate terms, values are not reduced)."""

    def __init__(self, nWires, nPubOut, nPubIn, nPrvIn, nLabels, nConstraints, a, b, c):
        self.nWires, self.nPubOut, self.nPubIn, self.nPrvIn, self.nLabels, self.nConstraints = nWires, nPubOut, nPubIn, nPrvIn, nLabels, nConstraints
        self.nVars, self.nPublic = nWires, nPubOut + nPubIn
        self.a, self.b, self.c = a, b, c


def ReadR1cs(path):
    """circuit.r1cs -> R1cs.  Every malformation is a ValueError that names the section."""
    N = _R1CS_NAMES
    data, sec = _read_sections(path, b"r1cs", 1, N, (1, 2))
    for sid in (4, 5):
        if sid in sec and sec[sid][1]:
            raise ValueError("%s: section %s is not empty: circuits with custom gates are not supported by Groth16" % (path, N[sid]))
    off, length = sec[1]
    if length < 4:
        raise ValueError("%s: section %s is too short" % (path, N[1]))
    n8 = struct.unpack("<I", bytes(data[off:off + 4]))[0]
    if n8 != 32:
        raise ValueError("%s: section %s: n8 = %d, BN128 needs 32" % (path, N[1], n8))
    _expect_len(path, N, 1, sec, 4 + 32 + 16 + 8 + 4)
    if int.from_bytes(bytes(data[off + 4:off + 36]), "little") != R:
        raise ValueError("%s: section %s: the prime is not BN128's r" % (path, N[1]))
    nwires, npubout, npubin, nprvin, nlabels, ncons = struct.unpack("<IIIIQI", bytes(data[off + 36:off + 64]))
    if 1 + npubout + npubin + nprvin > nwires:
        raise ValueError("%s: section %s: 1 + nPubOut + nPubIn + nPrvIn = %d exceeds nWires = %d" % (path, N[1], 1 + npubout + npubin + nprvin, nwires))
    off, length = sec[2]
    bad_len = ValueError("%s: section %s has %d bytes, which its %d constraints do not fill exactly" % (path, N[2], length, ncons))
    if length % 4:
        raise bad_len
    words = data[off:off + length].view("<u4")
    # the count word of every linear combination: one step per combination (its position depends on the counts before it) ...
    nlc = 3 * ncons
    pos, cnt = np.zeros(nlc, dtype=np.int64), np.zeros(nlc, dtype=np.int64)
    p, nw = 0, words.size
    for j in range(nlc):
        if p >= nw:
            raise bad_len
        pos[j], cnt[j] = p, words[p]
        p += 1 + 9 * int(words[p])
    if p != nw:
        raise bad_len
    # ... and every term at once: word index of term t of combination j = pos[j] + 1 + 9 t
    first = np.cumsum(cnt) - cnt
    at = np.repeat(pos + 1 - 9 * first, cnt) + 9 * np.arange(int(cnt.sum()), dtype=np.int64)
    wires = np.asarray(words[at], dtype=np.uint32)
    if wires.size and int(wires.max()) >= nwires:
        raise ValueError("%s: section %s: wire %d, the circuit has %d" % (path, N[2], int(wires.max()), nwires))
    vals = np.ascontiguousarray(np.asarray(words)[at[:, None] + np.arange(1, 9)], dtype="<u4").view("<u8").reshape(-1, 4)
    which = np.repeat(np.arange(nlc, dtype=np.int64) % 3, cnt)
    csr = []
    for k in range(3):
        rp = np.concatenate([[0], np.cumsum(cnt[k::3])]).astype(np.uint32)
        csr.append((rp, wires[which == k], vals[which == k]))
    return R1cs(nwires, npubout, npubin, nprvin, nlabels, ncons, csr[0], csr[1], csr[2])


def WriteR1cs(path, nWires, nPubOut, nPubIn, nPrvIn, constraints, extra_sections=()):
    """constraints: (A, B, C) per constraint, each a list of (wire, value) pairs (values as they are given, below 2^256) -> circuit.r1cs.
    For fixtures and tests."""
    body = []
    for lcs in constraints:
        for lc in lcs:
            body.append(struct.pack("<I", len(lc)) + b"".join(struct.pack("<I", int(w)) + int(v).to_bytes(32, "little") for w, v in lc))
    body = b"".join(body)
    head = struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<IIIIQI", nWires, nPubOut, nPubIn, nPrvIn, nWires, len(constraints))
    secs = [(1, head), (2, body), (3, np.arange(nWires, dtype="<u8").tobytes())] + list(extra_sections)
    with open(path, "wb") as f:
        f.write(b"r1cs" + struct.pack("<II", 1, len(secs)))
        for sid, payload in secs:
            f.write(struct.pack("<IQ", sid, len(payload)) + payload)


class Ptau:
    """A parsed powers-of-tau file: power, ceremonyPower and the point sections as read-only uint8 views of the memory-mapped file."""

    def __init__(self, power, ceremonyPower, tauG1, tauG2, alphaTauG1, betaTauG1, betaG2):
        self.power, self.ceremonyPower = power, ceremonyPower
        self.tauG1, self.tauG2, self.alphaTauG1, self.betaTauG1, self.betaG2 = tauG1, tauG2, alphaTauG1, betaTauG1, betaG2


def ReadPtau(path):
    """A .ptau file -> Ptau.  Every malformation is a ValueError that names the section."""
    N = _PTAU_NAMES
    data, sec = _read_sections(path, b"ptau", 1, N, (1, 2, 3, 4, 5, 6))
    off, length = sec[1]
    if length < 4:
        raise ValueError("%s: section %s is too short" % (path, N[1]))
    n8 = struct.unpack("<I", bytes(data[off:off + 4]))[0]
    if n8 != 32:
        raise ValueError("%s: section %s: n8 = %d, BN128 needs 32" % (path, N[1], n8))
    _expect_len(path, N, 1, sec, 4 + 32 + 8)
    if int.from_bytes(bytes(data[off + 4:off + 36]), "little") != Q:
        raise ValueError("%s: section %s: the prime is not BN128's q" % (path, N[1]))
    power, ceremony = struct.unpack("<II", bytes(data[off + 36:off + 44]))
    if power > 28 or ceremony < power:
        raise ValueError("%s: section %s: power = %d (ceremonyPower = %d) is not in 0 .. 28" % (path, N[1], power, ceremony))
    for sid, count, size in ((2, (2 << power) - 1, G1_BYTES), (3, 1 << power, G2_BYTES), (4, 1 << power, G1_BYTES), (5, 1 << power, G1_BYTES),
                             (6, 1, G2_BYTES)):
        _expect_len(path, N, sid, sec, count * size)
    view = lambda sid: data[sec[sid][0]:sec[sid][0] + sec[sid][1]]      # noqa: E731
    return Ptau(power, ceremony, view(2), view(3), view(4), view(5), view(6))


def WritePtau(path, power, tau, alpha, beta, extra_sections=()):
    """The transcript of the toxic scalars tau, alpha, beta -> a .ptau file of 2^power (fixtures and tests; the points come from the
    device's fixed-base multiplication, so this needs one)."""
    n = 1 << power
    pw = [1]
    for _ in range(2 * n - 2):
        pw.append(pw[-1] * tau % R)
    g1 = lambda s: capi.g1_download_affine_mont(capi.g1_fixed_base(capi.ints_to_u64(s))).tobytes()      # noqa: E731
    g2 = lambda s: capi.g2_download_affine_mont(capi.g2_fixed_base(capi.ints_to_u64(s))).tobytes()      # noqa: E731
    head = struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<II", power, power)
    secs = [(1, head), (2, g1(pw)), (3, g2(pw[:n])), (4, g1([alpha * t % R for t in pw[:n]])), (5, g1([beta * t % R for t in pw[:n]])),
            (6, g2([beta % R]))] + list(extra_sections)
    with open(path, "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, len(secs)))
        for sid, payload in secs:
            f.write(struct.pack("<IQ", sid, len(payload)) + payload)


def NewPtau(path, power):
    """The transcript of tau = alpha = beta = 1 -> a .ptau file of 2^power: every point is its generator, sections 1 - 6.  The starting
    point of a chain of ContributePtau calls; host code only, written in pieces (power 28 is a 137 GB file, not 137 GB of memory)."""
    power = int(power)
    if not 0 <= power <= 28:
        raise ValueError("%s: power = %d is not in 0 .. 28" % (path, power))
    n = 1 << power
    g1, g2 = G1ToZkey(G1_GEN), G2ToZkey(G2_GEN)
    head = struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<II", power, power)
    piece = 1 << 16                                                 # points per write
    with open(path, "wb") as f:
        f.write(b"ptau" + struct.pack("<II", 1, 6))
        f.write(struct.pack("<IQ", 1, len(head)) + head)
        for sid, point, count in ((2, g1, 2 * n - 1), (3, g2, n), (4, g1, n), (5, g1, n), (6, g2, 1)):
            f.write(struct.pack("<IQ", sid, count * len(point)))
            block = point * min(count, piece)
            for _ in range(count // piece):
                f.write(block)
            f.write(point * (count % piece))


_PTAU_PREPARED = (12, 13, 14, 15)      # the prepared Lagrange bases of a transcript: stale after a contribution, and computed here anyway


def _ptau_section_list(data):
    """Every section of an already validated .ptau memory map, in file order: [(id, offset, length)]."""
    nsec = struct.unpack("<I", bytes(data[8:12]))[0]
    out, pos = [], 12
    for _ in range(nsec):
        sid, length = struct.unpack("<IQ", bytes(data[pos:pos + 12]))
        out.append((sid, pos + 12, length))
        pos += 12 + length
    return out


def ContributePtau(ptau_in, ptau_out, tau, alpha, beta, slab_log2=22, timing=None):
    """One phase-1 contribution with the secrets tau, alpha, beta, on the points (nobody needs to know the transcript's own tau):
        tauG1[i] *= tau^i    tauG2[i] *= tau^i    alphaTauG1[i] *= alpha tau^i    betaTauG1[i] *= beta tau^i    betaG2 *= beta
    Every section streams through the device in slabs of at most 2^slab_log2 points -- memory-mapped input -> gs_g*_upload_affine_mont ->
    gs_g*_scale_powers -> gs_g*_download_affine_mont into the memory-mapped output -- the slab that starts at index s with the factor
    c tau^s, and a slab's handles are freed before the next is uploaded: the device holds the input and the output of one slab (beside
    the upload's staging copy and the series of that slab), whatever the power.  The header is copied (ceremonyPower included); section 7 and every unknown section are copied as found; the prepared
    Lagrange bases, sections 12 - 15, are DROPPED: they would be stale, and SetupFromPtau computes the bases itself.
    NO CONTRIBUTION RECORD IS WRITTEN: no proof of knowledge of the secrets, no challenge hash, nothing appended to section 7 -- the same
    statement ContributeDelta makes for a key.  The result is a transcript for SetupFromPtau / VerifyPtau of this module; `snarkjs
    powersoftau verify` checks the chain of records and will not accept it.
    `timing`: a dict that receives the wall milliseconds of parsing, uploads, downloads and file writing, the device milliseconds of the
    multiplications (gs_last_timing), the wall milliseconds of the whole call and the largest gs_memory_query library_bytes seen between
    two device calls."""
    import os
    import time
    t0 = time.perf_counter()
    tau, alpha, beta = int(tau) % R, int(alpha) % R, int(beta) % R
    for name, v in (("tau", tau), ("alpha", alpha), ("beta", beta)):
        if v == 0:
            raise ValueError("%s must not be 0 mod r" % name)
    slab_log2 = int(slab_log2)
    if not 0 <= slab_log2 <= 28:
        raise ValueError("slab_log2 = %d is not in 0 .. 28" % slab_log2)
    ptau = ReadPtau(ptau_in)
    if os.path.exists(ptau_out) and os.path.samefile(ptau_in, ptau_out):
        raise ValueError("%s: the output must not be the input file (the input is read while the output is written)" % ptau_out)
    data = np.memmap(ptau_in, dtype=np.uint8, mode="r")
    keep = [s for s in _ptau_section_list(data) if s[0] not in _PTAU_PREPARED]
    ms = {"parse_ms": (time.perf_counter() - t0) * 1e3, "upload_ms": 0.0, "device_ms": 0.0, "download_ms": 0.0, "write_ms": 0.0,
          "library_bytes_max": 0, "slabs": 0}
    capi.init()
    t1 = time.perf_counter()
    with open(ptau_out, "wb") as f:
        f.truncate(12 + sum(12 + length for _, _, length in keep))
    out = np.memmap(ptau_out, dtype=np.uint8, mode="r+")
    put = lambda at, b: out.__setitem__(slice(at, at + len(b)), np.frombuffer(b, dtype=np.uint8))      # noqa: E731
    put(0, b"ptau" + struct.pack("<II", 1, len(keep)))
    ms["write_ms"] += (time.perf_counter() - t1) * 1e3
    # section id -> (point bytes, upload, scale, download, the factor of point 0, the ratio)
    g1 = (G1_BYTES, capi.g1_upload_affine_mont, capi.g1_scale_powers, capi.g1_download_affine_mont)
    g2 = (G2_BYTES, capi.g2_upload_affine_mont, capi.g2_scale_powers, capi.g2_download_affine_mont)
    plan = {2: g1 + (1, tau), 3: g2 + (1, tau), 4: g1 + (alpha, tau), 5: g1 + (beta, tau), 6: g2 + (beta, 1)}
    slab, pos = 1 << slab_log2, 12
    for sid, off, length in keep:
        put(pos, struct.pack("<IQ", sid, length))
        pos += 12
        if sid not in plan:
            t1 = time.perf_counter()
            out[pos:pos + length] = data[off:off + length]
            ms["write_ms"] += (time.perf_counter() - t1) * 1e3
            pos += length
            continue
        size, up, scale, down, c, t = plan[sid]
        for s in range(0, length // size, slab):
            cnt = min(slab, length // size - s)
            t1 = time.perf_counter()
            src = up(data[off + s * size:off + (s + cnt) * size])
            t2 = time.perf_counter()
            dst = scale(src, 0, cnt, c * pow(t, s, R) % R, t)
            ms["device_ms"] += capi.last_timing()["total_ms"]
            ms["library_bytes_max"] = max(ms["library_bytes_max"], capi.memory_query()["library_bytes"])
            src.free()
            t3 = time.perf_counter()
            down(dst, out[pos + s * size:pos + (s + cnt) * size])
            dst.free()
            ms["upload_ms"] += (t2 - t1) * 1e3
            ms["download_ms"] += (time.perf_counter() - t3) * 1e3
            ms["slabs"] += 1
        pos += length
    t1 = time.perf_counter()
    out.flush()
    del out
    ms["write_ms"] += (time.perf_counter() - t1) * 1e3
    if timing is not None:
        timing.update(ms, wall_ms=(time.perf_counter() - t0) * 1e3, power=ptau.power)


# prepared section -> (the section it is the Lagrange form of, its top level beyond `power`, point bytes)
_PTAU_LEVELS = {12: (2, 1, G1_BYTES), 13: (3, 0, G2_BYTES), 14: (4, 0, G1_BYTES), 15: (5, 0, G1_BYTES)}


class PtauPrepared(Ptau):
    """Ptau plus the prepared sections: `lagrange[sid]` (sid = 12 .. 15) is the read-only uint8 view of a section, level(sid, p) the view
    of its level p -- the Lagrange basis of the domain 2^p, 2^p points at point offset 2^p - 1."""

    def __init__(self, ptau, lagrange):
        Ptau.__init__(self, ptau.power, ptau.ceremonyPower, ptau.tauG1, ptau.tauG2, ptau.alphaTauG1, ptau.betaTauG1, ptau.betaG2)
        self.lagrange = dict(lagrange)

    def top_level(self, sid):
        return self.power + _PTAU_LEVELS[sid][1]

    def level(self, sid, p):
        size = _PTAU_LEVELS[sid][2]
        if not 0 <= p <= self.top_level(sid):
            raise ValueError("section %s holds the levels 0 .. %d, level %d was asked for" % (_PTAU_PREPARED_NAMES[sid], self.top_level(sid), p))
        return self.lagrange[sid][((1 << p) - 1) * size:((2 << p) - 1) * size]


def ReadPtauPrepared(path):
    """A prepared .ptau file -> PtauPrepared: what ReadPtau returns plus the sections 12 - 15 (layout: the comment above ReadR1cs; NOT yet
    checked against a file written by snarkjs).  A missing prepared section or one of the wrong length is a ValueError that names it.
    The points are NOT checked here: VerifyPtauPrepared does that."""
    ptau = ReadPtau(path)
    N = _PTAU_PREPARED_NAMES
    data, sec = _read_sections(path, b"ptau", 1, N, _PTAU_PREPARED)
    for sid in _PTAU_PREPARED:
        _, extra, size = _PTAU_LEVELS[sid]
        _expect_len(path, N, sid, sec, ((2 << (ptau.power + extra)) - 1) * size)
    return PtauPrepared(ptau, {sid: data[sec[sid][0]:sec[sid][0] + sec[sid][1]] for sid in _PTAU_PREPARED})


def PreparePtau(ptau_in, ptau_out, batch_log2=20, timing=None):
    """What `snarkjs powersoftau prepare phase2` does, on the device: the Lagrange bases of every domain 2^0 .. 2^power (2^(power+1) for
    tauG1) of the four array sections, appended as sections 12 - 15.  Every section of the input is copied in file order -- an existing
    12 - 15 is dropped and recomputed -- then 12, 13, 14, 15 follow.  Per section: one upload, ONE gs_g*_lagrange_levels call for the
    levels 0 .. min(top, batch_log2) (every level's stage of one span in one launch), one gs_g*_lagrange call per level above; each result
    goes straight into its place in the memory-mapped output and its handle is freed before the next call.  Level power+1 of tauG1 is the
    transform of its 2^(power+1) - 1 points and one point at infinity.  power <= 26 (level power+1 is a transform of 2^27 points at most).
    NO CONTRIBUTION RECORD IS READ OR WRITTEN, as in ContributePtau; the result is for SetupFromPtau(prepared=True) / VerifyPtauPrepared.
    `timing`: as ContributePtau's -- wall milliseconds of parsing, uploads, downloads and file writing, device milliseconds of the
    transforms, the wall milliseconds of the whole call, the largest library_bytes seen, the number of device calls."""
    import os
    import time
    t0 = time.perf_counter()
    batch_log2 = int(batch_log2)
    if not 0 <= batch_log2 <= 27:
        raise ValueError("batch_log2 = %d is not in 0 .. 27" % batch_log2)
    ptau = ReadPtau(ptau_in)
    if ptau.power > 26:
        raise ValueError("%s: section %s: power = %d, preparing needs power <= 26 (level power + 1 is one transform of at most 2^27 points)"
                         % (ptau_in, _PTAU_NAMES[1], ptau.power))
    if os.path.exists(ptau_out) and os.path.samefile(ptau_in, ptau_out):
        raise ValueError("%s: the output must not be the input file (the input is read while the output is written)" % ptau_out)
    data = np.memmap(ptau_in, dtype=np.uint8, mode="r")
    keep = [s for s in _ptau_section_list(data) if s[0] not in _PTAU_PREPARED]
    new = [(sid, ((2 << (ptau.power + _PTAU_LEVELS[sid][1])) - 1) * _PTAU_LEVELS[sid][2]) for sid in _PTAU_PREPARED]
    ms = {"parse_ms": (time.perf_counter() - t0) * 1e3, "upload_ms": 0.0, "device_ms": 0.0, "download_ms": 0.0, "write_ms": 0.0,
          "library_bytes_max": 0, "calls": 0}
    capi.init()
    t1 = time.perf_counter()
    with open(ptau_out, "wb") as f:
        f.truncate(12 + sum(12 + length for _, _, length in keep) + sum(12 + length for _, length in new))
    out = np.memmap(ptau_out, dtype=np.uint8, mode="r+")
    put = lambda at, b: out.__setitem__(slice(at, at + len(b)), np.frombuffer(b, dtype=np.uint8))      # noqa: E731
    put(0, b"ptau" + struct.pack("<II", 1, len(keep) + len(new)))
    pos = 12
    for sid, off, length in keep:
        put(pos, struct.pack("<IQ", sid, length))
        out[pos + 12:pos + 12 + length] = data[off:off + length]
        pos += 12 + length
    ms["write_ms"] += (time.perf_counter() - t1) * 1e3
    source = {2: ptau.tauG1, 3: ptau.tauG2, 4: ptau.alphaTauG1, 5: ptau.betaTauG1}
    g1 = (capi.g1_upload_affine_mont, capi.g1_lagrange_levels, capi.g1_lagrange, capi.g1_download_affine_mont)
    g2 = (capi.g2_upload_affine_mont, capi.g2_lagrange_levels, capi.g2_lagrange, capi.g2_download_affine_mont)
    for sid, length in new:
        put(pos, struct.pack("<IQ", sid, length))
        pos += 12
        src_id, extra, size = _PTAU_LEVELS[sid]
        up, levels, single, down = g2 if size == G2_BYTES else g1
        top, batch = ptau.power + extra, min(ptau.power + extra, batch_log2)
        points = source[src_id]
        if extra and batch < top:            # the single-level call of level power + 1 takes 2^(power+1) points: the last is the format's infinity
            points = np.concatenate([points, np.zeros(size, dtype=np.uint8)])

        def run(fn, at, count, *args):
            dst = fn(src, *args)
            ms["device_ms"] += capi.last_timing()["total_ms"]
            ms["library_bytes_max"] = max(ms["library_bytes_max"], capi.memory_query()["library_bytes"])
            t3 = time.perf_counter()
            down(dst, out[pos + at * size:pos + (at + count) * size])
            dst.free()
            ms["download_ms"] += (time.perf_counter() - t3) * 1e3
            ms["calls"] += 1

        t1 = time.perf_counter()
        src = up(points)
        ms["upload_ms"] += (time.perf_counter() - t1) * 1e3
        run(levels, 0, (2 << batch) - 1, 0, batch)
        for p in range(batch + 1, top + 1):
            run(single, (1 << p) - 1, 1 << p, p)
        src.free()
        pos += length
    t1 = time.perf_counter()
    out.flush()
    del out
    ms["write_ms"] += (time.perf_counter() - t1) * 1e3
    if timing is not None:
        timing.update(ms, wall_ms=(time.perf_counter() - t0) * 1e3, power=ptau.power)


def _coef_values(vals):
    """[n, 4] uint64 standard-form values -> [n, 32] uint8 of v * 2^512 mod r: one big-integer product per DISTINCT value (the values
    below 2^64 and the wider ones are told apart first: the first are sorted as machine words)."""
    v = np.ascontiguousarray(vals, dtype="<u8").reshape(-1, 4)
    out = np.zeros((v.shape[0], 32), dtype=np.uint8)
    small = ~v[:, 1:].any(axis=1)
    for mask, keys in ((small, v[small, 0]), (~small, np.ascontiguousarray(v[~small]).view("V32").reshape(-1))):
        if keys.size:
            uniq, inverse = np.unique(keys, return_inverse=True)
            table = b"".join((int.from_bytes(u.tobytes(), "little") * _COEF_SHIFT % R).to_bytes(32, "little") for u in uniq)
            out[mask] = np.frombuffer(table, dtype=np.uint8).reshape(-1, 32)[inverse.reshape(-1)]
    return out


_COEF_DTYPE = np.dtype([("matrix", "<u4"), ("row", "<u4"), ("signal", "<u4"), ("value", np.uint8, (32,))])


def _setup_records(r1cs):
    """Section 4 of the key of a circuit: the A and B terms of every constraint in file order (A's before B's per constraint), then the
    rows nConstraints + s = (signal s, 1) of A for s = 0 .. nPublic -> a [nCoefs] array of 44-byte records."""
    counts = [np.diff(m[0].astype(np.int64)) for m in (r1cs.a, r1cs.b)]
    rows = [np.repeat(np.arange(r1cs.nConstraints, dtype=np.int64), c) for c in counts]
    na, nb, npub = rows[0].size, rows[1].size, r1cs.nPublic + 1
    order = np.argsort(np.concatenate([2 * rows[0], 2 * rows[1] + 1]), kind="stable")
    rec = np.zeros(na + nb + npub, dtype=_COEF_DTYPE)
    assert rec.dtype.itemsize == COEF_BYTES
    head = rec[:na + nb]
    head["matrix"] = np.concatenate([np.zeros(na, dtype=np.uint32), np.ones(nb, dtype=np.uint32)])[order]
    head["row"] = np.concatenate(rows)[order]
    head["signal"] = np.concatenate([r1cs.a[1], r1cs.b[1]])[order]
    head["value"] = _coef_values(np.concatenate([r1cs.a[2].reshape(-1, 4), r1cs.b[2].reshape(-1, 4)]))[order]
    tail = rec[na + nb:]
    tail["row"] = r1cs.nConstraints + np.arange(npub)
    tail["signal"] = np.arange(npub)
    tail["value"] = np.frombuffer(_COEF_SHIFT.to_bytes(32, "little"), dtype=np.uint8)
    return rec


def _setup_domain_bits(r1cs):
    return max(1, (r1cs.nConstraints + r1cs.nPublic).bit_length())      # ceil(log2(nConstraints + nPublic + 1)), at least 1


def _setup_system(r1cs, k):
    """The circuit's constraints with the rows nConstraints + s = (signal s, 1) appended to A, as a domain R1CS over 2^k."""
    npub = r1cs.nPublic + 1
    rp_a = np.concatenate([r1cs.a[0].astype(np.int64), int(r1cs.a[0][-1]) + np.arange(1, npub + 1)]).astype(np.uint32)
    col_a = np.concatenate([r1cs.a[1], np.arange(npub, dtype=np.uint32)])
    one = np.zeros((npub, 4), dtype=np.uint64)
    one[:, 0] = 1
    val_a = np.concatenate([r1cs.a[2].reshape(-1, 4), one])
    pad = lambda m: (np.concatenate([m[0], np.full(npub, m[0][-1], dtype=np.uint32)]), m[1], m[2])      # noqa: E731
    return DeviceDomainR1CS(k, (rp_a, col_a, val_a), pad(r1cs.b), pad(r1cs.c), r1cs.nVars)


def CheckWtns(r1cs_path, wtns_path, cap=16):
    """What `snarkjs wtns check` answers, on the device: which constraints of circuit.r1cs does witness.wtns break?  ->
    r1csqap.WitnessReport (report.explain(i, ReadR1cs(r1cs_path)) spells a reported row out).  The system is the one SetupFromPtau
    builds the key on; its appended rows hold no B and no C and are satisfied by every witness, so a reported row is a constraint of
    the file."""
    r1cs, w = ReadR1cs(r1cs_path), ReadWtns(wtns_path)
    if w.shape[0] != r1cs.nWires:
        raise ValueError("%s holds %d values, %s has nWires = %d" % (wtns_path, w.shape[0], r1cs_path, r1cs.nWires))
    return _setup_system(r1cs, _setup_domain_bits(r1cs)).CheckWitness(np.ascontiguousarray(w, dtype=np.uint64), cap)


def SetupFromPtau(r1cs_path, ptau_path, zkey_path, timing=None, prepared=False):
    """What `snarkjs groth16 setup` does, on the device: circuit.r1cs + a powers-of-tau file -> circuit.zkey with delta = 1 (apply
    ContributeDelta before using the key: with delta = 1 proofs can be forged).  The Lagrange bases of the domain are inverse transforms of
    the transcript's sections in the group (gs_g1_lagrange / gs_g2_lagrange; the prepared sections 12 - 15 of a transcript are not read),
    A, B1, B2, C and IC column sums of the circuit's matrices over them (gs_r1cs_colsum_g1 / _g2), H the odd half of the transform of
    twice the size.  The arrays leave the device straight into the memory-mapped output file.
    prepared=True reads the bases from the transcript's prepared sections instead (ReadPtauPrepared; PreparePtau writes them): L, L2, La,
    Lb are level k of sections 12, 13, 14, 15 and H the odd entries of level k + 1 of section 12, no transform runs and
    timing["transforms_ms"] stays 0; a file without usable prepared sections is a ValueError before the device is touched.  The prepared
    sections are TRUSTED INPUT: nothing here checks that they are the Lagrange form of sections 2 - 5 -- run VerifyPtauPrepared on the
    transcript before the setup, or VerifyZkey on the key after it.
    -> (groth16.DevicePk, DeviceZkeyR1CS, groth16.Vk) of the key just written, built from the resident arrays.
    `timing`: a dict that receives the device milliseconds of the phases (transforms, column sums), the wall milliseconds of the
    downloads and file writing, and the largest gs_memory_query library_bytes seen between two device calls."""
    import time
    r1cs, ptau = ReadR1cs(r1cs_path), (ReadPtauPrepared if prepared else ReadPtau)(ptau_path)
    k = _setup_domain_bits(r1cs)
    m, nvars, npub = 1 << k, r1cs.nVars, r1cs.nPublic + 1
    if ptau.power < k:
        raise ValueError("%s: section %s: power = %d, but %d constraints and %d public signals need a domain of 2^%d points"
                         % (ptau_path, _PTAU_NAMES[1], ptau.power, r1cs.nConstraints, r1cs.nPublic, k))
    if npub > nvars:
        raise ValueError("%s: section %s: nPublic + 1 = %d exceeds nWires = %d" % (r1cs_path, _R1CS_NAMES[1], npub, nvars))
    capi.init()
    ms = {"transforms_ms": 0.0, "colsums_ms": 0.0, "write_ms": 0.0, "library_bytes_max": 0}

    def timed(phase, fn, *args, **kw):
        out = fn(*args, **kw)
        ms[phase] += capi.last_timing()["total_ms"]
        ms["library_bytes_max"] = max(ms["library_bytes_max"], capi.memory_query()["library_bytes"])
        return out

    system = _setup_system(r1cs, k)
    if prepared:
        L = capi.g1_upload_affine_mont(ptau.level(12, k))
        H = capi.g1_upload_affine_mont(np.ascontiguousarray(np.asarray(ptau.level(12, k + 1)).reshape(-1, G1_BYTES)[1::2]).reshape(-1))
        L2 = capi.g2_upload_affine_mont(ptau.level(13, k))
        La, Lb = capi.g1_upload_affine_mont(ptau.level(14, k)), capi.g1_upload_affine_mont(ptau.level(15, k))
    else:
        tau1 = capi.g1_upload_affine_mont(ptau.tauG1[:min(2 * m, (2 << ptau.power) - 1) * G1_BYTES])
        L = timed("transforms_ms", capi.g1_lagrange, tau1, k)
        H = timed("transforms_ms", capi.g1_lagrange, tau1, k, odd_half=True)
        tau1 = None
        L2 = timed("transforms_ms", capi.g2_lagrange, capi.g2_upload_affine_mont(ptau.tauG2[:m * G2_BYTES]), k)
        La = timed("transforms_ms", capi.g1_lagrange, capi.g1_upload_affine_mont(ptau.alphaTauG1[:m * G1_BYTES]), k)
        Lb = timed("transforms_ms", capi.g1_lagrange, capi.g1_upload_affine_mont(ptau.betaTauG1[:m * G1_BYTES]), k)
    A = timed("colsums_ms", capi.r1cs_colsum, system, L, None, None)
    B1 = timed("colsums_ms", capi.r1cs_colsum, system, None, L, None)
    B2 = timed("colsums_ms", capi.r1cs_colsum, system, None, L2, None, g2=True)
    K = timed("colsums_ms", capi.r1cs_colsum, system, Lb, La, L)
    L = L2 = La = Lb = system = None
    # the file: header and records from the host, the arrays from the device into their sections
    t0 = time.perf_counter()
    rec = _setup_records(r1cs)
    alpha1, beta1, beta2 = bytes(ptau.alphaTauG1[:G1_BYTES]), bytes(ptau.betaTauG1[:G1_BYTES]), bytes(ptau.betaG2)
    head = struct.pack("<I", 32) + Q.to_bytes(32, "little") + struct.pack("<I", 32) + R.to_bytes(32, "little") + struct.pack("<III", nvars, r1cs.nPublic, m)
    head += alpha1 + beta1 + beta2 + G2ToZkey(G2_GEN) + G1ToZkey(G1_GEN) + G2ToZkey(G2_GEN)
    sizes = {1: 4, 2: len(head), 3: npub * G1_BYTES, 4: 4 + rec.size * COEF_BYTES, 5: nvars * G1_BYTES, 6: nvars * G1_BYTES, 7: nvars * G2_BYTES,
             8: (nvars - npub) * G1_BYTES, 9: m * G1_BYTES}
    offs, pos = {}, 12
    for sid in range(1, 10):
        offs[sid] = pos + 12
        pos += 12 + sizes[sid]
    with open(zkey_path, "wb") as f:
        f.truncate(pos)
    out = np.memmap(zkey_path, dtype=np.uint8, mode="r+")
    put = lambda at, b: out.__setitem__(slice(at, at + len(b)), np.frombuffer(b, dtype=np.uint8))      # noqa: E731
    put(0, b"zkey" + struct.pack("<II", 1, 9))
    for sid in range(1, 10):
        put(offs[sid] - 12, struct.pack("<IQ", sid, sizes[sid]))
    put(offs[1], struct.pack("<I", 1))
    put(offs[2], head)
    put(offs[4], struct.pack("<I", rec.size))
    section = lambda sid, skip=0: out[offs[sid] + skip:offs[sid] + sizes[sid]]      # noqa: E731
    section(4, 4)[:] = rec.view(np.uint8).reshape(-1)
    capi.g1_download_affine_mont(A, section(5))
    capi.g1_download_affine_mont(B1, section(6))
    capi.g2_download_affine_mont(B2, section(7))
    capi.g1_download_affine_mont(H, section(9))
    capi.g1_download_affine_mont(K, section(3), n=npub)
    kbytes = capi.g1_download_affine_mont(K)                       # C = K without the public signals; the resident C has infinities there
    section(8)[:] = kbytes[npub * G1_BYTES:]
    out.flush()
    ms["write_ms"] = (time.perf_counter() - t0) * 1e3
    kbytes[:npub * G1_BYTES] = 0
    ic = [G1FromZkey(row) for row in np.asarray(section(3)).reshape(-1, G1_BYTES)]
    a1, b1p, b2p = G1FromZkey(alpha1), G1FromZkey(beta1), G2FromZkey(beta2)
    key = groth16.device_pk_domain_from_handles(A, B1, B2, capi.g1_upload_affine_mont(kbytes), H, a1, b1p, G1_GEN, b2p, G2_GEN, k, nvars, r1cs.nPublic)
    prod = DeviceZkeyR1CS(k, nvars, rec.view(np.uint8).reshape(-1))
    del out
    if timing is not None:
        timing.update(ms, log2_domain=k, nVars=nvars, nCoefs=int(rec.size))
    return key, prod, groth16.Vk(IC=ic, G1_Alpha=a1, G2_Beta=b2p, G2_Gamma=G2_GEN, G2_Delta=G2_GEN)


def ContributeDelta(zkey_in, zkey_out, delta):
    """One phase-2 contribution with the secret `delta`: C and H are multiplied by 1 / delta (gs_g1_scale), delta1 and delta2 by delta, and
    everything else -- every other section, section 10 if the file has one, unknown sections -- is copied byte for byte.
    NO CONTRIBUTION TRANSCRIPT IS WRITTEN: `snarkjs zkey verify` checks the chain of contributions recorded in section 10, and producing that
    record (the challenge hashes and the proof of knowledge of delta) is out of scope here; the key proves and verifies, it does not pass
    `zkey verify`.  VerifyZkey below is the check this module offers in its place: the key against its circuit and transcript."""
    delta = int(delta) % R
    if delta == 0:
        raise ValueError("delta must not be 0 mod r")
    ReadZkey(zkey_in)                                                  # validates the layout
    data, sec = _read_sections(zkey_in, b"zkey", 1, _ZKEY_NAMES, (2, 8, 9))
    capi.init()
    shutil.copyfile(zkey_in, zkey_out)
    out = np.memmap(zkey_out, dtype=np.uint8, mode="r+")
    inv = pow(delta, -1, R)
    for sid in (8, 9):
        off, length = sec[sid]
        if length:
            capi.g1_download_affine_mont(capi.g1_scale(capi.g1_upload_affine_mont(data[off:off + length]), inv), out[off:off + length])
    d1 = sec[2][0] + sec[2][1] - G2_BYTES - G1_BYTES                  # delta1 | delta2 end the header
    capi.g1_download_affine_mont(capi.g1_scale(capi.g1_upload_affine_mont(data[d1:d1 + G1_BYTES]), delta), out[d1:d1 + G1_BYTES])
    d2 = capi.g2_upload_affine_mont(data[d1 + G1_BYTES:d1 + G1_BYTES + G2_BYTES])
    p = capi.msm(d2, capi.ints_to_u64([delta]), g2=True)
    out[d1 + G1_BYTES:d1 + G1_BYTES + G2_BYTES] = np.frombuffer(G2ToZkey(G2_INF if p is None else (p[0], p[1], (1, 0))), dtype=np.uint8)
    out.flush()
    del out


# ---- checking a key and a transcript ---------------------------------------------------------------------------------------------
class CheckReport:
    """The outcome of VerifyZkey / VerifyPtau: truthy only when every check passed.  `checks`: [(name, ok, lhs, rhs)] in the order they
    were made, the two points of a check as affine int tuples (None = infinity; None, None for the host-side checks; the coefs checks
    carry the number of differing rows as lhs, and the membership checks of membership=True the number of points outside the order-r
    subgroup as lhs and the smallest index of one (None: there is none) as rhs); `failed`: the names of the checks that did not pass;
    `points[name]` = (lhs, rhs)."""

    def __init__(self, checks, seed):
        self.checks, self.seed = list(checks), seed
        self.failed = [name for name, ok, _, _ in self.checks if not ok]
        self.points = {name: (lhs, rhs) for name, _, lhs, rhs in self.checks}

    def __bool__(self):
        return not self.failed

    def __repr__(self):
        return "%s(%s)" % (type(self).__name__, "all %d checks passed" % len(self.checks) if self else "FAILED: " + ", ".join(self.failed))


class ZkeyReport(CheckReport):
    pass


class PtauReport(CheckReport):
    pass


def _membership_check(name, points, off=0, n=None):
    """(name, ok, nbad, first_bad) over a resident G2 array (gs_g2_subgroup_check), and the device milliseconds it took."""
    nbad, first = capi.g2_subgroup_check(points, off, n)
    return (name, nbad == 0, nbad, first), capi.last_timing()["total_ms"]


def _challenge(seed):
    """A challenge in 1 .. r - 1: from `seed` (tests: reproducible) or from the operating system's randomness."""
    if seed is None:
        import secrets
        return 1 + secrets.randbelow(R - 1)
    import random
    return random.Random(seed).randrange(1, R)


def VerifyZkey(r1cs_path, ptau_path, zkey_path, seed=None, timing=None, membership=False):
    """Is the key at `zkey_path` the Groth16 key of the circuit at `r1cs_path` over the transcript at `ptau_path`, with C and H scaled by
    the delta of its header?  -> ZkeyReport.  Host side: the counts of the three files against each other (a mismatch is a ValueError that
    names file and section, raised before the device is touched), then the checks `header` (alfa1 / beta1 / beta2 against the transcript,
    gamma2 = the generator) and `delta` (delta1 finite, e(delta1, G2) = e(G1, delta2)).  Device side (gs_groth16_key_check): coefs A,
    coefs B, A, B1, B2, IC, C, H -- random linear combinations of every section against combinations of transcript points whose scalars
    come from the circuit, for a challenge drawn after the files are opened (`seed`: a fixed one, for tests).  A wrong key passes with
    probability at most max(nVars, 2 domainSize) / r.  What this proves: the key's relation to THIS circuit and THIS transcript.  What it
    does not: who contributed to either (no contribution chain is read or checked), or that the transcript is sound -- see VerifyPtau.
    `timing`: a dict that receives the device milliseconds of the check (gs_last_timing) and the wall milliseconds of the whole call.
    membership=True appends `tauG2 membership` (the domainSize transcript points used) and `B2 membership` (the key's nVars points): every
    G2 point is tested for the order-r subgroup (gs_g2_subgroup_check, on the arrays already uploaded), (name, ok, points outside, smallest
    index or None).  The uploads test the curve equation only and the twist's cofactor has the factor 10069, so the B2 check alone lets a
    point off the subgroup by an element of that order through about once in 10069 challenges: files of unknown origin need
    membership=True.  It is not the default because the default report is a fixed list that callers compare against, and files one wrote
    oneself do not need it.  `timing` then also receives `membership_ms`."""
    import time
    t0 = time.perf_counter()
    r1cs, ptau, z = ReadR1cs(r1cs_path), ReadPtau(ptau_path), ReadZkey(zkey_path)
    k = _setup_domain_bits(r1cs)
    m = 1 << k
    for name, have, want in (("nVars", z.nVars, r1cs.nVars), ("nPublic", z.nPublic, r1cs.nPublic), ("domainSize", z.domainSize, m)):
        if have != want:
            raise ValueError("%s: section %s: %s = %d, but the circuit %s (section %s) needs %d"
                             % (zkey_path, _ZKEY_NAMES[2], name, have, r1cs_path, _R1CS_NAMES[1], want))
    if ptau.power < k:
        raise ValueError("%s: section %s: power = %d, but the key's domain of 2^%d points needs a transcript of at least that power"
                         % (ptau_path, _PTAU_NAMES[1], ptau.power, k))
    s = _challenge(seed)
    header = (z.alfa1 == G1FromZkey(ptau.alphaTauG1[:G1_BYTES]) and z.beta1 == G1FromZkey(ptau.betaTauG1[:G1_BYTES])
              and _g2(z.beta2) == _g2(G2FromZkey(ptau.betaG2)) and _g2(z.gamma2) == G2_GEN)
    from . import bn128
    neg = lambda p: (p[0], (Q - p[1]) % Q, p[2])      # noqa: E731
    delta = z.delta1[2] % Q != 0 and _g2(z.delta2)[2] != (0, 0) and bn128.PairingCheck([z.delta1, neg(G1_GEN)], [G2_GEN, _g2(z.delta2)])
    checks = [("header", bool(header), None, None), ("delta", bool(delta), None, None)]
    capi.init()
    up1, up2 = capi.g1_upload_affine_mont, capi.g2_upload_affine_mont
    tau1 = up1(ptau.tauG1[:min(2 * m, (2 << ptau.power) - 1) * G1_BYTES])
    tau2, b2 = up2(ptau.tauG2[:m * G2_BYTES]), up2(z.B2)
    checks += capi.groth16_key_check(up1(z.A), up1(z.B1), b2, up1(z.IC), up1(z.C), up1(z.H), DeviceZkeyR1CS(k, z.nVars, z.coefs),
                                     _setup_system(r1cs, k), tau1, tau2, up1(ptau.alphaTauG1[:m * G1_BYTES]),
                                     up1(ptau.betaTauG1[:m * G1_BYTES]), _g2(z.delta2), k, z.nPublic, s)
    device = capi.last_timing()
    if membership:
        (c1, ms1), (c2, ms2) = _membership_check("tauG2 membership", tau2), _membership_check("B2 membership", b2)
        checks += [c1, c2]
        device["membership_ms"] = ms1 + ms2
    if timing is not None:
        timing.update(device, wall_ms=(time.perf_counter() - t0) * 1e3, log2_domain=k, nVars=z.nVars)
    return ZkeyReport(checks, s)


def VerifyPtau(ptau_path, power=None, seed=None, timing=None, membership=False):
    """Is the transcript at `ptau_path` consistent with itself over its first 2^power powers (default: all it holds)?  -> PtauReport of
    gs_ptau_check's checks: tauG1[0] and tauG2[0] are the generators, both sections are the powers of ONE tau, alphaTauG1 and betaTauG1 are
    geometric with that ratio, betaG2 carries betaTauG1[0]'s scalar.  What this does not prove: who contributed -- the contribution chain of
    a ceremony (challenge hashes, proofs of knowledge) is out of scope.
    membership=True appends `tauG2 membership`: each of the 2^power tauG2 points checked is tested for the order-r subgroup
    (gs_g2_subgroup_check, on the array already uploaded), (name, ok, points outside, smallest index or None).  The uploads test the curve
    equation only and the twist's cofactor has the factor 10069, so the tauG2 check alone lets tau^j G2 + S with S of that order through
    about once in 10069 challenges: a file of unknown origin needs membership=True.  It is not the default because the default report is
    a fixed list that callers compare against, and a transcript one wrote oneself does not need it.  `timing` then also receives
    `membership_ms`, the device milliseconds of that test."""
    import time
    t0 = time.perf_counter()
    ptau = ReadPtau(ptau_path)
    power = ptau.power if power is None else int(power)
    if not 1 <= power <= ptau.power:
        raise ValueError("%s: section %s: power = %d, so 2^%d powers cannot be checked (1 <= power <= %d)"
                         % (ptau_path, _PTAU_NAMES[1], ptau.power, power, ptau.power))
    s = _challenge(seed)
    n = 1 << power
    capi.init()
    up1 = capi.g1_upload_affine_mont
    tau2 = capi.g2_upload_affine_mont(ptau.tauG2[:n * G2_BYTES])
    checks = capi.ptau_check(up1(ptau.tauG1[:(2 * n - 1) * G1_BYTES]), tau2,
                             up1(ptau.alphaTauG1[:n * G1_BYTES]), up1(ptau.betaTauG1[:n * G1_BYTES]), _g2(G2FromZkey(ptau.betaG2)), power, s)
    device = capi.last_timing()
    if membership:
        check, device["membership_ms"] = _membership_check("tauG2 membership", tau2)
        checks.append(check)
    if timing is not None:
        timing.update(device, wall_ms=(time.perf_counter() - t0) * 1e3, power=power)
    return PtauReport(checks, s)


PTAU_PREPARED_CHECKS = ("tauG1 Lagrange", "tauG2 Lagrange", "alphaTauG1 Lagrange", "betaTauG1 Lagrange")


def VerifyPtauPrepared(ptau_path, power=None, seed=None, timing=None, membership=False):
    """Are the prepared sections 12 - 15 of the transcript at `ptau_path` the Lagrange bases of its sections 2 - 5?  -> PtauReport of four
    checks named after the sections (gs_g*_lagrange_levels_check: per section one random linear combination of all its levels against one
    combination of the section's powers whose scalars come from scalar transforms; no transform runs in the group).  `power` (default: the
    file's) limits the check to the levels 0 .. power, a prefix of each section -- 0 .. power + 1 for tauG1, whose level power + 1 is the
    padded one (2^(power+1) - 1 points and an infinity) only at the file's own power.  At most power 24: one sum takes the 2^(power+2) - 1
    points of tauG1's levels and a sum holds 2^26 - 1 terms.  A wrong section passes with probability at most 2^(power+2) / r (G2: for
    differences in the order-r subgroup, see include/gosnark_hip.h).  What this does not prove: that sections 2 - 5 themselves are sound
    -- see VerifyPtau.
    `timing`: a dict that receives the device milliseconds of the four checks and the wall milliseconds of the whole call.
    membership=True appends `tauG2 Lagrange membership`: each of the 2^(power+1) - 1 level points of section 13 checked is tested for the
    order-r subgroup (gs_g2_subgroup_check, on the array already uploaded), (name, ok, points outside, smallest index or None) -- what
    closes the G2 caveat above, and what a file of unknown origin needs.  It is not the default because the default report is a fixed list
    that callers compare against, and a file one prepared oneself does not need it.  `timing` then also receives `membership_ms`."""
    import time
    t0 = time.perf_counter()
    ptau = ReadPtauPrepared(ptau_path)
    power = ptau.power if power is None else int(power)
    if not 0 <= power <= min(ptau.power, 24):
        raise ValueError("%s: section %s: power = %d, so the levels 0 .. %d cannot be checked (0 <= power <= %d; 24 at most: tauG1's levels "
                         "0 .. power + 1 are one sum of 2^(power+2) - 1 terms)" % (ptau_path, _PTAU_NAMES[1], ptau.power, power, min(ptau.power, 24)))
    s = _challenge(seed)
    capi.init()
    source = {2: ptau.tauG1, 3: ptau.tauG2, 4: ptau.alphaTauG1, 5: ptau.betaTauG1}
    checks, device_ms, member = [], 0.0, None
    for sid, name in zip(_PTAU_PREPARED, PTAU_PREPARED_CHECKS):
        src_id, extra, size = _PTAU_LEVELS[sid]
        g2 = size == G2_BYTES
        up = capi.g2_upload_affine_mont if g2 else capi.g1_upload_affine_mont
        hi = power + extra
        pw = up(source[src_id][:(1 << hi) * size])                     # tauG1 at the file's own power: 2^hi - 1 points, the padded level
        lv = up(ptau.lagrange[sid][:((2 << hi) - 1) * size])
        checks.append((capi.g2_lagrange_levels_check if g2 else capi.g1_lagrange_levels_check)(pw, lv, hi, s, name))
        device_ms += capi.last_timing()["total_ms"]
        if membership and g2:
            member = _membership_check(name + " membership", lv)
        pw.free()
        lv.free()
    if member is not None:
        checks.append(member[0])
    if timing is not None:
        timing.update(device_ms=device_ms, wall_ms=(time.perf_counter() - t0) * 1e3, power=power)
        if member is not None:
            timing["membership_ms"] = member[1]
    return PtauReport(checks, s)
