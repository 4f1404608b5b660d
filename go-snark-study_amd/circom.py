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
Values are decimal strings; ["0", "1", "0"] (Z = 0) is the point at infinity.  The newer .zkey / .wtns binaries are not read here."""
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
