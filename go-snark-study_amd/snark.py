"""Mirror of the reference's Pinocchio prover interface (snark.go:16-26, 59-69, 254-289)."""
import ctypes

import numpy as np

from . import _scheme, capi
from ._scheme import GS_ERR_BUSY   # noqa: F401
from .groth16 import Circuit, R   # noqa: F401


class Pk:
    """snark.Pk (snark.go:16-26)."""

    def __init__(self, G1T, A, B, C, Kp, Ap, Bp, Cp, Z):
        self.G1T, self.A, self.B, self.C = G1T, A, B, C
        self.Kp, self.Ap, self.Bp, self.Cp, self.Z = Kp, Ap, Bp, Cp, Z
        self._dev = None


class Proof:
    """snark.Proof (snark.go:59-69)."""
    FIELDS = ("PiA", "PiAp", "PiB", "PiBp", "PiC", "PiCp", "PiH", "PiKp")

    def __init__(self, **kw):
        for k in self.FIELDS:
            setattr(self, k, kw[k])


class Vk:
    """snark.Vk (snark.go:28-38): affine Jacobian tuples."""
    FIELDS = ("Vka", "Vkb", "Vkc", "G1Kbg", "G2Kbg", "G2Kg", "Vkz")

    def __init__(self, IC, **kw):
        self.IC = IC
        for k in self.FIELDS:
            setattr(self, k, kw[k])


class DevicePk:
    def __init__(self, handle, nvars, npublic):
        self.h, self.handle, self.nvars, self.npublic = handle.h, handle, nvars, npublic


# G1TEval: evaluation-basis copy of G1T; G1TQuot: quotient-basis array Q_m = sum_{d <= m} g_d G1T[m - d], g = 1 / rev(Z)
PK_ARRAYS = {"A": 0, "Ap": 1, "B": 2, "Bp": 3, "C": 4, "Cp": 5, "Kp": 6, "G1T": 7, "G1TEval": 9, "G1TQuot": 10}


def device_pk_from_handles(A, Ap, B, Bp, C, Cp, Kp, G1T, z_u64, nvars, npublic):
    """Assemble a DevicePk from already-resident base arrays (gs_pinocchio_pk_create; B in G2, the others in G1)."""
    capi.init()
    z = np.ascontiguousarray(z_u64, dtype=np.uint64).reshape(-1, 4)
    cell = capi.HandleCell()
    capi.call("gs_pinocchio_pk_create", *map(capi.raw, (A, Ap, B, Bp, C, Cp, Kp, G1T)), capi.ptr64(z), z.shape[0], nvars, npublic, cell.ref)
    return DevicePk(cell.result(), nvars, npublic)


def UploadPk(pk, circuit):
    if pk._dev is not None:
        return pk._dev
    capi.init()
    g1 = {k: capi.g1_upload(capi.g1_points_to_u64(getattr(pk, k))) for k in ("A", "Ap", "Bp", "C", "Cp", "Kp", "G1T")}
    b2 = capi.g2_upload(capi.g2_points_to_u64(pk.B))
    pk._dev = device_pk_from_handles(B=b2, z_u64=capi.ints_to_u64([x % R for x in pk.Z]), nvars=circuit.NVars, npublic=circuit.NPublic, **g1)
    return pk._dev


def _proof_from_words(out, inf):
    v = capi.u64_to_ints(out)
    res, pos = {}, 0
    for i, k in enumerate(Proof.FIELDS):
        if k == "PiB":
            res[k] = ((0, 0), (0, 0), (0, 0)) if inf[i] else ((v[pos], v[pos + 1]), (v[pos + 2], v[pos + 3]), (1, 0))
            pos += 4
        else:
            res[k] = (0, 0, 0) if inf[i] else (v[pos], v[pos + 1], 1)
            pos += 2
    return Proof(**res)


_S = _scheme.Scheme(prefix="gs_pinocchio_", proof=(72, 8), partials=(72, 8), has_rs=False, decode=_proof_from_words, arrays=PK_ARRAYS,
                    g2_array=2, h_array=7, eval_array=9, quot_array=10, DevicePk=DevicePk, UploadPk=UploadPk, negative_note="")


def GenerateProofs(circuit, pk, w, px):
    """snark.GenerateProofs(circuit, pk, w, px) (snark.go:254-289).  Deterministic.  Round 6 (as go/snarkhip.GenerateProofs): a host-buffer
    ticket collected at once (gs_pinocchio_prove_host_begin + gs_pinocchio_prove_end); the blocking entry point when all slots are taken."""
    return _scheme.generate(_S, circuit, pk, w, px)


def GenerateProofsFromWitness(circuit, pk, dev_r1cs, w):
    """go/snarkhip.GenerateProofsFromWitness: witness -> proof against the circuit's resident sparse R1CS, a host-buffer ticket collected at once."""
    return _scheme.generate_from_witness(_S, circuit, pk, dev_r1cs, w)


def GenerateProofsChecked(circuit, pk, dev_r1cs, w, check_r1cs=None):
    """go/snarkhip.GenerateProofsChecked: as groth16.GenerateProofsChecked -- a witness that breaks a constraint raises
    r1csqap.WitnessError before anything is proved."""
    return _scheme.generate_checked(_S, circuit, pk, dev_r1cs, w, check_r1cs=check_r1cs)


def GenerateProofsFromInputs(circuit, pk, dev_r1cs, plan, inputs):
    """As groth16.GenerateProofsFromInputs: the witness is solved on the device from the plan's input values, checked, then proved."""
    return _scheme.generate_from_inputs(_S, circuit, pk, dev_r1cs, plan, inputs)


class Prover(_scheme.Prover):
    """The streaming drop-in (go/snarkhip.Prover; see groth16.Prover): Submit(w[, px]) / Collect(), three proofs in flight."""
    scheme = _S

    def Submit(self, w, px=None):
        self._submit(w, px)


def NewProver(circuit, pk, dev_r1cs=None):
    return Prover(circuit, pk, dev_r1cs)


def prove_resident(dev_pk, w_handle, px_handle):
    """snark.GenerateProofs with the key, w and px already resident in HBM (gs_pinocchio_prove_resident)."""
    return _scheme.prove(_S, "prove_resident", dev_pk, w_handle, px_handle)


def prove_from_witness(dev_pk, dev_r1cs, w_handle):
    """Sparse R1CS + resident witness -> proof, H(x) straight from the constraint values (gs_pinocchio_prove_witness): no px."""
    return _scheme.prove(_S, "prove_witness", dev_pk, dev_r1cs, w_handle)


def prove_witness_begin(dev_pk, dev_r1cs, w_handle):
    """Enqueue one witness -> proof (gs_pinocchio_prove_witness_begin) -> ticket for prove_end."""
    return _scheme.begin(_S, "prove_witness_begin", dev_pk, dev_r1cs, w_handle)


def prove_host_begin(dev_pk, w, px):
    """snark.GenerateProofs' own call shape, pipelined (gs_pinocchio_prove_host_begin): w and px in host memory -> ticket for prove_end."""
    return _scheme.prove_host_begin(_S, dev_pk, w, px)


def prove_witness_host_begin(dev_pk, dev_r1cs, w):
    """A fresh host witness against the resident sparse R1CS (gs_pinocchio_prove_witness_host_begin) -> ticket for prove_end."""
    return _scheme.prove_witness_host_begin(_S, dev_pk, dev_r1cs, w)


def prove_from_witness_host(dev_pk, dev_r1cs, w):
    """Blocking: host witness -> proof (gs_pinocchio_prove_witness_host)."""
    return _scheme.prove_from_witness_host(_S, dev_pk, dev_r1cs, w)


def SetEvalBasis(dev_pk, points):
    """Attach an evaluation-basis copy of G1T (n Jacobian int triples) to a resident key: gs_pinocchio_pk_set_eval."""
    _scheme.set_basis(_S, "eval", dev_pk, capi.g1_points_to_u64(points))


def SetQuotBasis(dev_pk, points):
    """Attach a quotient-basis array (len(G1T) Jacobian int triples, PK_ARRAYS) to a resident key: gs_pinocchio_pk_set_quot.
    points = None detaches it: the key divides px by Z again."""
    _scheme.set_basis(_S, "quot", dev_pk, None if points is None else capi.g1_points_to_u64(points))


def DeriveQuotBasis(dev_pk):
    """Compute the quotient-basis array of a resident key from its G1T and Z (gs_pinocchio_pk_derive_quot) and attach it."""
    _scheme.derive_basis(_S, "quot", dev_pk)


def DeriveEvalBasis(dev_pk, n):
    """Compute the evaluation-basis array of a resident key from its G1T alone (gs_pinocchio_pk_derive_eval) and attach it as
    SetEvalBasis would.  n = the number of constraints."""
    _scheme.derive_basis(_S, "eval", dev_pk, int(n))


def prove_begin(dev_pk, w_handle, px_handle):
    """Enqueue one Pinocchio proof (gs_pinocchio_prove_begin) -> ticket.  Up to three operations may be outstanding."""
    return _scheme.begin(_S, "prove_begin", dev_pk, w_handle, px_handle)


def prove_end(ticket):
    """Collect the proof of a ticket (gs_pinocchio_prove_end)."""
    return _scheme.prove_end(_S, ticket)


# ---- several GPUs (SURVEY 8e applied to snark.go:254-289): a proof is the sum of the ranks' eight partial points ----------------
def ShardPk(dev_pk, shard_index, shard_count, target_device=None):
    """Slice `shard_index` of `shard_count` of a resident full key (gs_pinocchio_pk_shard), on logical device `target_device` if given
    (gs_pinocchio_pk_shard_to).  -> DevicePk holding 1 / shard_count of every array."""
    return _scheme.shard(_S, dev_pk, shard_index, shard_count, target_device)


def _sums(out, inf):
    return np.array(out, dtype=np.uint64), [int(x) for x in inf]


def prove_partials(dev_pk, w_handle, px_handle, shard_index, shard_count):
    """The eight sums over shard `shard_index` of the term ranges (gs_pinocchio_prove_partials) -> (72 words, 8 infinity flags),
    the layout of a proof; add the ranks' records with combine()."""
    return _sums(*_scheme.partials(_S, "prove_partials", dev_pk, w_handle, px_handle, shard_index, shard_count))


def witness_values(dev_pk, dev_r1cs, w_handle, hv_handle=None):
    """The proof owner's polynomial stage (gs_pinocchio_witness_values) -> (handle of the n values H(n+1..2n), violated)."""
    return _scheme.witness_values(_S, dev_pk, dev_r1cs, w_handle, hv_handle)


def prove_partials_values(dev_pk, w_handle, hv_slice, shard_index, shard_count):
    """gs_pinocchio_prove_partials_values: the eight sums with PiH over this rank's slice of H's values."""
    return _sums(*_scheme.partials(_S, "prove_partials_values", dev_pk, w_handle, hv_slice, shard_index, shard_count))


def combine(records):
    """gs_pinocchio_combine: [(72 words, 8 flags)] of every rank -> Proof."""
    n = len(records)
    sums = np.ascontiguousarray(np.concatenate([np.asarray(r[0], dtype=np.uint64).reshape(72) for r in records]))
    fl = (ctypes.c_int * (8 * n))(*[int(x) for r in records for x in r[1]])
    return _scheme.call_proof(_S, "combine", capi.ptr64(sums), fl, n)


def prove_multi(dev_pks, w_handles, third_handles, values=False):
    """One proof over len(dev_pks) logical devices of THIS process (gs_pinocchio_prove_multi, or _multi_values when `third_handles`
    are the devices' slices of H's values instead of replicas of px).  -> (Proof, used_rccl)."""
    return _scheme.prove_multi(_S, "prove_multi_values" if values else "prove_multi", dev_pks, w_handles, third_handles)


def prove_sharded_rccl(dev_pk, w_handle, third_handle, values=False):
    """One process per GPU, records gathered INSIDE the library over the communicator of capi.comm_init_rank
    (gs_pinocchio_prove_sharded / _sharded_values).  Every rank returns the same Proof."""
    return _scheme.prove(_S, "prove_sharded_values" if values else "prove_sharded", dev_pk, w_handle, third_handle)


def prove_batch(pk_of_device, w_handles, px_handles):
    """A batch of independent proofs round-robined over logical devices (gs_pinocchio_prove_batch): proof i runs where w_handles[i]
    lives, with pk_of_device[that device] (None for unused devices).  No collective."""
    return _scheme.prove_batch(_S, pk_of_device, w_handles, px_handles)


def GenerateTrustedSetupSparse(n, nvars, npublic, a_csr, b_csr, c_csr, toxic):
    """snark.GenerateTrustedSetup (snark.go:98-251) on a sparse R1CS, toxic = (T, Ka, Kb, Kc, Kbeta, Kgamma, RhoA, RhoB)
    injected instead of drawn at :114-148; runs on the device (gs_pinocchio_setup).  -> (DevicePk, Vk)."""
    # the key's 288 u32 words + IC, as u64 limbs
    dev, v = _scheme.setup(_S, n, nvars, npublic, (a_csr, b_csr, c_csr), toxic, 4 * (72 + 6 * (npublic + 1)))
    g1, g2 = _scheme.g1_at, _scheme.g2_at
    return dev, Vk(IC=[g1(v, 36 + 3 * i) for i in range(npublic + 1)], Vka=g2(v, 0), Vkb=g1(v, 6), Vkc=g2(v, 9), G1Kbg=g1(v, 15),
                   G2Kbg=g2(v, 18), G2Kg=g2(v, 24), Vkz=g2(v, 30))


def ExportPkArray(dev_pk, name):
    return _scheme.ExportPkArray(_S, dev_pk, name)


_CHECKS = ("e(piA, Va) == e(piA', g2), valid knowledge commitment for A",
           "e(Vb, piB) == e(piB', g2), valid knowledge commitment for B",
           "e(piC, Vc) == e(piC', g2), valid knowledge commitment for C",
           "e(Vkx+piA, piB) == e(piH, Vkz) * e(piC, g2), QAP disibility checked",
           "e(Vkx+piA+piC, g2KbetaKgamma) * e(g1KbetaKgamma, piB) == e(piK, g2Kgamma)")


def _proof_words(proof):
    """A proof as the 108 words of gs_pinocchio_verify: PiA, PiAp | PiB | PiBp, PiC, PiCp, PiH, PiKp."""
    words = np.concatenate([capi.g1_points_to_u64([proof.PiA, proof.PiAp]).reshape(-1), capi.g2_points_to_u64([proof.PiB]).reshape(-1),
                            capi.g1_points_to_u64([proof.PiBp, proof.PiC, proof.PiCp, proof.PiH, proof.PiKp]).reshape(-1)])
    return np.ascontiguousarray(words, dtype=np.uint64)


def VerifyProofsEachChecks(vk, proofs, publicSignalsList):
    """Many proofs of ONE verification key on the device (gs_pinocchio_verify_each) -> list[int]: per proof 0, or 1..5 for the first of
    the five equations, in the reference's order, that does not hold -- what gs_pinocchio_verify reports as failed_check for that proof
    with its signals.  Under gs_verify_set_strict(1) a proof refused for a non-canonical encoding also reports 0: VerifyProofsEach
    gives the verdicts.  Needs an initialised device."""
    return _verify_each(vk, proofs, publicSignalsList, "VerifyProofsEachChecks")[1]


def VerifyProofsEach(vk, proofs, publicSignalsList, debug=False):
    """Many proofs of ONE verification key, a verdict for each, on the device (gs_pinocchio_verify_each) -> list[bool]: exactly
    [VerifyProof(vk, p, s) for p, s in zip(proofs, publicSignalsList)], deterministic, no challenge.  debug=True prints, per rejected
    proof, the line VerifyProof(debug=True) prints for its failing check.  VerifyProofsEachChecks returns the failing equation of each
    proof instead; VerifyProof in a loop on the host gives the same answers and takes five final exponentiations per proof on one core.
    Needs an initialised device."""
    ok, bad = _verify_each(vk, proofs, publicSignalsList, "VerifyProofsEach")
    if debug:
        for i, which in enumerate(bad):
            if which:
                print("proof %d: ❌ %s" % (i, _CHECKS[which - 1]))
    return ok


def _verify_each(vk, proofs, publicSignalsList, who):
    if len(proofs) != len(publicSignalsList):
        raise ValueError("%s: %d proofs, %d lists of public signals" % (who, len(proofs), len(publicSignalsList)))
    npublic = len(publicSignalsList[0]) if publicSignalsList else 0
    if any(len(s) != npublic for s in publicSignalsList):
        raise ValueError("%s: every proof of one key has the same number of public signals" % who)
    ic, nic, _, _ = _scheme.verify_inputs(vk, [0] * npublic)
    g1 = capi.g1_points_to_u64([vk.Vkb, vk.G1Kbg])
    g2 = capi.g2_points_to_u64([vk.Vka, vk.Vkc, vk.G2Kbg, vk.G2Kg, vk.Vkz])
    flat = [int(x) % capi.R for s in publicSignalsList for x in s]
    pub = capi.ints_to_u64(flat) if flat else np.zeros((1, 4), dtype=np.uint64)
    n = len(proofs)
    words = np.ascontiguousarray(np.concatenate([_proof_words(p) for p in proofs])) if n else np.zeros(108, dtype=np.uint64)
    ok, bad = np.zeros(max(n, 1), dtype=np.intc), np.zeros(max(n, 1), dtype=np.intc)
    nbad = ctypes.c_uint64(0)
    capi.call("gs_pinocchio_verify_each", capi.ptr64(g2[0]), capi.ptr64(g1[0]), capi.ptr64(g2[1]), capi.ptr64(g1[1]), capi.ptr64(g2[2]),
              capi.ptr64(g2[3]), capi.ptr64(g2[4]), ic, nic, capi.ptr64(pub), npublic, capi.ptr64(words), n, ok.ctypes.data_as(capi.intp),
              bad.ctypes.data_as(capi.intp), ctypes.byref(nbad))
    return [bool(x) for x in ok[:n]], [int(x) for x in bad[:n]]


def VerifyProof(vk, proof, publicSignals, debug=False):
    """snark.VerifyProof(vk, proof, publicSignals, debug) (snark.go:292-368) -> bool: the five pairing equations in the
    reference's order (gs_pinocchio_verify, host side, no device needed).  Many proofs of one key: VerifyProofsEach gives the same
    verdicts on the device, VerifyProofsEachChecks the failing equation of each."""
    inputs = _scheme.verify_inputs(vk, publicSignals)
    g1 = capi.g1_points_to_u64([vk.Vkb, vk.G1Kbg])
    g2 = capi.g2_points_to_u64([vk.Vka, vk.Vkc, vk.G2Kbg, vk.G2Kg, vk.Vkz])
    words = _proof_words(proof)
    ok, bad = ctypes.c_int(0), ctypes.c_int(0)
    capi.call("gs_pinocchio_verify", capi.ptr64(g2[0]), capi.ptr64(g1[0]), capi.ptr64(g2[1]), capi.ptr64(g1[1]), capi.ptr64(g2[2]),
              capi.ptr64(g2[3]), capi.ptr64(g2[4]), *inputs, capi.ptr64(words), ctypes.byref(ok), ctypes.byref(bad))
    if debug:
        for i, text in enumerate(_CHECKS):
            if bad.value and i + 1 == bad.value:
                print("❌ " + text)
                break
            print("✓ " + text)
    return bool(ok.value)
