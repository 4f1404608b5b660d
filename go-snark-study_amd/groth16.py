"""Mirror of the reference's groth16 prover interface (groth16/groth16.go) on the HIP library.

    pk = groth16.Pk(...)                      # same fields as groth16.go:15-32
    proof = groth16.GenerateProofs(circuit, pk, w, px)            # groth16.go:225
    proof = groth16.GenerateProofsWithRS(circuit, pk, w, px, r, s)   # randomness injected

Values are Python ints / tuples shaped like the reference's big.Int structures.  Proof elements
are returned in the affine normal form [x, y, 1] (infinity = all zero)."""
import ctypes
import os

import numpy as np

from . import _scheme, capi
from ._scheme import GS_ERR_BUSY   # noqa: F401
from .capi import R


class Circuit:
    """The fields of circuitcompiler.Circuit the prover reads (circuit.go:12-26; groth16.go:243,248)."""

    def __init__(self, NVars, NPublic):
        self.NVars = NVars
        self.NPublic = NPublic


class Pk:
    """groth16.Pk (groth16.go:15-32)."""

    def __init__(self, BACDelta, Z, G1_Alpha, G1_Beta, G1_Delta, G1_At, G1_BACGamma,
                 G2_Beta, G2_Delta, G2_BACGamma, PowersTauDelta, G2_Gamma=None):
        self.BACDelta, self.Z = BACDelta, Z
        self.G1_Alpha, self.G1_Beta, self.G1_Delta = G1_Alpha, G1_Beta, G1_Delta
        self.G1_At, self.G1_BACGamma = G1_At, G1_BACGamma
        self.G2_Beta, self.G2_Gamma, self.G2_Delta = G2_Beta, G2_Gamma, G2_Delta
        self.G2_BACGamma = G2_BACGamma
        self.PowersTauDelta = PowersTauDelta
        self._dev = None


class Proof:
    """groth16.Proof (groth16.go:61-65)."""

    def __init__(self, PiA, PiB, PiC):
        self.PiA, self.PiB, self.PiC = PiA, PiB, PiC


class DevicePk:
    """Proving key resident in HBM (upload + affine-normalise once per circuit, SURVEY hard part 4)."""

    def __init__(self, handle, nvars, npublic, keep=None):
        self.handle, self.nvars, self.npublic, self._keep = handle, nvars, npublic, keep


def _pk_create(op, at, bacgamma1, bacgamma2, bacdelta, ptd, alpha, beta, delta, beta2, delta2, z_u64, nvars, npublic, *shard):
    capi.init()
    a = capi.g1_points_to_u64([alpha, beta, delta])
    b = capi.g2_points_to_u64([beta2, delta2])
    z = np.ascontiguousarray(z_u64, dtype=np.uint64).reshape(-1, 4)
    cell = capi.HandleCell()
    capi.call(op, *map(capi.raw, (at, bacgamma1, bacgamma2, bacdelta, ptd)), *map(capi.ptr64, (a[0], a[1], a[2], b[0], b[1], z)),
              z.shape[0], nvars, npublic, *shard, cell.ref)
    return DevicePk(cell.result(), nvars, npublic)


def device_pk_from_handles(at, bacgamma1, bacgamma2, bacdelta, ptd, alpha, beta, delta, beta2, delta2, z_u64, nvars, npublic):
    """Assemble a DevicePk from already-resident base arrays (capi.DeviceHandle) and Jacobian int tuples."""
    return _pk_create("gs_groth16_pk_create", at, bacgamma1, bacgamma2, bacdelta, ptd, alpha, beta, delta, beta2, delta2, z_u64, nvars, npublic)


def device_pk_domain_from_handles(at, bacgamma1, bacgamma2, bacdelta, h_coset, alpha, beta, delta, beta2, delta2, log2_domain, nvars, npublic):
    """A coset-only key (gs_groth16_pk_create_domain): `h_coset` holds the 2^log2_domain points of the coset evaluation basis in place
    of PowersTauDelta; Z = x^(2^log2_domain) - 1 is built by the library."""
    capi.init()
    a = capi.g1_points_to_u64([alpha, beta, delta])
    b = capi.g2_points_to_u64([beta2, delta2])
    cell = capi.HandleCell()
    capi.call("gs_groth16_pk_create_domain", *map(capi.raw, (at, bacgamma1, bacgamma2, bacdelta, h_coset)),
              *map(capi.ptr64, (a[0], a[1], a[2], b[0], b[1])), int(log2_domain), nvars, npublic, cell.ref)
    return DevicePk(cell.result(), nvars, npublic)


def device_pk_shard_from_handles(at, bacgamma1, bacgamma2, bacdelta, ptd, alpha, beta, delta, beta2, delta2, z_u64, nvars, npublic,
                                 nptd_total, shard_index, shard_count):
    return _pk_create("gs_groth16_pk_create_shard", at, bacgamma1, bacgamma2, bacdelta, ptd, alpha, beta, delta, beta2, delta2, z_u64,
                      nvars, npublic, nptd_total, shard_index, shard_count)


class Vk:
    """groth16.Vk (groth16.go:33-43): affine Jacobian tuples."""

    def __init__(self, IC, G1_Alpha, G2_Beta, G2_Gamma, G2_Delta):
        self.IC, self.G1_Alpha, self.G2_Beta, self.G2_Gamma, self.G2_Delta = IC, G1_Alpha, G2_Beta, G2_Gamma, G2_Delta


# "PowersTauDeltaEval": the evaluation-basis copy of PowersTauDelta (include/gosnark_hip.h, gs_groth16_pk_set_eval) -- not a field
# of the reference's Pk; keys built by gs_groth16_setup carry it, the binary key container stores it as an extra section.
# "PowersTauDeltaQuot": the quotient-basis array Q_m = sum_{d <= m} g_d PowersTauDelta[m - d], g = 1 / rev(Z) (gs_groth16_pk_set_quot):
# with it the h-sum of a proof runs over the top coefficients of px and nothing is divided by Z.
PK_ARRAYS = {"G1_At": 0, "G1_BACGamma": 1, "G2_BACGamma": 2, "BACDelta": 3, "PowersTauDelta": 4, "PowersTauDeltaEval": 7, "PowersTauDeltaQuot": 10}


def UploadPk(pk, circuit):
    """Additive extension: make pk resident.  Cached on the Pk object."""
    if pk._dev is not None:
        return pk._dev
    at = capi.g1_upload(capi.g1_points_to_u64(pk.G1_At))
    b1 = capi.g1_upload(capi.g1_points_to_u64(pk.G1_BACGamma))
    b2 = capi.g2_upload(capi.g2_points_to_u64(pk.G2_BACGamma))
    cd = capi.g1_upload(capi.g1_points_to_u64(pk.BACDelta))
    pt = capi.g1_upload(capi.g1_points_to_u64(pk.PowersTauDelta))
    pk._dev = device_pk_from_handles(at, b1, b2, cd, pt, pk.G1_Alpha, pk.G1_Beta, pk.G1_Delta, pk.G2_Beta, pk.G2_Delta,
                                     capi.ints_to_u64([z % R for z in pk.Z]), circuit.NVars, circuit.NPublic)
    return pk._dev


def _proof_from_words(out, inf):
    v = capi.u64_to_ints(out)
    PiA = (0, 0, 0) if inf[0] else (v[0], v[1], 1)
    PiB = ((0, 0), (0, 0), (0, 0)) if inf[1] else ((v[2], v[3]), (v[4], v[5]), (1, 0))
    PiC = (0, 0, 0) if inf[2] else (v[6], v[7], 1)
    return Proof(PiA, PiB, PiC)


_S = _scheme.Scheme(prefix="gs_groth16_", proof=(32, 3), partials=(48, 5), has_rs=True, decode=_proof_from_words, arrays=PK_ARRAYS,
                    g2_array=2, h_array=4, eval_array=7, quot_array=10, DevicePk=DevicePk, UploadPk=UploadPk,
                    negative_note=" (the reference drops the sign, fq.go:138-140)")


def GenerateTrustedSetupSparse(n, nvars, npublic, a_csr, b_csr, c_csr, toxic):
    """groth16.GenerateTrustedSetup (groth16.go:94-222) on a sparse R1CS with the toxic scalars
    (T, Kalpha, Kbeta, Kgamma, Kdelta) injected instead of drawn at :99-119.  Everything heavy runs on the device
    (gs_groth16_setup); returns (DevicePk resident in HBM, Vk)."""
    dev, v = _scheme.setup(_S, n, nvars, npublic, (a_csr, b_csr, c_csr), toxic, 12 + 72 + 12 * (npublic + 1))
    g1, g2 = _scheme.g1_at, _scheme.g2_at
    return dev, Vk(IC=[g1(v, 21 + 3 * i) for i in range(npublic + 1)], G1_Alpha=g1(v, 0), G2_Beta=g2(v, 3), G2_Gamma=g2(v, 9), G2_Delta=g2(v, 15))


def ExportPkArray(dev_pk, name):
    """One array of a resident key as affine Jacobian int tuples (testing / serialisation)."""
    return _scheme.ExportPkArray(_S, dev_pk, name)


def _shard_range(n, count, index):
    q, rem = divmod(n, count)
    lo = index * q + min(index, rem)
    return lo, lo + q + (1 if index < rem else 0)


def ShardPk(dev_pk, shard_index, shard_count):
    """The slice of a resident full key that rank `shard_index` of `shard_count` needs for prove_partials / prove_sharded
    (gs_groth16_pk_shard).  Free the full key afterwards (dev_pk.handle.free()) to keep only 1/shard_count of it in HBM."""
    return _scheme.shard(_S, dev_pk, shard_index, shard_count)


def ShardPkTo(dev_pk, shard_index, shard_count, target_device):
    """The same slice, created on logical device `target_device` (gs_groth16_pk_shard_to; the copies cross xGMI when the two
    are different GPUs)."""
    return _scheme.shard(_S, dev_pk, shard_index, shard_count, int(target_device))


def UploadPkShard(pk, circuit, shard_index, shard_count):
    """Upload ONLY this rank's slice of a host key (gs_groth16_pk_create_shard): arrays cut with the split prove_partials uses."""
    capi.init()
    wlo, whi = _shard_range(circuit.NVars, shard_count, shard_index)
    hlo, hhi = _shard_range(len(pk.PowersTauDelta), shard_count, shard_index)
    empty1, empty2 = np.zeros((0, 12), dtype=np.uint64), np.zeros((0, 24), dtype=np.uint64)
    up1 = lambda pts: capi.g1_upload(capi.g1_points_to_u64(pts) if pts else empty1)     # noqa: E731
    at, b1, cd = up1(pk.G1_At[wlo:whi]), up1(pk.G1_BACGamma[wlo:whi]), up1(pk.BACDelta[wlo:whi])
    pt = up1(pk.PowersTauDelta[hlo:hhi])
    sl2 = pk.G2_BACGamma[wlo:whi]
    b2 = capi.g2_upload(capi.g2_points_to_u64(sl2) if sl2 else empty2)
    return device_pk_shard_from_handles(at, b1, b2, cd, pt, pk.G1_Alpha, pk.G1_Beta, pk.G1_Delta, pk.G2_Beta, pk.G2_Delta,
                                        capi.ints_to_u64([z % R for z in pk.Z]), circuit.NVars, circuit.NPublic, len(pk.PowersTauDelta),
                                        shard_index, shard_count)


def FqRRand():
    """Utils.FqR.Rand (fields/fq.go:116-132): 30 random bytes, big-endian, mod r."""
    return int.from_bytes(os.urandom(30), "big") % R


def GenerateProofsWithRS(circuit, pk, w, px, r, s):
    """groth16.go:225-278 with r, s given instead of drawn at :231-238.  Round 6 (as go/groth16hip.GenerateProofsWithRS): w and px travel
    as a HOST-BUFFER TICKET collected at once (gs_groth16_prove_host_begin + gs_groth16_prove_end: staged into the slot's own device
    buffers, nothing allocated per proof, concurrent callers pipeline); when all three slots are taken, the blocking entry point."""
    return _scheme.generate(_S, circuit, pk, w, px, (r, s))


def GenerateProofs(circuit, pk, w, px):
    """groth16.GenerateProofs(circuit, pk, w, px) (groth16.go:225)."""
    return GenerateProofsWithRS(circuit, pk, w, px, FqRRand(), FqRRand())


def GenerateProofsFromWitnessWithRS(circuit, pk, dev_r1cs, w, r, s):
    """go/groth16hip.GenerateProofsFromWitnessWithRS: the callers' R1CSToQAP -> CombinePolynomials -> GenerateProofs chain (cli/main.go:480-501)
    from the witness alone, against the circuit's resident sparse R1CS (r1csqap.DeviceR1CS); a host-buffer ticket collected at once."""
    return _scheme.generate_from_witness(_S, circuit, pk, dev_r1cs, w, (r, s))


def GenerateProofsChecked(circuit, pk, dev_r1cs, w, r=None, s=None, check_r1cs=None):
    """go/groth16hip.GenerateProofsChecked: the witness is checked against ALL constraints of check_r1cs (default: dev_r1cs) first
    (DeviceR1CS.CheckWitness); a bad one raises r1csqap.WitnessError before anything is proved, a good one is proved from the same
    resident vector (gs_groth16_prove_witness): the proof of the unchecked call with the same r, s."""
    return _scheme.generate_checked(_S, circuit, pk, dev_r1cs, w, (FqRRand() if r is None else r, FqRRand() if s is None else s), check_r1cs)


def GenerateProofsFromInputs(circuit, pk, dev_r1cs, plan, inputs, r=None, s=None):
    """go/gosnarkhip R1csSolve + GenerateProofsChecked: the witness is SOLVED on the device from the values of the plan's input variables
    (plan = dev_r1cs.PlanSolve(input_vars), once per circuit), checked against all constraints and proved from the same resident
    vector.  r1csqap.SolveError: variables stay unsolved or a divisor was zero; r1csqap.WitnessError: a check row is broken."""
    return _scheme.generate_from_inputs(_S, circuit, pk, dev_r1cs, plan, inputs, (FqRRand() if r is None else r, FqRRand() if s is None else s))


class Prover(_scheme.Prover):
    """The streaming drop-in (go/groth16hip.Prover, tests/c/stream_producer.c): one resident key, a NEW witness per Submit, up to three
    proofs in flight, proofs back in submission order.
        p = groth16.NewProver(circuit, pk, dev_r1cs)          # dev_r1cs = None: every Submit brings px
        for w in witnesses:
            p.Submit(w)                                       # or p.Submit(w, px)
            if p.InFlight() == 3: proof = p.Collect()
        while p.InFlight(): proof = p.Collect()
    A Submit on a full pipeline first collects the oldest ticket into a done-queue (it never fails with GS_ERR_BUSY)."""
    scheme = _S

    def SubmitWithRS(self, w, px, r, s):
        self._submit(w, px, (r, s))

    def Submit(self, w, px=None):
        self.SubmitWithRS(w, px, FqRRand(), FqRRand())


def NewProver(circuit, pk, dev_r1cs=None):
    return Prover(circuit, pk, dev_r1cs)


def prove_resident(dev_pk, w_handle, px_handle, r, s):
    """Inputs already resident in HBM (what bench.py times)."""
    return _scheme.prove(_S, "prove_resident", dev_pk, w_handle, px_handle, (r, s))


def prove_from_r1cs(dev_pk, dev_r1cs, w_handle, r, s, px_handle=None):
    """Sparse R1CS + resident witness -> proof in one call (gs_groth16_prove_r1cs): px is computed behind the accumulations
    over w.  Returns (Proof, px_handle); pass the previous px_handle to overwrite it instead of allocating."""
    return _scheme.prove_from_r1cs(_S, dev_pk, dev_r1cs, w_handle, (r, s), px_handle)


def prove_from_witness(dev_pk, dev_r1cs, w_handle, r, s):
    """Sparse R1CS + resident witness -> proof, H(x) straight from the constraint values (gs_groth16_prove_witness): no px."""
    return _scheme.prove(_S, "prove_witness", dev_pk, dev_r1cs, w_handle, (r, s))


def prove_witness_begin(dev_pk, dev_r1cs, w_handle, r, s):
    """Enqueue one witness -> proof (gs_groth16_prove_witness_begin) -> ticket for prove_end.  With an evaluation-basis key the
    call never waits for the device."""
    return _scheme.begin(_S, "prove_witness_begin", dev_pk, dev_r1cs, w_handle, (r, s))


def prove_host_begin(dev_pk, w, px, r, s):
    """groth16.GenerateProofs' own call shape at the pipelined rate (gs_groth16_prove_host_begin): w and px in HOST memory (ints or
    [n, 4] uint64 arrays), new ones every call, staged into the ticket slot's own device buffers -> ticket for prove_end."""
    return _scheme.prove_host_begin(_S, dev_pk, w, px, (r, s))


def prove_witness_host_begin(dev_pk, dev_r1cs, w, r, s):
    """A fresh witness in HOST memory against the resident sparse R1CS (gs_groth16_prove_witness_host_begin) -> ticket for prove_end."""
    return _scheme.prove_witness_host_begin(_S, dev_pk, dev_r1cs, w, (r, s))


def prove_from_witness_host(dev_pk, dev_r1cs, w, r, s):
    """Blocking: host witness -> proof (gs_groth16_prove_witness_host)."""
    return _scheme.prove_from_witness_host(_S, dev_pk, dev_r1cs, w, (r, s))


def SetEvalBasis(dev_pk, points):
    """Attach an evaluation-basis copy of PowersTauDelta (n Jacobian int triples, e.g. read from a key file) to a resident key:
    gs_groth16_pk_set_eval.  The witness route then runs its h-MSM over H's values (no interpolation)."""
    _scheme.set_basis(_S, "eval", dev_pk, capi.g1_points_to_u64(points))


def SetQuotBasis(dev_pk, points):
    """Attach a quotient-basis array (len(PowersTauDelta) Jacobian int triples, PK_ARRAYS above) to a resident key:
    gs_groth16_pk_set_quot.  points = None detaches it: the key divides px by Z again."""
    _scheme.set_basis(_S, "quot", dev_pk, None if points is None else capi.g1_points_to_u64(points))


def DeriveQuotBasis(dev_pk):
    """Compute the quotient-basis array of a resident key from its PowersTauDelta and Z (gs_groth16_pk_derive_quot: a transform in
    the group, seconds for a 2^20 key) and attach it."""
    _scheme.derive_basis(_S, "quot", dev_pk)


def DeriveEvalBasis(dev_pk, n):
    """Compute the evaluation-basis array of a resident key from its PowersTauDelta alone (gs_groth16_pk_derive_eval: a transposed
    subproduct tree in the group over the nodes n+1..2n) and attach it as SetEvalBasis would.  n = the number of constraints."""
    _scheme.derive_basis(_S, "eval", dev_pk, int(n))


SUM_IS_G2 = [False, False, True, False, False]


def _sums_from_words(out, inf):
    """A rank's five raw MSM sums [At, G1.BACGamma, G2.BACGamma, BACDelta, h.PTD] as affine points / None."""
    v = capi.u64_to_ints(out)
    return [None if inf[0] else (v[0], v[1]), None if inf[1] else (v[2], v[3]),
            None if inf[2] else ((v[4], v[5]), (v[6], v[7])), None if inf[3] else (v[8], v[9]), None if inf[4] else (v[10], v[11])]


def prove_partials(dev_pk, w_handle, px_handle, shard_index, shard_count):
    """This rank's five raw MSM sums (gs_groth16_prove_partials): [At, G1.BACGamma, G2.BACGamma, BACDelta, h.PTD] as affine
    points / None, plus the g2 flags parallel.allgather_points wants."""
    return _sums_from_words(*_scheme.partials(_S, "prove_partials", dev_pk, w_handle, px_handle, shard_index, shard_count)), SUM_IS_G2


def finish(dev_pk, sums, r, s):
    """gs_groth16_finish: the O(1) tail of groth16.go:253-275 on the (combined) five sums."""
    arr, ia = capi.affine_words(sums, SUM_IS_G2)
    return _scheme.call_proof(_S, "finish", capi.raw(dev_pk), capi.ptr64(arr), ia, *capi.rs_limbs(r, s))


def prove_sharded(dev_pk, w_handle, px_handle, r, s, group=None):
    """One proof over all ranks of `group` (one process per GPU): local sums over this rank's term ranges -> ONE all-gather of
    the 5 partial points per rank -> local combination -> tail.  Every rank returns the same Proof."""
    import torch.distributed as dist
    from . import parallel
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    pts, flags = prove_partials(dev_pk, w_handle, px_handle, rank, world)
    per_rank = parallel.allgather_points(pts, flags, group)
    return finish(dev_pk, parallel.combine_partials(per_rank, flags), r, s)


def prove_multi(dev_pks, w_handles, px_handles, r, s):
    """One proof over len(dev_pks) logical devices of THIS process (gs_groth16_prove_multi): dev_pks[d] is the full key or
    slice d on logical device d, w_handles[d] / px_handles[d] replicas there.  Returns (Proof, used_rccl)."""
    return _scheme.prove_multi(_S, "prove_multi", dev_pks, w_handles, px_handles, (r, s))


def witness_values(dev_pk, dev_r1cs, w_handle, hv_handle=None):
    """The proof owner's polynomial stage (gs_groth16_witness_values): resident sparse R1CS + witness -> the n values H(n+1..2n) as a
    resident scalar vector.  Returns (hv_handle, violated); violated != 0 means the witness breaks a constraint and the values are void."""
    return _scheme.witness_values(_S, dev_pk, dev_r1cs, w_handle, hv_handle)


def prove_partials_values(dev_pk, w_handle, hv_slice, shard_index, shard_count):
    """gs_groth16_prove_partials_values: this rank's five sums, the fifth over its slice of H's values (no polynomial work here)."""
    return _sums_from_words(*_scheme.partials(_S, "prove_partials_values", dev_pk, w_handle, hv_slice, shard_index, shard_count)), SUM_IS_G2


def partials_values_begin(dev_pk, w_handle, hv_slice, shard_index, shard_count):
    """gs_groth16_partials_values_begin -> ticket (collect with partials_end)."""
    return _scheme.partials_begin(_S, "partials_values_begin", dev_pk, w_handle, hv_slice, shard_index, shard_count)


def partials_end(ticket):
    """gs_groth16_partials_end -> the five sums as prove_partials returns them."""
    return _sums_from_words(*_scheme.partials_end(_S, ticket))


def scatter_values(hv_handle, ndev):
    """The owner's scatter between the logical devices of this process: slice d of the contiguous split of H's values -> device d."""
    n = len(hv_handle)
    out = []
    for d in range(ndev):
        lo, hi = _shard_range(n, ndev, d)
        out.append(capi.scalars_clone(hv_handle, d, lo, hi - lo))
    return out


def prove_multi_values(dev_pks, w_handles, hv_slices, r, s):
    """One proof over the logical devices of this process with the polynomial stage done ONCE (gs_groth16_prove_multi_values):
    hv_slices[d] = device d's slice of H's values (scatter_values).  Returns (Proof, used_rccl)."""
    return _scheme.prove_multi(_S, "prove_multi_values", dev_pks, w_handles, hv_slices, (r, s))


def prove_sharded_values_rccl(dev_pk, w_handle, hv_slice, r, s):
    """One process per GPU, values route (gs_groth16_prove_sharded_values): this rank's slice of H's values came from the owner
    through capi.scalars_scatter; the 416-byte records are gathered inside the library."""
    return _scheme.prove(_S, "prove_sharded_values", dev_pk, w_handle, hv_slice, (r, s))


def prove_sharded_rccl(dev_pk, w_handle, px_handle, r, s):
    """One process per GPU, gathered INSIDE the library over the communicator of capi.comm_init_rank
    (gs_groth16_prove_sharded).  Every rank returns the same Proof."""
    return _scheme.prove(_S, "prove_sharded", dev_pk, w_handle, px_handle, (r, s))


def prove_batch(pk_of_device, w_handles, px_handles, rs_pairs):
    """A batch of independent proofs round-robined over logical devices (gs_groth16_prove_batch, BASELINE configs[4]): proof i
    runs where w_handles[i] lives, with pk_of_device[that device] (None for unused devices).  No collective."""
    return _scheme.prove_batch(_S, pk_of_device, w_handles, px_handles, rs_pairs)


def prove_begin(dev_pk, w_handle, px_handle, r, s):
    """Enqueue one proof (gs_groth16_prove_begin) -> ticket.  At most three may be outstanding."""
    return _scheme.begin(_S, "prove_begin", dev_pk, w_handle, px_handle, (r, s))


def prove_end(ticket):
    """Wait for that proof and return it (gs_groth16_prove_end)."""
    return _scheme.prove_end(_S, ticket)


def VerifyProof(vk, proof, publicSignals, debug=False):
    """groth16.VerifyProof(vk, proof, publicSignals, debug) (groth16.go:281-305) -> bool.  Host side
    (gs_groth16_verify: one 4-pair multi-pairing with a shared final exponentiation); needs no device."""
    inputs = _scheme.verify_inputs(vk, publicSignals)
    g1 = capi.g1_points_to_u64([vk.G1_Alpha, proof.PiA, proof.PiC])
    g2 = capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta, proof.PiB])
    ok = ctypes.c_int(0)
    capi.call("gs_groth16_verify", capi.ptr64(g1[0]), capi.ptr64(g2[0]), capi.ptr64(g2[1]), capi.ptr64(g2[2]), *inputs,
              capi.ptr64(g1[1]), capi.ptr64(g2[3]), capi.ptr64(g1[2]), ctypes.byref(ok))
    if debug:
        print("✓ groth16 verification passed" if ok.value else "❌ groth16 verification not passed")
    return bool(ok.value)


def VerifyProofsEach(vk, proofs, publicSignalsList):
    """Many proofs of ONE verification key, a verdict for each, on the device (gs_groth16_verify_each) -> list[bool]: exactly
    [VerifyProof(vk, p, s) for p, s in zip(proofs, publicSignalsList)], deterministic, no challenge and no soundness caveat.
    When to use which: VerifyProofs answers "are all of them valid" for about a third of the cost and is the right first call for a
    batch that is expected to be clean; when it says False -- or when the verdicts are wanted one by one anyway -- this call says WHICH
    proofs are bad, where VerifyProof in a loop on the host would take hundreds of times as long.  Needs an initialised device."""
    if len(proofs) != len(publicSignalsList):
        raise ValueError("VerifyProofsEach: %d proofs, %d lists of public signals" % (len(proofs), len(publicSignalsList)))
    npublic = len(publicSignalsList[0]) if publicSignalsList else 0
    if any(len(s) != npublic for s in publicSignalsList):
        raise ValueError("VerifyProofsEach: every proof of one key has the same number of public signals")
    return _verify_each_words(vk, _proof_words(proofs), publicSignalsList, npublic)


def _proof_words(proofs):
    """[Proof] -> (A as [n, 12] uint64 Jacobian words, B as [n, 24], C as [n, 12])."""
    return (capi.g1_points_to_u64([p.PiA for p in proofs]), capi.g2_points_to_u64([p.PiB for p in proofs]),
            capi.g1_points_to_u64([p.PiC for p in proofs]))


def _verify_each_words(vk, abc, publicSignalsList, npublic):
    """gs_groth16_verify_each on the proofs' points as word arrays (_proof_words, or compressed.decompress_proof_arrays) -> list[bool]."""
    n = len(publicSignalsList)
    ic, nic, _, _ = _scheme.verify_inputs(vk, [0] * npublic)
    g1 = capi.g1_points_to_u64([vk.G1_Alpha])
    g2 = capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta])
    flat = [int(x) % capi.R for s in publicSignalsList for x in s]
    pub = capi.ints_to_u64(flat) if flat else np.zeros((1, 4), dtype=np.uint64)
    a, b, c = [np.ascontiguousarray(v, dtype=np.uint64) if n else np.zeros((1, w), dtype=np.uint64) for v, w in zip(abc, (12, 24, 12))]
    ok = np.zeros(max(n, 1), dtype=np.intc)
    nbad = ctypes.c_uint64(0)
    capi.call("gs_groth16_verify_each", capi.ptr64(g1[0]), capi.ptr64(g2[0]), capi.ptr64(g2[1]), capi.ptr64(g2[2]), ic, nic,
              capi.ptr64(pub), npublic, capi.ptr64(a), capi.ptr64(b), capi.ptr64(c), n, ok.ctypes.data_as(capi.intp),
              ctypes.byref(nbad))
    return [bool(x) for x in ok[:n]]


class DeviceVk:
    """A verification key prepared and resident on the device (gs_groth16_vk_create): its IC points, the prepared lines of gamma and
    delta and the Miller value of e(alpha, beta).  `handle` is freed like the other device objects; `npublic` = len(vk.IC) - 1."""

    def __init__(self, handle, npublic):
        self.handle, self.npublic = handle, npublic


def PrepareVerificationKey(vk):
    """Do once per key what VerifyProofsEach does per call -- the curve tests of the key, the Miller value of e(alpha, beta), the
    prepared lines of gamma and delta -- and keep the result on the device -> DeviceVk, for VerifyProofsEachKeys.  A key that cannot
    verify anything (a point off its curve, a G2 point that is not of order r) raises GosnarkHipError naming the point, where
    VerifyProofsEach would answer False for every proof."""
    g2 = capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta])
    handle = capi.groth16_vk_create(capi.g1_points_to_u64([vk.G1_Alpha])[0], g2[0], g2[1], g2[2], capi.g1_points_to_u64(vk.IC))
    return DeviceVk(handle, len(vk.IC) - 1)


def VerifyProofsEachKeys(keys, key_of_proof, proofs, publicSignalsList):
    """Proofs of MANY verification keys in one call, a verdict for each, on the device (gs_groth16_verify_each_keys) -> list[bool]:
    exactly [VerifyProof(vk of keys[key_of_proof[i]], proofs[i], publicSignalsList[i]) for i ...].  `keys` are DeviceVk objects from
    PrepareVerificationKey (the same one may appear twice, one may have no proofs); every proof brings exactly its key's npublic
    signals.  One call costs the latency of one wave's loop however many keys it names, where VerifyProofsEach per key costs it once
    per key.  A proof whose key index is out of range raises GosnarkHipError; a length mismatch ValueError."""
    return _verify_each_keys_words(keys, key_of_proof, _proof_words(proofs), publicSignalsList, "VerifyProofsEachKeys")


def _verify_each_keys_words(keys, key_of_proof, abc, publicSignalsList, what):
    key_of_proof = [int(k) for k in key_of_proof]
    n = len(publicSignalsList)
    if len(key_of_proof) != n or len(abc[0]) != n:
        raise ValueError("%s: %d proofs, %d key indices, %d lists of public signals" % (what, len(abc[0]), len(key_of_proof), n))
    for i, (k, s) in enumerate(zip(key_of_proof, publicSignalsList)):
        if 0 <= k < len(keys) and len(s) != keys[k].npublic:
            raise ValueError("%s: proof %d has %d public signals, its key (keys[%d]) takes %d" % (what, i, len(s), k, keys[k].npublic))
        if k < 0:
            raise ValueError("%s: proof %d has the key index %d" % (what, i, k))
    flat = [int(x) % capi.R for s in publicSignalsList for x in s]
    pub = capi.ints_to_u64(flat) if flat else np.zeros((1, 4), dtype=np.uint64)
    ok, _ = capi.groth16_verify_each_keys(keys, key_of_proof, pub, *abc)
    return [bool(x) for x in ok]


def VerifyProofsEachKeysCompressed(keys, key_of_proof, blobs, publicSignalsList, codec):
    """VerifyProofsEachKeys on proofs as they arrive over a wire (128 bytes each, see VerifyProofsEachCompressed): the points are
    decompressed on the device, then go to gs_groth16_verify_each_keys -> list[bool], False for a proof with a point that does not
    decompress; the other verdicts are unaffected by it."""
    from . import compressed
    if len(blobs) != len(publicSignalsList):
        raise ValueError("VerifyProofsEachKeysCompressed: %d proofs, %d lists of public signals" % (len(blobs), len(publicSignalsList)))
    a, b, c, ok = compressed.decompress_proof_arrays(blobs, codec)
    got = _verify_each_keys_words(keys, key_of_proof, (a, b, c), publicSignalsList, "VerifyProofsEachKeysCompressed")
    return [bool(v and o) for v, o in zip(got, ok)]


def VerifyProofs(vk, proofs, publicSignalsList, seed=None):
    """Many proofs of ONE verification key in one randomised check on the device (gs_groth16_verify_batch) -> bool: the answer of
    all(VerifyProof(vk, p, s) ...), wrong with probability at most (len(proofs) - 1) / r, and only towards True.  The challenge is
    drawn from the operating system's randomness unless `seed` is given (tests: reproducible; a predictable challenge voids the
    bound).  False does not say which proof is bad: VerifyProofsEach says which (VerifyProof on each does too, on the host).  Needs an
    initialised device."""
    if len(proofs) != len(publicSignalsList):
        raise ValueError("VerifyProofs: %d proofs, %d lists of public signals" % (len(proofs), len(publicSignalsList)))
    npublic = len(publicSignalsList[0]) if publicSignalsList else 0
    if any(len(s) != npublic for s in publicSignalsList):
        raise ValueError("VerifyProofs: every proof of one key has the same number of public signals")
    return _verify_batch_words(vk, _proof_words(proofs), publicSignalsList, npublic, seed)


def _verify_batch_words(vk, abc, publicSignalsList, npublic, seed):
    """gs_groth16_verify_batch on the proofs' points as word arrays -> bool."""
    n = len(publicSignalsList)
    ic, nic, _, _ = _scheme.verify_inputs(vk, [0] * npublic)
    if seed is None:
        import secrets
        challenge = 2 + secrets.randbelow(capi.R - 2)
    else:
        import random
        challenge = random.Random(seed).randrange(2, capi.R)
    g1 = capi.g1_points_to_u64([vk.G1_Alpha])
    g2 = capi.g2_points_to_u64([vk.G2_Beta, vk.G2_Gamma, vk.G2_Delta])
    flat = [int(x) % capi.R for s in publicSignalsList for x in s]
    pub = capi.ints_to_u64(flat) if flat else np.zeros((1, 4), dtype=np.uint64)
    a, b, c = [np.ascontiguousarray(v, dtype=np.uint64) if n else np.zeros((1, w), dtype=np.uint64) for v, w in zip(abc, (12, 24, 12))]
    ok = ctypes.c_int(0)
    capi.call("gs_groth16_verify_batch", capi.ptr64(g1[0]), capi.ptr64(g2[0]), capi.ptr64(g2[1]), capi.ptr64(g2[2]), ic, nic,
              capi.ptr64(pub), npublic, capi.ptr64(a), capi.ptr64(b), capi.ptr64(c), n, capi.ptr64(capi.ints_to_u64([challenge])),
              ctypes.byref(ok))
    return bool(ok.value)


def _compressed_inputs(what, blobs, publicSignalsList, codec):
    from . import compressed
    if len(blobs) != len(publicSignalsList):
        raise ValueError("%s: %d proofs, %d lists of public signals" % (what, len(blobs), len(publicSignalsList)))
    npublic = len(publicSignalsList[0]) if publicSignalsList else 0
    if any(len(s) != npublic for s in publicSignalsList):
        raise ValueError("%s: every proof of one key has the same number of public signals" % what)
    a, b, c, ok = compressed.decompress_proof_arrays(blobs, codec)
    return (a, b, c), ok, npublic


def VerifyProofsEachCompressed(vk, blobs, publicSignalsList, codec):
    """VerifyProofsEach on proofs as they arrive over a wire: 128 bytes each, A | B | C, compressed points in the format `codec`
    (compressed.GNARK, .ARKWORKS, .BN256_PAIRING) -> list[bool].  The points are decompressed on the device (one gs_g1_decompress call
    over A and C, one gs_g2_decompress call) and go to gs_groth16_verify_each as they come back: exactly VerifyProofsEach of
    compressed.DecompressProofs(blobs, codec), and False for a proof with a point that does not decompress; the other verdicts are
    unaffected by it."""
    abc, ok, npublic = _compressed_inputs("VerifyProofsEachCompressed", blobs, publicSignalsList, codec)
    return [bool(v and o) for v, o in zip(_verify_each_words(vk, abc, publicSignalsList, npublic), ok)]


def VerifyProofsCompressed(vk, blobs, publicSignalsList, codec, seed=None):
    """VerifyProofs on compressed proofs -> bool: False when any point fails to decompress, else VerifyProofs of the decompressed
    proofs (same challenge rule, same bound)."""
    abc, ok, npublic = _compressed_inputs("VerifyProofsCompressed", blobs, publicSignalsList, codec)
    if not bool(np.all(ok)):
        return False
    return _verify_batch_words(vk, abc, publicSignalsList, npublic, seed)
