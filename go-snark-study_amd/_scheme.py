"""The binding of the prover entry points, written once for both proof schemes (the Python twin of prove.h's ProverKey).

A Scheme is data: what differs between gs_groth16_* and gs_pinocchio_*.  Every function here takes one and marshals one family of
entry points; groth16.py and snark.py hold a Scheme each and give the functions their public names and signatures.  `rs` is the
pair (r, s) for a scheme whose calls carry randomness and () otherwise."""
import collections
import ctypes

import numpy as np

from . import capi, r1csqap
from .capi import call, harr, ptr64, raw

GS_ERR_BUSY = -6

Scheme = collections.namedtuple("Scheme", (
    "prefix",          # "gs_groth16_" / "gs_pinocchio_"
    "proof",           # (words, infinity flags) of a proof
    "partials",        # (words, infinity flags) of a rank's partial sums
    "has_rs",          # the calls carry r, s
    "decode",          # (words, flags) -> Proof
    "arrays",          # PK_ARRAYS: name -> index of gs_*_pk_export; all hold nvars points of G1 except the four below
    "g2_array", "h_array", "eval_array", "quot_array",     # the G2 array; nvars - 1 points; gs_pk_eval_count; gs_pk_quot_count
    "DevicePk",        # DevicePk(handle, nvars, npublic)
    "UploadPk",        # (host Pk, circuit) -> DevicePk
    "negative_note"))  # tail of the message that rejects negative host scalars


def _rs(S, rs):
    assert len(rs) == (2 if S.has_rs else 0)
    return capi.rs_limbs(*rs) if rs else ()


def call_proof(S, op, *args):
    """Blocking entry point whose arguments end in the proof's words and infinity flags."""
    out, inf = capi.result(*S.proof)
    call(S.prefix + op, *args, ptr64(out), inf)
    return S.decode(out, inf)


def call_ticket(S, op, *args):
    """*_begin entry point whose arguments end in the ticket."""
    t = capi.ticket_cell()
    call(S.prefix + op, *args, ctypes.byref(t))
    return t.value


def _rows(a):
    return ptr64(a), a.shape[0]


def host_scalars(S, x, what):
    """The reference's []*big.Int (Python ints: reduced mod r here, negatives rejected) or an [n, 4] uint64 limb array (taken as it
    is: the device reduces any value < 2^256) -> contiguous [n, 4] uint64."""
    if not isinstance(x, np.ndarray) and any(v < 0 for v in x):
        raise ValueError("negative %s values are not supported%s" % (what, S.negative_note))
    return capi.u64_rows(x)


def resident(S, circuit, pk):
    return pk if isinstance(pk, S.DevicePk) else S.UploadPk(pk, circuit)


# ---- one proof on one device: three resident objects (key, w, px | key, R1CS, w | key, w, H's values) or host buffers ------------
def prove(S, op, pk, a, b, rs=()):
    """op: prove_resident, prove_witness, prove_sharded, prove_sharded_values."""
    return call_proof(S, op, raw(pk), raw(a), raw(b), *_rs(S, rs))


def begin(S, op, pk, a, b, rs=()):
    """op: prove_begin, prove_witness_begin -> ticket for prove_end."""
    return call_ticket(S, op, raw(pk), raw(a), raw(b), *_rs(S, rs))


def prove_from_r1cs(S, pk, r1cs, w, rs=(), px_handle=None):
    cell = capi.HandleCell(px_handle)
    return call_proof(S, "prove_r1cs", raw(pk), raw(r1cs), raw(w), cell.ref, *_rs(S, rs)), cell.result()


def prove_host(S, pk, w, px, rs=()):
    return call_proof(S, "prove", raw(pk), *_rows(capi.u64_rows(w)), *_rows(capi.u64_rows(px)), *_rs(S, rs))


def prove_host_begin(S, pk, w, px, rs=()):
    return call_ticket(S, "prove_host_begin", raw(pk), *_rows(capi.u64_rows(w)), *_rows(capi.u64_rows(px)), *_rs(S, rs))


def prove_from_witness_host(S, pk, r1cs, w, rs=()):
    return call_proof(S, "prove_witness_host", raw(pk), raw(r1cs), *_rows(capi.u64_rows(w)), *_rs(S, rs))


def prove_witness_host_begin(S, pk, r1cs, w, rs=()):
    return call_ticket(S, "prove_witness_host_begin", raw(pk), raw(r1cs), *_rows(capi.u64_rows(w)), *_rs(S, rs))


def prove_end(S, ticket):
    return call_proof(S, "prove_end", ticket)


def _unless_busy(S, begin_ticket, blocking):
    """A host-buffer ticket collected at once; the blocking entry point when all of the device's ticket slots are taken."""
    try:
        return prove_end(S, begin_ticket())
    except capi.GosnarkHipError as e:
        if e.code != GS_ERR_BUSY:
            raise
    return blocking()


def generate(S, circuit, pk, w, px, rs=()):
    dev, wa, pa = resident(S, circuit, pk), host_scalars(S, w, "witness"), host_scalars(S, px, "px")
    return _unless_busy(S, lambda: prove_host_begin(S, dev, wa, pa, rs), lambda: prove_host(S, dev, wa, pa, rs))


def generate_from_witness(S, circuit, pk, r1cs, w, rs=()):
    dev, wa = resident(S, circuit, pk), host_scalars(S, w, "witness")
    return _unless_busy(S, lambda: prove_witness_host_begin(S, dev, r1cs, wa, rs), lambda: prove_from_witness_host(S, dev, r1cs, wa, rs))


def generate_checked(S, circuit, pk, r1cs, w, rs=(), check_r1cs=None):
    """Refusal on request: the witness is uploaded once, checked against ALL constraints of `check_r1cs` (default: `r1cs`; the
    three-matrix system of circuit.r1cs when `r1cs` is a .zkey key's product system) with cap 16, and only a witness that passes is
    proved, from the same resident vector (prove_witness).  A bad one raises r1csqap.WitnessError before anything is proved."""
    dev = resident(S, circuit, pk)
    dw = capi.scalars_upload(host_scalars(S, w, "witness"))
    try:
        report = (r1cs if check_r1cs is None else check_r1cs).CheckWitness(dw, cap=16)
        if not report:
            report._witness = w
            raise r1csqap.WitnessError(report)
        return prove(S, "prove_witness", dev, r1cs, dw, rs)
    finally:
        dw.free()


def generate_from_inputs(S, circuit, pk, r1cs, plan, inputs, rs=()):
    """From the input values to the proof without a host witness: the witness is solved on the device (plan: r1csqap.SolvePlan of
    `r1cs`, made once per circuit by r1cs.PlanSolve), checked against ALL constraints -- the plan's check rows are examined by nothing
    else --, and proved from the same resident vector.  r1csqap.SolveError when variables stay unsolved or a divisor was zero,
    r1csqap.WitnessError when the solved witness breaks a constraint; nothing is proved then."""
    dev = resident(S, circuit, pk)
    (dw,), report = plan.Solve([list(inputs)])
    try:
        if not report:
            raise r1csqap.SolveError(report)
        check = r1cs.CheckWitness(dw, cap=16)
        if not check:
            raise r1csqap.WitnessError(check)
        return prove(S, "prove_witness", dev, r1cs, dw, rs)
    finally:
        dw.free()


class Prover:
    """Submit / Collect / Close over one resident key: up to MaxInFlight host-buffer tickets, proofs back in submission order.
    A subclass names its `scheme` and gives _submit its public face."""
    MaxInFlight = 3
    scheme = None

    def __init__(self, circuit, pk, dev_r1cs=None):
        self.dev = resident(self.scheme, circuit, pk)
        self.r1cs = dev_r1cs
        self.tickets, self.done = [], []

    def _collect_oldest(self):
        self.done.append(prove_end(self.scheme, self.tickets.pop(0)))

    def _submit(self, w, px, rs=()):
        S = self.scheme
        if px is None and self.r1cs is None:
            raise ValueError("this prover has no resident R1CS: Submit needs px")
        wa = host_scalars(S, w, "witness")
        pa = None if px is None else host_scalars(S, px, "px")
        while True:
            if len(self.tickets) >= self.MaxInFlight:
                self._collect_oldest()
            try:
                t = prove_witness_host_begin(S, self.dev, self.r1cs, wa, rs) if pa is None else prove_host_begin(S, self.dev, wa, pa, rs)
            except capi.GosnarkHipError as e:
                if e.code == GS_ERR_BUSY and self.tickets:       # another prover shares the device's slots: make room and retry
                    self._collect_oldest()
                    continue
                raise
            self.tickets.append(t)
            return

    def InFlight(self):
        return len(self.tickets) + len(self.done)

    def Collect(self):
        if not self.done:
            if not self.tickets:
                raise ValueError("Collect without a submitted proof")
            self._collect_oldest()
        return self.done.pop(0)

    def Close(self):
        for t in self.tickets:
            capi.ticket_cancel(t)
        self.tickets, self.done = [], []


# ---- one proof over several devices or ranks ------------------------------------------------------------------------------------
def partials(S, op, pk, w, third, shard_index, shard_count):
    """op: prove_partials, prove_partials_values -> (words, infinity flags) of this rank's sums."""
    out, inf = capi.result(*S.partials)
    call(S.prefix + op, raw(pk), raw(w), raw(third), shard_index, shard_count, ptr64(out), inf)
    return out, inf


def partials_begin(S, op, pk, w, third, shard_index, shard_count):
    return call_ticket(S, op, raw(pk), raw(w), raw(third), shard_index, shard_count)


def partials_end(S, ticket):
    out, inf = capi.result(*S.partials)
    call(S.prefix + "partials_end", ticket, ptr64(out), inf)
    return out, inf


def witness_values(S, pk, r1cs, w, hv_handle=None):
    cell, bad = capi.HandleCell(hv_handle), ctypes.c_uint32(0)
    call(S.prefix + "witness_values", raw(pk), raw(r1cs), raw(w), cell.ref, ctypes.byref(bad))
    return cell.result(), int(bad.value)


def prove_multi(S, op, pks, ws, thirds, rs=()):
    """op: prove_multi, prove_multi_values -> (Proof, used_rccl)."""
    out, inf = capi.result(*S.proof)
    used = ctypes.c_int(0)
    call(S.prefix + op, harr(pks), harr(ws), harr(thirds), len(pks), *_rs(S, rs), ptr64(out), inf, ctypes.byref(used))
    return S.decode(out, inf), bool(used.value)


def prove_batch(S, pk_of_device, ws, pxs, rs_pairs=()):
    n = len(ws)
    words, flags = S.proof
    out, inf = capi.result(words, flags, rows=max(n, 1))
    out = out.reshape(-1, words)
    rs = []
    if S.has_rs:          # one limb row per proof for r, then for s
        rs = [capi.ints_to_u64([p[i] % capi.R for p in rs_pairs]) if n else np.zeros((1, 4), dtype=np.uint64) for i in (0, 1)]
    call(S.prefix + "prove_batch", harr(pk_of_device), len(pk_of_device), harr(ws), harr(pxs), n, *map(ptr64, rs), ptr64(out), inf)
    return [S.decode(out[i], inf[flags * i:flags * (i + 1)]) for i in range(n)]


# ---- keys -----------------------------------------------------------------------------------------------------------------------
def shard(S, pk, shard_index, shard_count, target_device=None):
    cell = capi.HandleCell()
    if target_device is None:
        call(S.prefix + "pk_shard", raw(pk), shard_index, shard_count, cell.ref)
    else:
        call(S.prefix + "pk_shard_to", raw(pk), shard_index, shard_count, int(target_device), cell.ref)
    return S.DevicePk(cell.result(), pk.nvars, pk.npublic)


def set_basis(S, which, pk, points_u64, *domain):
    """gs_*_pk_set_eval / _set_quot / _set_eval_domain: upload [n, 12] uint64 Jacobian points and attach them (None detaches)."""
    b = None if points_u64 is None else capi.g1_upload(points_u64)
    call(S.prefix + "pk_set_" + which, raw(pk), raw(b), *domain)
    if b is not None:
        b.free()


def derive_basis(S, which, pk, *n):
    call(S.prefix + "pk_derive_" + which, raw(pk), *n)


def export_words(S, pk, which, count, shape):
    out = np.zeros(shape, dtype=np.uint64)
    call(S.prefix + "pk_export", raw(pk), which, ptr64(out), count)
    return out


def export_array(S, pk, which):
    """Array `which` of S.arrays as [count, 12 | 24] uint64 Jacobian limbs."""
    count = (capi.pk_eval_count(pk) if which == S.eval_array else capi.pk_quot_count(pk) if which == S.quot_array else
             pk.nvars - 1 if which == S.h_array else pk.nvars)
    shape = (count, 24 if which == S.g2_array else 12)
    return export_words(S, pk, which, count, shape) if count else np.zeros(shape, dtype=np.uint64)


def ExportPkArray(S, pk, name):
    a = export_array(S, pk, S.arrays[name])
    return capi.g2_tuples(a) if a.shape[1] == 24 else capi.g1_tuples(a)


def setup(S, n, nvars, npublic, csrs, toxic, vk_words):
    """gs_*_setup on a sparse R1CS with the toxic scalars injected -> (DevicePk, the verification key's words as ints)."""
    capi.init()
    tox = capi.ints_to_u64([t % capi.R for t in toxic]).reshape(-1)
    vk = np.zeros(vk_words, dtype=np.uint64)
    cell = capi.HandleCell()
    call(S.prefix + "setup", n, nvars, npublic, *capi.csr_args(csrs), ptr64(tox), cell.ref, ptr64(vk))
    return S.DevicePk(cell.result(), nvars, npublic), capi.u64_to_ints(vk)


def g1_at(v, o):
    return (v[o], v[o + 1], v[o + 2])


def g2_at(v, o):
    return ((v[o], v[o + 1]), (v[o + 2], v[o + 3]), (v[o + 4], v[o + 5]))


def verify_inputs(vk, publicSignals):
    """What both VerifyProof marshal alike: vk.IC and the public signals (the reference indexes vk.IC[i + 1] for every signal)."""
    if len(vk.IC) < len(publicSignals) + 1:
        raise IndexError("index out of range: %d public signals, vk.IC has %d points" % (len(publicSignals), len(vk.IC)))
    ic = capi.g1_points_to_u64(vk.IC)
    pub = capi.ints_to_u64([int(x) % capi.R for x in publicSignals]) if publicSignals else np.zeros((1, 4), dtype=np.uint64)
    return ptr64(ic), len(vk.IC), ptr64(pub), len(publicSignals)
