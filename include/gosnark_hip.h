/* gosnark_hip.h -- C ABI of libgosnark_hip.so: the MI355X (gfx950) prover hot path of
 * arnaucube/go-snark-study.
 *
 * The reference has no FFI or plugin seam (pure Go on math/big); the drop-in boundary is the
 * pair of Go functions
 *     groth16.GenerateProofs(circuit, pk, w, px) (Proof, error)     groth16/groth16.go:225-278
 *     snark.GenerateProofs  (circuit, pk, w, px) (Proof, error)     snark.go:254-289
 * plus the finer seams they are built from (bn128/g1.go:140 MulScalar + :32 Add loops,
 * bn128/g2.go:142/:32, r1csqap/r1csqap.go:57-216).  A cgo binding (go/gosnarkhip, shown in
 * INTEGRATION.md) flattens the Go structs and calls the entry points below; each entry point
 * cites the reference code it replaces.
 *
 * Conventions
 *  - Field elements (Fq and Fr): 4 x uint64_t little-endian limbs, STANDARD (non-Montgomery)
 *    form, i.e. exactly big.Int.Bits() of the reference value padded to 4 words.  Scalars and
 *    polynomial coefficients may be any value < 2^256; they are reduced mod r on the device.
 *  - G1 points: Jacobian triples [X, Y, Z] = 12 words, as the reference stores them
 *    ([3]*big.Int, bn128/g1.go:9-12).  G2 points: [[X0,X1],[Y0,Y1],[Z0,Z1]] = 24 words
 *    ([3][2]*big.Int, bn128/g2.go:9-12).  Z == 0 means infinity (g1.go:28-30).
 *  - Results are returned in AFFINE normal form [x, y, 1] (g1.go:157-170 / g2.go:183-200) with
 *    an is-infinity flag; the reference's raw Jacobian Z depends on its exact double/add order
 *    and cannot be reproduced by a bucket method.  Infinity is [0, 0, 0].
 *  - Every function returns 0 on success or a negative gs_status; gs_last_error() gives the
 *    message (thread-local).  Nothing falls back to a CPU path: without a usable gfx950
 *    device every prover/setup/polynomial/MSM call fails with GS_ERR_NO_DEVICE.  (The verifier
 *    entry points at the end are host code by design -- O(1) pairings -- and say so.)
 *  - The library copies caller buffers during the call and never retains host pointers
 *    (cgo pointer rule).  Device memory lives behind opaque handles freed by gs_free().
 *  - One context per LOGICAL DEVICE: gs_init takes a list of HIP ordinals and creates one context -- streams, workspaces,
 *    handle table, lock -- per entry (the same ordinal may appear several times).  A handle or ticket carries its logical
 *    device in its top byte, so every entry point that takes one runs on the right device whatever thread calls it; entry
 *    points that only CREATE objects (uploads, fixed-base batches, setups, the gs_poly_* family) use the calling thread's current
 *    logical device (gs_set_device, default 0; a Go caller wraps the pair in runtime.LockOSThread).  Calls on one logical
 *    device are serialised on its lock and are safe from any number of goroutines/threads; different logical devices run
 *    concurrently.  While pipelined tickets (gs_*_begin) are outstanding, every other call still works: uploads, downloads,
 *    gs_free (deferred until the tickets that read the object are collected) and gs_r1cs_px proceed at once, the rest
 *    first wait for the outstanding device work -- they queue, they do not fail.
 */
#ifndef GOSNARK_HIP_H
#define GOSNARK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)
#endif

typedef uint64_t gs_handle;

typedef enum {
  GS_OK = 0,
  GS_ERR_NO_DEVICE = -1,   /* no gfx950 device / HIP runtime unusable */
  GS_ERR_HIP = -2,         /* a HIP call or kernel failed */
  GS_ERR_ARG = -3,         /* bad argument (null pointer, size mismatch, bad handle) */
  GS_ERR_SHAPE = -4,       /* instance violates the reference's shape contract */
  GS_ERR_NOT_INIT = -5,
  GS_ERR_BUSY = -6         /* gs_*_begin: all three in-flight slots of this logical device are taken -- collect one with gs_*_end and retry */
} gs_status;

/* ---- lifetime ------------------------------------------------------------------------- */
/* Create one context per entry of `devices` (HIP ordinals, 1 <= ndev <= 64): "logical device" i drives devices[i].  One
 * process per GPU passes one entry; a single Go process that drives a whole node passes all eight ("one stream +
 * context per (goroutine, device)"); listing one ordinal N times gives N logical devices that time-slice that GPU (how the
 * multi-device entry points below are tested on a 1-GPU box).  Calling it again with the same list is a no-op; a different
 * list needs gs_shutdown first.  gs_shutdown releases everything, on every device. */
int gs_init(const int* devices, int ndev);
void gs_shutdown(void);
/* Number of logical devices; the calling thread's current one (objects are created there); the device a handle/ticket lives on. */
int gs_device_count(void);
int gs_set_device(int logical_device);
int gs_get_device(void);
int gs_handle_device(gs_handle h);
const char* gs_last_error(void);
/* ABI/version string, e.g. "gosnark-hip 0.1 gfx950". */
const char* gs_version(void);
int gs_free(gs_handle h);

/* ---- resident base-point arrays (proving-key material) --------------------------------- */
/* Upload n Jacobian points, convert to Montgomery affine on the device (x = X/Z^2, y = Y/Z^3,
 * bn128/g1.go:157-170), keep them resident.  Replaces the per-call big.Int traffic of
 * pk.G1.At / pk.G1.BACGamma / pk.BACDelta / pk.PowersTauDelta (groth16.go:15-32).
 * Every finite point must satisfy its curve equation (y^2 = x^3 + 3; on the twist y^2 = x^3 + 3/(9+u)): otherwise
 * GS_ERR_ARG, naming the first offender (the reference never checks and would sum garbage). */
int gs_g1_upload(const uint64_t* jacobian /* n x 12 */, size_t n, gs_handle* out);
/* Same for G2 arrays, e.g. pk.G2.BACGamma (groth16.go:29), snark Pk.B (snark.go:19). */
int gs_g2_upload(const uint64_t* jacobian /* n x 24 */, size_t n, gs_handle* out);
/* Number of points behind a base handle, coefficients behind a scalar handle, or At entries a Groth16 key (slice) holds. */
int gs_len(gs_handle h, size_t* out);
/* Read points back as affine Jacobian triples [x, y, 1] / [0,0,0] (testing / serialisation). */
int gs_g1_download(gs_handle bases, uint64_t* jacobian /* n x 12 */, size_t n);
int gs_g2_download(gs_handle bases, uint64_t* jacobian /* n x 24 */, size_t n);

/* Fixed-base batch: out[i] = k[i] * G  for the G1 / G2 generator (bn128.go:52-83); the hot
 * loop of groth16.GenerateTrustedSetup (groth16.go:139-175, `MulScalar(Utils.Bn.G1.G, ...)`)
 * and what the synthetic proving keys of bench.py are built with. */
int gs_g1_fixed_base(const uint64_t* scalars /* n x 4 */, size_t n, gs_handle* out);
int gs_g2_fixed_base(const uint64_t* scalars /* n x 4 */, size_t n, gs_handle* out);

/* ---- resident scalar vectors ------------------------------------------------------------- */
int gs_scalars_upload(const uint64_t* scalars /* n x 4 */, size_t n, gs_handle* out);
int gs_scalars_download(gs_handle scalars, uint64_t* out /* n x 4 */, size_t n);
/* Overwrite a resident vector IN PLACE with n = its length new scalars (a server's next witness into the handle of an earlier one):
 * no hipMalloc, no hipFree -- gs_scalars_upload + gs_free per proof costs both, and hipFree synchronises the whole device under the
 * outstanding tickets.  The copy is ordered behind every device read of the vector that pipelined operations enqueued before the
 * call and has landed when the call returns.  With four vectors rotating under three tickets it never waits.
 * One exception to "a ticket has read its inputs when the update returns": a WITNESS ticket on a key with an evaluation-basis array
 * (gs_*_prove_witness_begin) whose witness violates a constraint is proved again, on the exact route, when it is COLLECTED -- from the
 * resident vector as it is then.  A caller that may submit unsatisfying witnesses must not update a vector before the ticket that
 * reads it has been collected (host-buffer tickets own their copy and are not affected). */
int gs_scalars_update(gs_handle scalars, const uint64_t* values /* n x 4 */, size_t n);

/* Copies of [off, off + n) of a resident vector / base array onto another logical device (device-to-device; across xGMI
 * when the two are different GPUs).  How the shards of a term range are handed to the devices that will sum them. */
int gs_scalars_clone(gs_handle scalars, size_t off, size_t n, int target_device, gs_handle* out);
int gs_g1_clone(gs_handle bases, size_t off, size_t n, int target_device, gs_handle* out);
int gs_g2_clone(gs_handle bases, size_t off, size_t n, int target_device, gs_handle* out);

/* ---- multi-scalar multiplication ----------------------------------------------------------
 * out = sum_{i<n} scalars[i] * bases[off + i]: replaces the loop
 *     acc = G1.Add(acc, G1.MulScalar(bases[i], scalars[i]))
 * of groth16.go:243-250,269-271 / snark.go:265-286 (bn128/g1.go:140-155 + :32-89) by a signed-
 * digit Pippenger bucket method.  out_affine = [x, y] (8 words); *is_inf set when the sum is
 * the identity (then out is all zero). */
int gs_msm_g1(gs_handle bases, const uint64_t* scalars /* n x 4 */, size_t off, size_t n,
              uint64_t out_affine[8], int* is_inf);
/* G2 flavour (bn128/g2.go:142-181 + :32-89); out_affine = [x0, x1, y0, y1] (16 words). */
int gs_msm_g2(gs_handle bases, const uint64_t* scalars /* n x 4 */, size_t off, size_t n,
              uint64_t out_affine[16], int* is_inf);
/* Same with the scalars already resident (handle from gs_scalars_upload / a poly result);
 * soff = first scalar used.  This is what bench.py times. */
int gs_msm_g1_resident(gs_handle bases, size_t off, gs_handle scalars, size_t soff, size_t n,
                       uint64_t out_affine[8], int* is_inf);
int gs_msm_g2_resident(gs_handle bases, size_t off, gs_handle scalars, size_t soff, size_t n,
                       uint64_t out_affine[16], int* is_inf);
/* Pipelined form (everything resident): begin enqueues one MSM and returns a ticket, gs_msm_end waits for that MSM only and
 * writes the affine result (8 words for a G1 ticket, 16 for G2).  Three operations may be outstanding (MSM or proof tickets);
 * the sort of MSM k+1 runs under the accumulation of MSM k and its accumulation starts the moment that one ends. */
int gs_msm_g1_begin(gs_handle bases, size_t off, gs_handle scalars, size_t soff, size_t n, uint64_t* ticket);
int gs_msm_g2_begin(gs_handle bases, size_t off, gs_handle scalars, size_t soff, size_t n, uint64_t* ticket);
int gs_msm_end(uint64_t ticket, uint64_t* out_affine, int* is_inf);
/* Sum of n points given as affine [x,y] pairs with infinity flags (multi-GPU combine of the
 * per-rank partial sums): out = sum_i pts[i]. */
int gs_g1_sum_affine(const uint64_t* pts /* n x 8 */, const int* inf, size_t n, uint64_t out_affine[8], int* is_inf);
int gs_g2_sum_affine(const uint64_t* pts /* n x 16 */, const int* inf, size_t n, uint64_t out_affine[16], int* is_inf);

/* ---- polynomial field over Fr (r1csqap/r1csqap.go) ---------------------------------------- */
/* PolynomialField.Mul (r1csqap.go:57-67): out has na + nb - 1 coefficients. */
int gs_poly_mul(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out);
/* PolynomialField.Div (r1csqap.go:70-84): quotient (na - nb + 1 coefficients) and, if rem is
 * not NULL, remainder (nb - 1 coefficients).  Requires na >= nb >= 1 and b[nb-1] != 0. */
int gs_poly_div(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* quo, uint64_t* rem);
/* PolynomialField.Add / Sub (r1csqap.go:94-115): out has max(na, nb) coefficients. */
int gs_poly_add(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out);
int gs_poly_sub(const uint64_t* a, size_t na, const uint64_t* b, size_t nb, uint64_t* out);
/* PolynomialField.Eval (r1csqap.go:118-126). */
int gs_poly_eval(const uint64_t* v, size_t n, const uint64_t x[4], uint64_t out[4]);
/* PolynomialField.LagrangeInterpolation (r1csqap.go:150-158): n values at nodes 1..n ->
 * n coefficients.  Mathematically exact for every n (the reference's NewPolZeroAt overflows a
 * Go int for n >= 22, r1csqap.go:130-136; equal results for n <= 21). */
int gs_lagrange_interpolation(const uint64_t* values, size_t n, uint64_t* coeffs);
/* Z(x) = prod_{i=1}^{deg} (x - i): deg + 1 coefficients (r1csqap.go:177-186, groth16.go:122-131). */
int gs_zpoly(size_t deg, uint64_t* out);
/* Sparse R1CS -> P(x): the scalable replacement of R1CSToQAP + CombinePolynomials
 * (r1csqap.go:161-210).  A, B, C in CSR over n constraints x m variables (row_ptr n+1,
 * col idx, val nnz x 4); w: m scalars.  Outputs ax, bx, cx (n coeffs each, may be NULL) and
 * px = ax*bx - cx (2n - 1 coeffs).
 * What a matrix may contain (here, in gs_r1cs_upload and in both setups): a row holds any number of entries, 0 .. 2^32 - 1 in
 * all; its column indices need not be sorted, and an index may occur more than once -- repeated (row, column) entries ADD;
 * every value, and every witness entry, is any 256-bit integer and counts mod r (outputs are canonical).  Only an index >= m
 * or a row_ptr that is not monotone from 0 is refused (GS_ERR_ARG).  tests/test_gpu_r1cs_shapes.py holds each of these. */
int gs_r1cs_to_px(size_t n, size_t m,
                  const uint32_t* a_rowptr, const uint32_t* a_col, const uint64_t* a_val,
                  const uint32_t* b_rowptr, const uint32_t* b_col, const uint64_t* b_val,
                  const uint32_t* c_rowptr, const uint32_t* c_col, const uint64_t* c_val,
                  const uint64_t* w, uint64_t* ax, uint64_t* bx, uint64_t* cx, uint64_t* px);

/* The same split per circuit / per proof: gs_r1cs_upload validates and keeps A, B, C resident (free with gs_free);
 * gs_r1cs_px turns a resident witness (gs_scalars_upload, m elements) into the resident px (2n - 1 coefficients: pass
 * *px_inout = 0 to create the vector, or the handle of an earlier call to overwrite it) -- nothing crosses PCIe, and the
 * result feeds gs_groth16_prove_resident / gs_groth16_prove_begin directly.  gs_last_timing().poly_ms = device time. */
int gs_r1cs_upload(size_t n, size_t m,
                   const uint32_t* a_rowptr, const uint32_t* a_col, const uint64_t* a_val,
                   const uint32_t* b_rowptr, const uint32_t* b_col, const uint64_t* b_val,
                   const uint32_t* c_rowptr, const uint32_t* c_col, const uint64_t* c_val, gs_handle* out);
int gs_r1cs_px(gs_handle r1cs, gs_handle w, gs_handle* px_inout);
/* Which constraints does a witness break?  gs_r1cs_check needs no key and proves nothing: r1cs is a handle of gs_r1cs_upload or
 * gs_r1cs_upload_domain, w a resident scalar vector of exactly m elements (any 256-bit words, counted mod r).
 *   *nviolated                   the number of rows j < n with (A w)_j (B w)_j != (C w)_j mod r;
 *   rows[0 .. min(cap, count))   the violated rows, 0-based, ascending: the FIRST cap of them;
 *   values[i] (3 x 4 words)      (A w)_j, (B w)_j, (C w)_j of j = rows[i], canonical standard form; values may be NULL.
 * Entries at and beyond min(cap, count) are not written; cap = 0 (rows may then be NULL) only counts.
 * WHAT IS EXAMINED: all n rows of the system.  This is not the prover's criterion: the violated-constraint count of the witness
 * routes (gs_timing.fallbacks, *violated of gs_*_witness_values) looks at the deg Z roots of the KEY's Z, so for the reference's
 * m = n + 1 shape, where Z has n - 1 roots and the key does not enforce constraint n, the prover counts 0 for
 * a witness that breaks only the last row and this call still reports row n - 1.  The padded rows n .. 2^k - 1 of a domain system
 * are never reported.
 * Exact for every system the uploads accept and at any n: rows of more than 512 entries are summed by a workgroup each, up to 4096
 * of them per matrix and the rest by one thread each (slower, the same sums); the positions are exact prefix sums of one word per row.
 * Errors, nothing written: a product system (gs_r1cs_upload_zkey) is GS_ERR_SHAPE -- a .zkey key's system holds no C, and the check
 * needs the three matrices of circuit.r1cs --, and so is a w that does not have m elements; a handle of another kind or of another
 * logical device than r1cs's, a null nviolated, cap > 0 with null rows: GS_ERR_ARG; no device: GS_ERR_NOT_INIT.  No host fallback.
 * Blocking, but it does NOT wait for outstanding tickets: it works in buffers of its own on the stream of the polynomial stages, beside
 * the accumulations of the proofs in flight, and waits only for its own work; a gs_scalars_update of w after it returns is safe.
 * gs_last_timing(): poly_ms = the values stage (copy, Montgomery conversion, three sparse products), reduce_ms = flags, prefix sums
 * and gather, total_ms = all device time of the call including the result copies. */
int gs_r1cs_check(gs_handle r1cs, gs_handle w, size_t cap, uint64_t* nviolated, uint32_t* rows /* cap, may be NULL iff cap = 0 */,
                  uint64_t* values /* cap x 3 x 4 words, may be NULL */);
/* Solving witnesses FROM the system.  For the systems the reference's compiler emits every row holds one flattened gate whose `out`
 * sits alone in C (or alone in A / B for a division), so each row defines one new signal from earlier ones: a sparse triangular
 * solve, wide where circuits are wide and independent over the witnesses of one circuit.
 * gs_r1cs_solve_plan builds the level plan ONCE per (system, input variables) on the host (csrc/solve_plan.h holds the definition:
 * known_0 = {0} + inputs; level l takes every unused row with exactly one distinct variable outside known_(l-1) whose summed
 * coefficient is nonzero in exactly one matrix; lowest row wins a tie; rows left over whose variables all became known are CHECKS,
 * which the solve does not examine -- gs_r1cs_check does).  input_vars: ninputs distinct variables in 1 .. m-1 (variable 0 is the
 * constant one), in the order gs_r1cs_solve's values come in.  opts (may be NULL; a 0 field means the default of csrc/knobs.h):
 * levels narrower than `narrow` rows merge into sequential runs of at most `run_max_rows` rows, one launch each; every other level
 * is one launch.  *stats is optional.  The plan handle keeps its system alive; gs_free releases it.  The system's matrices are read
 * back from the device once, here.
 * gs_r1cs_solve_unsolved: *count = how many variables no row defines; vars[0 .. min(cap, count)) = the first of them, ascending.
 * gs_r1cs_solve: nwit witnesses in one set of launches.  inputs[b][k] (4 words, any 256-bit value, counted mod r) is input_vars[k] of
 * witness b.  w_inout[b]: 0 to create a vector of m elements, or a resident vector of exactly m elements to overwrite (the call
 * first waits for the reads pipelined operations still have on it, like gs_scalars_update).  Result: canonical standard form in
 * [0, r) -- what gs_scalars_upload of the integers would hold --, unsolved variables 0.  A row whose divisor is zero for a witness
 * stores 0 for that witness and goes on: nfailed[b] counts such rows, first_failed_row[b] is the first of them in solve order
 * (0xFFFFFFFF = none); both arrays are required and the call still returns GS_OK.
 * A row of more than 512 entries is walked by one thread: slow, the same sums.
 * Errors, nothing written (no output, no vector): a product system (gs_r1cs_upload_zkey) is GS_ERR_SHAPE, in gs_r1cs_check's words;
 * an input variable that is 0, >= m or listed twice, a handle of another kind, a null argument, nwit = 0: GS_ERR_ARG; an overwrite
 * vector that does not hold m elements: GS_ERR_SHAPE; no device: GS_ERR_NOT_INIT.  No host fallback.
 * Blocking, but like gs_r1cs_check it does not wait for outstanding tickets: the stream of the polynomial stages, workspaces of its own.
 * gs_last_timing(): h2d_ms = the inputs' copy, poly_ms = the level and run launches, total_ms = all device time of the call. */
typedef struct {
  uint32_t narrow;                  /* levels of fewer rows merge into runs; 0 = default */
  uint32_t run_max_rows;            /* a run is cut every so many rows; 0 = default */
} gs_solve_opts;
typedef struct {
  uint64_t solved;                  /* rows that define a variable = variables solved */
  uint64_t unsolved;                /* variables no row defines (inputs and variable 0 are not counted) */
  uint64_t checks;                  /* rows that define nothing and whose variables are all known */
  uint64_t stuck;                   /* rows with a variable that stays unsolved */
  uint64_t levels;
  uint64_t launches;                /* wide launches + runs */
  uint64_t wide_launches;
  uint64_t widest_level;            /* rows */
} gs_solve_stats;
int gs_r1cs_solve_plan(gs_handle r1cs, const uint32_t* input_vars, size_t ninputs, const gs_solve_opts* opts /* may be NULL */,
                       gs_handle* plan, gs_solve_stats* stats /* may be NULL */);
int gs_r1cs_solve_unsolved(gs_handle plan, size_t cap, uint32_t* vars /* cap, may be NULL iff cap = 0 */, uint64_t* count);
int gs_r1cs_solve(gs_handle plan, size_t nwit, const uint64_t* inputs /* nwit x ninputs x 4 words */, gs_handle* w_inout /* nwit */,
                  uint64_t* nfailed /* nwit */, uint32_t* first_failed_row /* nwit */);
int gs_solve_abi_sizes(size_t* opts_bytes, size_t* stats_bytes);
/* The same sparse system as a QAP over a POWER-OF-TWO DOMAIN -- what snarkjs / circom Groth16 keys (proving_key.json: polsA/B/C, A,
 * B1, B2, C, hExps) are built on.  m = 2^log2_domain, 1 <= log2_domain <= 27, n <= m constraints; omega = 5^((r-1)/m); row c of the
 * system sits at omega^c (rows n .. m-1 are empty); ax, bx, cx are the interpolants of degree < m, Z = x^m - 1, and
 * H = floor((ax bx - cx) / Z) = coefficients m .. 2m-2 of px.  Same CSR rules and validation as gs_r1cs_upload.  The handle is accepted
 * by gs_r1cs_px (px has 2m - 1 coefficients: one transform per polynomial, no subproduct tree) and by every Groth16 witness entry point
 * (gs_groth16_prove_r1cs, gs_groth16_prove_witness, _witness_begin, _witness_host_begin, _witness_host) -- together with a FULL key whose
 * Z is exactly x^m - 1 for the same m and whose PowersTauDelta (hExps) holds at least m - 1 points: anything else is GS_ERR_SHAPE, and
 * so are Pinocchio keys, key slices and the multi-device entry points (gs_*_witness_values, *_values).  gs_r1cs_to_px stays nodes-only.
 * The root convention is confirmed against snarkjs for log2_domain = 2 (the reference's externalVerif/circom-test fixture) and is the
 * same formula above that.
 * COSET EVALUATION BASIS.  With g = 5^((r-1)/(2m)), y_j = g omega^j and T = PowersTauDelta[0..m):
 *     sum_j (ax bx - cx)(y_j) E[j] = sum_i h_i T[i]    for    E[j] = -(1/(2m)) sum_{i<m} y_j^(-i) T[i]    (Z(y_j) = -2 for every j),
 * so a key that holds E (m G1 points, natural order j <-> y_j) proves a witness with three forward and three inverse transforms of size
 * m and one point-wise kernel: no product of size 2m, no division; the violated-constraint count is read when the proof is collected and a
 * non-zero count repeats the proof on the exact route (px, floor quotient), as for the node basis.  gs_groth16_pk_derive_eval_domain
 * computes E from the key's PowersTauDelta alone -- ONE transform of size m carried out in the group, m + m/2 log2 m scalar
 * multiplications, once per key, blocking, explicit only; GS_ERR_SHAPE unless the key's Z is x^(2^log2_domain) - 1.
 * gs_groth16_pk_set_eval_domain attaches an array from a file (not checked against tau, as gs_groth16_pk_set_eval);
 * gs_groth16_pk_export which = 7 reads it back; gs_handle_bytes / gs_memory_query account for it like the node basis.  A key holds ONE
 * evaluation-basis array: the route is taken only when the array's basis matches the R1CS of the call; gs_set_eval_basis(0) closes it. */
int gs_r1cs_upload_domain(size_t log2_domain, size_t n, size_t m,
                          const uint32_t* a_rowptr, const uint32_t* a_col, const uint64_t* a_val,
                          const uint32_t* b_rowptr, const uint32_t* b_col, const uint64_t* b_val,
                          const uint32_t* c_rowptr, const uint32_t* c_col, const uint64_t* c_val, gs_handle* out);
int gs_groth16_pk_derive_eval_domain(gs_handle pk, size_t log2_domain);
int gs_groth16_pk_set_eval_domain(gs_handle pk, gs_handle bases, size_t log2_domain);

/* ---- zkey: the binary files circom / snarkjs write today ---------------------------------------- */
/* A circuit.zkey is not a re-encoding of proving_key.json: it has NO C matrix (the prover takes c_j = a_j b_j on the domain), NO
 * monomial h array (section 9 is the coset evaluation basis E above), and its numbers are in machine form already.  Four entry points
 * take its sections as they lie in the file -- e.g. memory-mapped; caller memory of any alignment, staged through the pinned buffers
 * like gs_g1_upload -- and convert on the device.  (go-snark-study_amd/circom.py parses the container; no file written by snarkjs itself has been
 * read yet, so the container layout is the parser's concern and these entry points do not depend on it.)
 *
 * gs_g1_upload_affine_mont / gs_g2_upload_affine_mont: n affine points, G1 as x | y, G2 as x.c0 | x.c1 | y.c0 | y.c1, every coordinate 32
 * little-endian bytes of value * 2^256 mod q; all-zero bytes are the point at infinity.  One Montgomery product by a constant per
 * coordinate.  A coordinate >= q and a point off its curve are GS_ERR_ARG with the first offending index.  The result is an ordinary
 * base-array handle.
 *
 * gs_r1cs_upload_zkey: `coefs` = the ncoefs 44-byte records of section 4 (u32 matrix: 0 = A, 1 = B; u32 row < 2^log2_domain;
 * u32 signal < nvars; 32 bytes of value * 2^512 mod r), any order, repeated (matrix, row, signal) add up.  The CSR arrays of A and B are
 * built on the device (count, scan, scatter); a record out of range is GS_ERR_ARG with its index.  The handle is a domain R1CS that is a
 * PRODUCT SYSTEM: it has no C matrix, the third value vector is a_j b_j (one point-wise kernel), there is nothing to check -- the
 * violated-constraint count is 0, gs_timing.fallbacks stays 0, and a wrong witness gives a proof the verifier rejects, as in snarkjs.
 * Every Groth16 witness entry point and gs_r1cs_px accept it, on the coset route and (with a key that has PowersTauDelta) on the px route;
 * Pinocchio, key slices and the multi-device values routes refuse it like any domain R1CS.
 *
 * gs_groth16_pk_create_domain: the arrays and points of gs_groth16_pk_create, with `h_coset` = the 2^log2_domain points of E in place of
 * PowersTauDelta; Z = x^m - 1 is built inside.  The result is a COSET-ONLY key: it proves from a witness with a domain R1CS of the same
 * log2_domain (product system or not) on the evaluation-basis route, and has no other route and no fallback.  Whatever needs
 * PowersTauDelta is GS_ERR_SHAPE ("the key holds the coset evaluation basis only"): gs_groth16_prove* with px, gs_groth16_prove_r1cs, a
 * witness call after gs_set_eval_basis(0), gs_groth16_pk_derive_quot / _derive_eval* / _set_quot / _set_eval, gs_groth16_pk_shard*.
 * gs_groth16_pk_export which = 4 has 0 points, which = 7 the m points of E. */
int gs_g1_upload_affine_mont(const void* bytes /* n x 64 */, size_t n, gs_handle* out);
int gs_g2_upload_affine_mont(const void* bytes /* n x 128 */, size_t n, gs_handle* out);
int gs_r1cs_upload_zkey(size_t log2_domain, size_t nvars, const void* coefs /* ncoefs x 44 */, size_t ncoefs, gs_handle* out);
int gs_groth16_pk_create_domain(gs_handle g1_at, gs_handle g1_bacgamma, gs_handle g2_bacgamma, gs_handle bacdelta, gs_handle h_coset,
                                const uint64_t g1_alpha[12], const uint64_t g1_beta[12], const uint64_t g1_delta[12],
                                const uint64_t g2_beta[24], const uint64_t g2_delta[24], size_t log2_domain, size_t nvars, size_t npublic,
                                gs_handle* out);

/* ---- setup from a transcript: circuit.r1cs + a powers-of-tau file -> the arrays of a circuit.zkey ---------------------------------- */
/* gs_groth16_setup takes the toxic scalars; whoever holds a real powers-of-tau transcript holds POINTS (tau^i G, alpha tau^i G, ..) and
 * not tau, so the two halves of `snarkjs groth16 setup` are carried out in the group.  All arithmetic is exact, every addition is the
 * complete one (a transcript or a basis may hold infinities, equal and opposite points), all results are ordinary base-array handles of
 * affine points.  Blocking; GS_ERR_ARG for a bad handle or a value out of range, GS_ERR_SHAPE for arrays that do not fit each other.
 *
 * gs_g1_lagrange / gs_g2_lagrange: one inverse transform of n = 2^log2_n points P[off ..] in the group, w = 5^((r-1)/n), v = 5^((r-1)/(2n)):
 *     odd_half = 0:  out[j] = (1/n)  sum_{i<n}  w^(-ij)      P[off+i]       0 <= log2_n <= 27, needs n points from off
 *     odd_half = 1:  out[j] = (1/2n) sum_{i<2n} v^(-(2j+1)i) P[off+i]       1 <= log2_n <= 27, needs 2n - 1 or 2n points from off
 *                                                                           (a missing P[off+2n-1] is the point at infinity)
 * n points out, natural order.  With P[i] = tau^i G the first is the Lagrange basis L_j(tau) G of the domain of the n-th roots of unity
 * (row j of a domain R1CS sits at w^j); the second -- the odd entries of the transform of size 2n, computed as ONE transform of size n
 * over P[i] - P[i+n] -- is the coset evaluation basis of section 9 of a .zkey for delta = 1.  m + (m/2) log2 m scalar multiplications
 * each (G1: 4-bit windows; G2: the same window, its 16-point table in private memory).  gs_g2_lagrange is the odd_half = 0 form.
 *
 * gs_r1cs_colsum_g1 / _g2: out[s] = sum_j a_js Ba[j] + b_js Bb[j] + c_js Bc[j] for every variable s < nvars of a resident R1CS
 * (gs_r1cs_upload, gs_r1cs_upload_domain, gs_r1cs_upload_zkey): the column sums of the sparse matrices over basis points.  A basis handle
 * of 0 leaves its matrix out; a basis holds at least as many points as the system has rows; a product system (no C matrix) with
 * basis_c != 0 is GS_ERR_SHAPE.  The matrix rules are those of gs_r1cs_upload: unsorted indices, repeated (row, column) entries add, any
 * 256-bit value counts mod r.  A coefficient of 1 or r - 1 costs one addition; any other v is multiplied through
 * min(bitlen(v mod r), bitlen(r - v mod r)) bits; columns of any length are summed by a segmented reduction in levels of 16 terms, so no
 * column is one thread's loop.  At most 2^28 - 1 terms per call.  nvars points out.
 *
 * gs_g1_scale: out[i] = k P[i] for any 256-bit k (a phase-2 contribution multiplies C and H by 1 / delta).
 * gs_g1_download_affine_mont / gs_g2_download_affine_mont: the first n points of a base array in the encoding gs_g*_upload_affine_mont
 * reads (the bytes of a .zkey section); `bytes` may be a writable memory map of the output file.
 * go-snark-study_amd/circom.py (SetupFromPtau, ContributeDelta) drives them from circuit.r1cs and a .ptau file. */
int gs_g1_lagrange(gs_handle powers, size_t off, size_t log2_n, int odd_half, gs_handle* out);
int gs_g2_lagrange(gs_handle powers, size_t off, size_t log2_n, gs_handle* out);
int gs_r1cs_colsum_g1(gs_handle r1cs, gs_handle basis_a, gs_handle basis_b, gs_handle basis_c, gs_handle* out);
int gs_r1cs_colsum_g2(gs_handle r1cs, gs_handle basis_a, gs_handle basis_b, gs_handle basis_c, gs_handle* out);
int gs_g1_scale(gs_handle bases, const uint64_t k[4], gs_handle* out);
int gs_g1_download_affine_mont(gs_handle bases, void* bytes /* n x 64 */, size_t n);
int gs_g2_download_affine_mont(gs_handle bases, void* bytes /* n x 128 */, size_t n);

/* ---- contributing to a transcript: one phase-1 (powers-of-tau) contribution on the points ---------------------------------------- */
/* A contribution multiplies a new secret into a transcript whose tau nobody knows: tauG1[i] *= tau^i, tauG2[i] *= tau^i,
 * alphaTauG1[i] *= alpha tau^i, betaTauG1[i] *= beta tau^i, betaG2 *= beta -- an array of points by a geometric series of scalars.
 *
 * gs_g1_scale_powers / gs_g2_scale_powers: out = a new base array of n points, out[i] = (c t^i mod r) P[off + i].  c and t are any
 * 256-bit values and count mod r; t^0 = 1 also for t = 0 (out[0] = c P[off], every later point is infinity); t = 1 is a uniform scale
 * (the G2 twin gs_g1_scale lacks); n = 0 gives an empty array; off + n beyond the array is GS_ERR_SHAPE, a bad handle or a null pointer
 * GS_ERR_ARG.  The series is built on the device, so the n scalars never exist on the host; one kernel launch reads the affine points,
 * multiplies each through 4-bit windows (256 doublings and at most 64 + 14 general additions, the 16-point table in private memory)
 * and writes affine points (one field inversion per point).  Every addition is the complete one: the input may
 * hold infinities, equal and opposite points, and every scalar including 0 is legal.  A caller that streams a long section in slabs
 * passes c t^s for the slab that starts at index s.  Blocking; gs_last_timing().total_ms = device time.
 * go-snark-study_amd/circom.py (ContributePtau) drives them over a .ptau file; go/gosnarkhip/ptau.go and tests/c/ptau_contribute.c are the same sequence. */
int gs_g1_scale_powers(gs_handle bases, size_t off, size_t n, const uint64_t c[4], const uint64_t t[4], gs_handle* out);
int gs_g2_scale_powers(gs_handle bases, size_t off, size_t n, const uint64_t c[4], const uint64_t t[4], gs_handle* out);

/* ---- checking a key and a transcript: is this .zkey the key of THIS circuit over THIS transcript? ------------------------------- */
/* Every array of a Groth16 key is a linear image of the transcript's points, so a random linear combination of a section equals a
 * combination of transcript points whose scalars come out of the circuit alone: the prover's own pipeline with a challenge vector in the
 * witness's place (sparse rows times a vector, values -> coefficients, MSM).  Only scalars go through a transform; the group work is
 * about a dozen table-free MSMs and two pairing products, against the five transforms in the group of a second setup.
 *
 * Notation: m = 2^log2_domain; M' = (A', B', C') the circuit's system with the rows nConstraints + s = (signal s, 1), s <= npublic,
 * appended to A' (what the setup sums over); rho_i = s^(i+1), i < nvars, and sigma_j = s^(j+1), j < m, for the challenge s (made on
 * the device); rho^pub = rho with the entries i > npublic zeroed, rho^prv = rho - rho^pub; p_X(x) = the m coefficients of the
 * interpolant of X' x on the domain (row j at w^j, w = 5^((r-1)/m)).  Every check has a left point from the key and a right point
 * from circuit and transcript:
 *
 *   0 coefs A   A_key rho                         A' rho                             the value vectors are equal, A_key / B_key = the
 *   1 coefs B   B_key rho                         B' rho                             key's own section 4 (lhs[0] = rows that differ)
 *   2 A         MSM(A, rho)                       MSM(tauG1[0..m), p_A(rho))         equal points
 *   3 B1        MSM(B1, rho)                      MSM(tauG1[0..m), p_B(rho))         equal points
 *   4 B2        MSM(B2, rho)                      MSM(tauG2[0..m), p_B(rho))         equal points (G2)
 *   5 IC        MSM(IC, rho[0..npublic])          K(rho^pub)                         equal points
 *   6 C         MSM(C, rho[npublic+1..])          K(rho^prv)                         e(lhs, delta2) = e(rhs, G2)
 *   7 H         MSM(H, sigma)                     MSM(tauG1[0..m), c) - MSM(tauG1[m..m+cnt), c[0..cnt))     e(lhs, delta2) = e(rhs, G2)
 *
 * with K(x) = MSM(betaTauG1, p_A(x)) + MSM(alphaTauG1, p_B(x)) + MSM(tauG1, p_C(x)), and for H: c_t = (1/2) v^(-t) q_t, q = the
 * coefficients of the interpolant of sigma, v = 5^((r-1)/(2m)); cnt = m when the transcript holds 2m or more tauG1 points and m - 1
 * otherwise.  That is gs_g1_lagrange's odd_half form read as a transposed map: H_j = (1/2m) sum_{i<2m} v^(-(2j+1)i) tau^i G / delta,
 * so the coefficient of tau^i G in sum_j sigma_j H_j delta is (1/2) v^(-i) q_(i mod m), and v^m = -1 gives c_(t+m) = -c_t; a missing
 * tauG1[2m-1] is the point at infinity, as there -- a key set up from a transcript of exactly 2m - 1 points and one set up from a longer
 * transcript differ in H, and each passes against its own transcript only.
 *
 * SOUNDNESS is Schwartz-Zippel over the challenge: both sides of every check are polynomials in s of degree at most max(nvars, 2m), so a
 * wrong key passes for at most max(nvars, 2m) values of s out of r ~ 2^254.  The caller draws s AFTER the key, the circuit and the
 * transcript are fixed (go-snark-study_amd/circom.py: VerifyZkey).  WHAT THIS PROVES: the key's arrays are the ones a setup of this circuit over this
 * transcript yields, scaled by the delta of its header.  WHAT IT DOES NOT: who contributed to the transcript or to delta -- the
 * contribution chain of a ceremony (challenge hashes, proofs of knowledge) is out of scope; and the header points themselves (alpha1,
 * beta1, beta2, gamma2, delta1 against delta2) are a few host comparisons and one pairing product that the caller makes (VerifyZkey).
 *
 * Handles: a, b1, b2 (nvars points), ic (npublic + 1), c (nvars - npublic - 1: section 8 as it lies in the file), h (m): the key's
 * arrays from gs_g1_upload_affine_mont / gs_g2_upload_affine_mont; key_system: gs_r1cs_upload_zkey of the key's section 4;
 * circuit_system: gs_r1cs_upload_domain of M'; tau_g1 (at least 2m - 1 points), tau_g2, alpha_tau_g1, beta_tau_g1 (at least m).
 * delta2: a Jacobian triple, standard form; it must be a point of the order-r subgroup (the rule of gs_pairing_check), else C and H fail.
 * Every MSM of the check is summed TABLE-FREE whatever the table policy -- each array is used once -- and after the call none of the
 * handles owns a window table (one it had is released); the call leaves no device memory behind except caches gs_trim frees.
 * Blocking; gs_last_timing has the device time (plan_ms, accumulate_ms, reduce_ms of the MSMs, poly_ms = the scalar side).
 * GS_ERR_SHAPE when the handles do not fit each other, GS_ERR_ARG for a bad handle or s = 0 mod r.
 *
 * gs_ptau_check: the same machinery on the transcript itself, for its first N = 2^log2_n powers (2N - 1 of tauG1), rho_i = s^(i+1):
 *   0 g1          tauG1[0]                        G1                                 equal points
 *   1 g2          tauG2[0]                        G2                                 equal points
 *   2 tau         tauG1[1]                        tauG2[1]                           e(lhs, G2) = e(G1, rhs)
 *   3 tauG1       sum_{i<2N-2} rho_i tauG1[i]     sum rho_i tauG1[i+1]               e(lhs, tauG2[1]) = e(rhs, G2)
 *   4 tauG2       sum_{i<N-1} rho_i tauG2[i]      sum rho_i tauG2[i+1]               e(tauG1[1], lhs) = e(G1, rhs)
 *   5 alphaTauG1  sum_{i<N-1} rho_i alphaTauG1[i] sum rho_i alphaTauG1[i+1]          e(lhs, tauG2[1]) = e(rhs, G2)
 *   6 betaTauG1   the same over betaTauG1
 *   7 betaG2      betaTauG1[0]                    betaG2                             e(lhs, G2) = e(G1, rhs)
 * Together: tauG1[i] = tau^i G1, tauG2[i] = tau^i G2 for ONE tau, alphaTauG1 and betaTauG1 are geometric with that ratio, and betaG2 has
 * betaTauG1[0]'s scalar.  The shifted sums are one MSM plan over two offsets of the resident array.  Soundness as above with degree 2N.
 *
 * Results: a point is affine, standard form, G1 in words 0..7 (x | y), G2 in words 0..15 (x.c0 | x.c1 | y.c0 | y.c1), zero at infinity.
 * gs_check_report is written through the caller's pointer: gs_check_abi_sizes tells a binding of another revision before it passes a
 * short buffer. */
#define GS_CHECK_MAX 8
enum { GS_KEY_COEFS_A = 0, GS_KEY_COEFS_B, GS_KEY_A, GS_KEY_B1, GS_KEY_B2, GS_KEY_IC, GS_KEY_C, GS_KEY_H };
enum { GS_PTAU_G1 = 0, GS_PTAU_G2, GS_PTAU_TAU, GS_PTAU_TAU_G1, GS_PTAU_TAU_G2, GS_PTAU_ALPHA_TAU_G1, GS_PTAU_BETA_TAU_G1, GS_PTAU_BETA_G2 };
typedef struct {
  int32_t ok;                       /* 1 = the check passed */
  int32_t lhs_g2, rhs_g2;           /* which group each point lives in */
  int32_t lhs_inf, rhs_inf;
  int32_t reserved;
  uint64_t lhs[16], rhs[16];
} gs_check_result;
typedef struct {
  uint32_t nchecks;                 /* entries of `check` in use */
  uint32_t failed;                  /* bit i set: check i failed */
  gs_check_result check[GS_CHECK_MAX];
} gs_check_report;
typedef struct {
  gs_handle a, b1, b2, ic, c, h;                        /* the key's arrays (sections 5, 6, 7, 3, 8, 9) */
  gs_handle key_system, circuit_system;
  gs_handle tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1;  /* the transcript (sections 2 .. 5) */
  uint64_t delta2[24];
  uint64_t challenge[4];                                /* s, any 256-bit value, not 0 mod r */
  uint64_t log2_domain, npublic;
} gs_key_check_input;
int gs_groth16_key_check(const gs_key_check_input* in, gs_check_report* out);
int gs_ptau_check(gs_handle tau_g1, gs_handle tau_g2, gs_handle alpha_tau_g1, gs_handle beta_tau_g1, const uint64_t beta_g2[24], size_t log2_n,
                  const uint64_t challenge[4], gs_check_report* out);
int gs_check_abi_sizes(size_t* input_bytes, size_t* report_bytes);

/* ---- preparing a transcript for phase 2: the Lagrange bases of every power-of-two domain ----------------------------------------- */
/* `snarkjs powersoftau prepare phase2` appends to a transcript, per array section, the Lagrange basis of EVERY domain 2^0 .. 2^top: a
 * setup then reads the level of its domain and runs no transform.  Level p of a section P is gs_g*_lagrange(P, 0, p, 0) of its first 2^p
 * points: level[p][j] = (1/2^p) sum_{i<2^p} w_p^(-ij) P[i], w_p = 5^((r-1)/2^p), natural order.
 *
 * gs_g1_lagrange_levels / gs_g2_lagrange_levels: out = a new base array of 2^(hi+1) - 2^lo affine points, level p (lo <= p <= hi) at
 * index 2^p - 2^lo.  The levels share one workspace and the decimation-in-time stage of span h has the same twiddles at every level, so
 * ONE launch carries that stage for all levels with 2^p >= 2h: hi stage launches instead of sum (p + 1) -- below about 2^17 butterflies a
 * stage does not fill the chip and costs one scalar multiplication's latency however small it is.  The array holds at least 2^hi points,
 * or exactly 2^hi - 1: then the missing last point of level hi is the point at infinity (tauG1 has 2^(power+1) - 1 points and its top
 * level is power + 1); fewer is GS_ERR_SHAPE.  lo > hi, hi > 27, a bad handle or a null `out` is GS_ERR_ARG.  All arithmetic is exact
 * and every addition the complete one.  Blocking; gs_last_timing().total_ms = device time.
 *
 * gs_g1_lagrange_levels_check / gs_g2_lagrange_levels_check: are the first 2^(hi+1) - 1 points of `levels` the levels 0 .. hi of
 * `powers` (at least 2^hi points, or 2^hi - 1 with the rule above)?  No transform runs in the group: with rho_i = s^(i+1) over the
 * section index i,
 *     lhs = MSM(levels, rho)          rhs = MSM(powers, c),   c_i = sum_p [i < 2^p] (coefficient i of the interpolant of rho's slice for
 *                                                                   level p on the domain of w_p: the 2^(-p) is the interpolation's own)
 * and the check is lhs = rhs as points (gs_ptau_check's machinery: only scalars go through a transform, both sums are table-free and
 * the handles own no window table afterwards).  *out is ONE gs_check_result.  s = 0 mod r or a bad handle is GS_ERR_ARG, arrays too
 * short GS_ERR_SHAPE; hi <= 25, since a sum takes at most 2^26 - 1 terms and the levels 0 .. hi are 2^(hi+1) - 1 (GS_ERR_ARG above).
 * SOUNDNESS: lhs - rhs = sum_i s^(i+1) D_i for the differences D_i = levels[i] - (what level i should be), a polynomial in s of degree at
 * most 2^(hi+1) with point coefficients.  In G1 every point has order r, so a wrong section passes for at most 2^(hi+1) values of s out
 * of r ~ 2^254.  In G2 that bound holds for differences INSIDE the order-r subgroup only: the twist's cofactor is not prime, and a
 * difference of small order t escapes whenever the combination of the powers of s it meets vanishes mod t -- for a single wrong point of
 * order t, whenever t divides s^(i+1), i.e. with probability about 1 / (the product of t's prime factors): no 2^-230 event -- see
 * gs_g2_subgroup_check below, which closes that case.  The levels of a checked transcript are sums
 * of subgroup points and lie in the subgroup, so whoever needs this for a section of unknown origin runs gs_g2_subgroup_check over its
 * points first (gs_ptau_check has the same case for tauG2 and the key check for B2; circom.py: membership=True does it for all three).
 * go-snark-study_amd/circom.py (PreparePtau, VerifyPtauPrepared, SetupFromPtau(prepared=True)) drives them over a .ptau file; go/gosnarkhip/ptau.go
 * and tests/c/ptau_prepare.c are the same sequence. */
int gs_g1_lagrange_levels(gs_handle powers, size_t lo, size_t hi, gs_handle* out);
int gs_g2_lagrange_levels(gs_handle powers, size_t lo, size_t hi, gs_handle* out);
int gs_g1_lagrange_levels_check(gs_handle powers, gs_handle levels, size_t hi, const uint64_t challenge[4], gs_check_result* out);
int gs_g2_lagrange_levels_check(gs_handle powers, gs_handle levels, size_t hi, const uint64_t challenge[4], gs_check_result* out);

/* ---- G2 subgroup membership of whole arrays -------------------------------------------------------------------------------------- */
/* The twist E'(Fq2) has r (2q - r) points and the cofactor 2q - r = 10069 x (a 246-bit number with no factor below 3 x 10^6): a point that
 * satisfies the curve equation -- all that the uploads test -- need not have order r.  The random linear combinations of gs_ptau_check,
 * gs_g2_lagrange_levels_check and gs_groth16_key_check bound a wrong point's chance by 2^-230 only INSIDE the subgroup; a point
 * tau^j G2 + S with S of order 10069 passes them about once in 10069 challenges.  No linear combination can do better: the map
 * phi = psi - [6 x^2] that vanishes exactly on the subgroup sends S into a group whose order has the factor 10069, so a combination of
 * images still vanishes once in about 10069 challenges.  The test has to be per point, and exact.
 *
 * gs_g2_subgroup_check: tests the points off .. off + n - 1 of a G2 base array (from gs_g2_upload, gs_g2_upload_affine_mont or any
 * entry that returns one).  *nbad = how many lie outside the order-r subgroup; *first_bad = the smallest index of one, counted from
 * the start of the ARRAY (not from off), UINT64_MAX when there is none.  The point at infinity is a member.  n = 0 is legal (0 and
 * UINT64_MAX); off + n beyond the array is GS_ERR_SHAPE; a bad handle, a handle of another kind or a null out-pointer GS_ERR_ARG.
 * One thread per point evaluates [x + 1] Q + psi([x] Q) + psi^2([x] Q) = psi^3([2x] Q) for the BN parameter x and the
 * untwist-Frobenius-twist endomorphism psi: 62 doublings and 23 mixed additions along the fixed non-adjacent form of x (no lane of a
 * wave diverges), three general additions, no inversion -- about a quarter of the field products of gs_g2_scale_powers over the same
 * points.  Every addition is the complete one.  The call reads the affine array only: it builds no window table and leaves no device
 * memory behind.  Blocking; gs_last_timing().total_ms = device time.  G1 needs no such call: its cofactor is 1.
 * go-snark-study_amd/circom.py (VerifyPtau, VerifyPtauPrepared, VerifyZkey with membership=True) runs it on the arrays the other checks
 * upload; go/gosnarkhip/g2_membership.go and tests/c/g2_membership.c are the plain call. */
int gs_g2_subgroup_check(gs_handle points, size_t off, size_t n, uint64_t* nbad, uint64_t* first_bad);

/* ---- compressed points: an x coordinate and a sign bit <-> a resident array of affine points -------------------------------------- */
/* A point on the wire is usually its x coordinate and one bit that says which of the two roots of y^2 = x^3 + b is meant: 32 bytes for
 * G1, 64 for G2, 128 for a Groth16 proof.  Getting y back is a square root in Fq (one power with a 252-bit exponent, q = 3 mod 4) or
 * in Fq2 (two such powers, the complex method, no inversion): go-snark-study_amd/csrc/sqrt.h.
 *
 * Coordinates here are 4 little-endian 64-bit words in STANDARD form, not Montgomery -- the form of the gs_g*_upload triples -- and an
 * Fq2 coordinate is c0 | c1.  Byte order and flag positions of a wire format are the host codec's business
 * (go-snark-study_amd/compressed.py: gnark, arkworks, the bn256 pairing crate); the device never sees a wire format.  One flag byte per
 * point:
 *   GS_POINT_LARGEST_Y   y is the LARGER of {y, q - y} as canonical integers; in Fq2 decided by c1, and by c0 only when c1 = 0
 *   GS_POINT_INFINITY    the point at infinity; x must be 0 and GS_POINT_LARGEST_Y clear
 * y = 0 cannot occur: a point with y = 0 has order 2 and both curves have odd order, so "larger" never ties.
 *
 * gs_g1_decompress / gs_g2_decompress: one lane per point computes y = sqrt(x^3 + 3) (G1) or sqrt(x^3 + 3/(9 + u)) (the twist), takes
 * the root the flag asks for and writes an ordinary affine base array of n points into *out -- every entry point that takes a base
 * array takes it.  An entry is BAD when a coordinate is >= q, when the right-hand side has no root, when GS_POINT_INFINITY comes with
 * x != 0 or with GS_POINT_LARGEST_Y, or when any flag bit above bit 1 is set.  A bad entry becomes the point at infinity and gets
 * ok[i] = 0 (a good one 1); the call still returns GS_OK -- unlike the uploads, which refuse a whole array for one point off the curve:
 * one malformed proof must not sink a batch.  ok may be NULL.  *nbad = how many entries are bad, *first_bad = the smallest index of
 * one, UINT64_MAX when there is none.  n = 0 gives an empty array.
 * gs_g2_decompress does NOT test subgroup membership: the result is on the twist, not necessarily in G2.  Run gs_g2_subgroup_check on
 * the handle where that matters (the pairing entry points require it).  G1 has cofactor 1.
 *
 * gs_g1_compress / gs_g2_compress: the points off .. off + n - 1 of a resident array -> x (n x 4 or n x 8 words) and flags (n bytes);
 * a point at infinity gives x = 0 and GS_POINT_INFINITY.
 *
 * A bad handle, a handle of the other group or a null pointer is GS_ERR_ARG, a range beyond the array GS_ERR_SHAPE.  All four calls
 * are blocking; gs_last_timing().total_ms = device time of the kernel.  No window table is built and no device memory is left behind
 * but the array of gs_g*_decompress.  go/gosnarkhip/point_codec.go and tests/c/point_codec.c are the plain call sequence. */
#define GS_POINT_LARGEST_Y 1u
#define GS_POINT_INFINITY  2u
int gs_g1_decompress(const uint64_t* x /* n x 4 */, const uint8_t* flags /* n */, size_t n,
                     gs_handle* out, uint8_t* ok /* n, or NULL */, uint64_t* nbad, uint64_t* first_bad);
int gs_g2_decompress(const uint64_t* x /* n x 8: c0 | c1 */, const uint8_t* flags, size_t n,
                     gs_handle* out, uint8_t* ok, uint64_t* nbad, uint64_t* first_bad);
int gs_g1_compress(gs_handle bases, size_t off, size_t n, uint64_t* x /* n x 4 */, uint8_t* flags /* n */);
int gs_g2_compress(gs_handle bases, size_t off, size_t n, uint64_t* x /* n x 8 */, uint8_t* flags);

/* ---- Groth16 prover (groth16/groth16.go) --------------------------------------------------- */
/* Device-resident proving key: groth16.Pk (groth16.go:15-32).  At, BACGamma (G1), BACDelta:
 * m points; G2 BACGamma: m points; PowersTauDelta: len(Z) points; single points as Jacobian
 * triples; Z: nz coefficients (monic).  npublic = circuit.NPublic. */
int gs_groth16_pk_create(gs_handle g1_at, gs_handle g1_bacgamma, gs_handle g2_bacgamma,
                         gs_handle bacdelta, gs_handle powers_tau_delta,
                         const uint64_t g1_alpha[12], const uint64_t g1_beta[12], const uint64_t g1_delta[12],
                         const uint64_t g2_beta[24], const uint64_t g2_delta[24],
                         const uint64_t* z, size_t nz, size_t nvars, size_t npublic, gs_handle* out);
/* groth16.GenerateProofs (groth16.go:225-278) with the randomness injected: r, s are what
 * Utils.FqR.Rand() would have returned (:231-238).  out_proof = PiA [x,y] (8 words) |
 * PiB [x0,x1,y0,y1] (16) | PiC [x,y] (8); inf[3] flags.  Requires len(w) == nvars and
 * npx - nz + 1 <= len(PowersTauDelta) (the reference indexes PowersTauDelta[i] for
 * i < len(hx), :269-271). */
int gs_groth16_prove(gs_handle pk, const uint64_t* w, size_t nw, const uint64_t* px, size_t npx,
                     const uint64_t r[4], const uint64_t s[4], uint64_t out_proof[32], int inf[3]);
/* Same with w and px already resident (gs_scalars_upload); what bench.py times. */
int gs_groth16_prove_resident(gs_handle pk, gs_handle w, gs_handle px,
                              const uint64_t r[4], const uint64_t s[4], uint64_t out_proof[32], int inf[3]);

/* Sparse R1CS + witness -> proof in ONE call (CombinePolynomials r1csqap.go:191-210 on the resident sparse system, then
 * GenerateProofs groth16.go:225-278): px is computed on the stream H(x) waits on, while the main stream already accumulates the
 * four sums over w, which do not need px.  *px_inout as in gs_r1cs_px (0 = create; px stays available to the caller).
 * Same proof as gs_r1cs_px followed by gs_groth16_prove_resident. */
int gs_groth16_prove_r1cs(gs_handle pk, gs_handle r1cs, gs_handle w, gs_handle* px_inout, const uint64_t r[4], const uint64_t s[4],
                          uint64_t out_proof[32], int inf[3]);

/* Witness -> proof WITHOUT px: H(x) = (A(x) B(x) - C(x)) / Z(x) is computed straight from the constraint values A w, B w, C w
 * (their values at the nodes n+1..2n by one batched convolution, ONE interpolation instead of three, a Taylor shift; no size-2n
 * product, no division) -- the fast form of CombinePolynomials + DivisorPolynomial (r1csqap.go:191-216) for a witness that
 * satisfies the R1CS, which is the only case in which a proof means anything.  If a constraint is violated the call falls back to
 * the exact route and returns what gs_groth16_prove_r1cs returns.  Same proof as gs_r1cs_px + gs_groth16_prove_resident. */
int gs_groth16_prove_witness(gs_handle pk, gs_handle r1cs, gs_handle w, const uint64_t r[4], const uint64_t s[4],
                             uint64_t out_proof[32], int inf[3]);
/* Keys with an EVALUATION-BASIS copy of PowersTauDelta take a shorter way still.  The prover only needs the group element
 * sum_i h_i PowersTauDelta[i] = H(tau) Z(tau)/delta G (groth16.go:139-149, 269-271); with E[j-1] = l_j(tau) Z(tau)/delta G, l_j the
 * Lagrange basis over the nodes n+1..2n (n = #constraints), the same element is sum_j H(n+j) E[j-1] -- an MSM over the VALUES of H,
 * which fall out of the one batched convolution: no interpolation, no Taylor shift, no host wait (the violated-constraint count
 * is read when the proof is collected; a non-zero count repeats the proof on the exact route).  gs_groth16_setup builds E while it
 * knows tau (64 B per constraint + its window table; gs_handle_bytes reports both); gs_groth16_pk_set_eval attaches one to a key
 * loaded from a file (`bases`: n G1 points from gs_g1_upload; nobody can check them against tau -- a wrong array yields proofs that
 * do not verify, as a wrong PowersTauDelta does); gs_groth16_pk_export which = 7 reads it back.  Bit-identical proofs either way.
 * gs_groth16_prove_witness_begin is the pipelined form (collect with gs_groth16_prove_end; same three slots per device). */
int gs_groth16_pk_set_eval(gs_handle pk, gs_handle bases);
int gs_pk_eval_count(gs_handle pk, size_t* count);     /* Groth16 or Pinocchio key: evaluation-basis points it holds (0 = none) */
int gs_groth16_prove_witness_begin(gs_handle pk, gs_handle r1cs, gs_handle w, const uint64_t r[4], const uint64_t s[4], uint64_t* ticket);
/* Keys with a QUOTIENT-BASIS array divide nothing by Z.  h = floor(px / Z) is linear in px and only ever enters the proof through
 * sum_j h_j PowersTauDelta[j]; with D = deg Z, g = 1 / rev(Z) as a power series and Q[m] = sum_{d <= m} g_d PowersTauDelta[m - d]
 * (m < len(PowersTauDelta)) that element is sum_{m < len(hx)} px[D + m] Q[m] for every px, whatever the remainder: ONE MSM over the top
 * coefficients of px as they are -- no transforms, no hx.  Every entry point that is handed px (or builds it: gs_groth16_prove_r1cs)
 * takes this route when the key holds the array; the witness routes above and px shorter than Z are as before.  gs_groth16_setup builds
 * Q (64 B per point; the key then keeps no window table of PowersTauDelta for these routes, so its table bytes do not grow);
 * gs_groth16_pk_set_quot attaches one to a key loaded from a file (`bases`: len(PowersTauDelta) G1 points; not checked -- a wrong array
 * yields proofs that do not verify) and bases = 0 detaches it; gs_groth16_pk_export which = 10 reads it back.  Key slices
 * (gs_groth16_pk_create_shard / gs_groth16_pk_shard) carry no such array and divide.  Bit-identical proofs either way; the environment
 * variable GS_NO_QUOT_BASIS (any value, read once) makes every key divide. */
int gs_groth16_pk_set_quot(gs_handle pk, gs_handle bases);
int gs_pk_quot_count(gs_handle pk, size_t* count);     /* Groth16 or Pinocchio key: quotient-basis points it holds (0 = none) */
/* Compute the quotient-basis array of a key that was built elsewhere (only T = PowersTauDelta is known): Q is the convolution of
 * the scalar series g with the point sequence T, by a number-theoretic transform carried out in the group (csrc/ecntt.hip):
 * N / 2 * log2 N + N scalar multiplications for N = 2^ceil(log2(2 len(T) - 1)) -- seconds for a 2^20 key, once per key; explicit
 * only, nothing derives the array on its own.  Blocking; replaces an attached array. */
int gs_groth16_pk_derive_quot(gs_handle pk);
/* Compute the evaluation-basis array of a key that was built elsewhere, from its PowersTauDelta alone, and attach it as
 * gs_groth16_pk_set_eval would:  E[j-1] = sum_{i < n} coeff_i(l_j) PowersTauDelta[i], l_j the Lagrange basis over the nodes n+1..2n --
 * the transposed Vandermonde system  sum_j E[j-1] (n+j)^i = PowersTauDelta[i], solved by pushing the point sequence down a subproduct
 * tree with the transforms carried out in the group (csrc/ecntt.hip): about 0.75 n log2^2 n + 2 n log2 n scalar multiplications, once
 * per key.  n_constraints cannot be read off the key: it is len(Z) when nvars = n + 1 and len(Z) - 1 when nvars = n + 2, and at most
 * len(PowersTauDelta); anything else is GS_ERR_SHAPE.  Full keys only.  Explicit only, nothing derives the array on its own.
 * Blocking; replaces an attached array. */
int gs_groth16_pk_derive_eval(gs_handle pk, size_t n_constraints);

/* Pipelined proving (inputs resident): gs_groth16_prove_begin enqueues the whole device side of one proof and returns a
 * ticket without waiting; gs_groth16_prove_end waits for THAT proof only, then runs the host tail and writes the proof
 * (same layout as gs_groth16_prove).  At most three tickets (proofs or MSMs) may be outstanding per logical device (a fourth begin returns
 * GS_ERR_BUSY); they own disjoint workspaces, so the plan and
 * bucket accumulations of proof k+1 run while the reduction tails, result download and host tail of proof k are still in
 * progress.  Other entry points stay usable meanwhile (see "Conventions"): the key and the vectors a ticket reads may even be
 * gs_free'd -- they are released when the ticket has been collected. */
int gs_groth16_prove_begin(gs_handle pk, gs_handle w, gs_handle px, const uint64_t r[4], const uint64_t s[4], uint64_t* ticket);
int gs_groth16_prove_end(uint64_t ticket, uint64_t out_proof[32], int inf[3]);
/* HOST-BUFFER TICKETS: the reference's own call shape -- groth16.GenerateProofs(circuit, pk, w, px) gets a NEW w (and px) in host
 * memory with every call (groth16/groth16.go:225; cli/main.go:480-501 computes them per proof) -- at the pipelined rate.  The
 * arrays are staged into device buffers that the ticket's SLOT owns (grow-only: once the three slots have been used a stream of
 * proofs performs no hipMalloc and no hipFree, see gs_alloc_counters) on a copy stream of their own: the PCIe transfer of proof
 * k + 3 runs beside the accumulations of proofs k + 1 and k + 2, and the call enqueues the proof once the copy has landed (measured:
 * cheaper than a cross-stream event; the device is busy with the tickets before this one meanwhile).  The caller's arrays have been
 * consumed when the call returns.  Collect with gs_groth16_prove_end; same three slots per device.
 *   gs_groth16_prove_host_begin          w and px from the host (32 + 64 MiB at 2^20 constraints)
 *   gs_groth16_prove_witness_host_begin  w only, against a resident sparse R1CS (gs_r1cs_upload): the witness routes above
 *   gs_groth16_prove_witness_host        the blocking form of the latter (the upload is part of the call, as in gs_groth16_prove) */
int gs_groth16_prove_host_begin(gs_handle pk, const uint64_t* w, size_t nw, const uint64_t* px, size_t npx, const uint64_t r[4], const uint64_t s[4],
                                uint64_t* ticket);
int gs_groth16_prove_witness_host_begin(gs_handle pk, gs_handle r1cs, const uint64_t* w, size_t nw, const uint64_t r[4], const uint64_t s[4],
                                        uint64_t* ticket);
int gs_groth16_prove_witness_host(gs_handle pk, gs_handle r1cs, const uint64_t* w, size_t nw, const uint64_t r[4], const uint64_t s[4],
                                  uint64_t out_proof[32], int inf[3]);
/* Abandon a ticket of any kind (proof or MSM) without collecting its result: waits for its device work, frees its slot and the
 * references it holds.  An error path that cannot call the matching _end must call this, or the slot stays occupied. */
int gs_ticket_cancel(uint64_t ticket);

/* One proof over several GPUs: every rank holds the key (or just its slice of it, below) and the resident w / px, takes shard `shard_index` of
 * `shard_count` of the term ranges (contiguous, first ranges one longer when they do not divide), computes H(x) locally
 * (the polynomial stage is replicated) and returns its five raw MSM sums as affine points:
 * out_sums = At (8 words) | G1.BACGamma (8) | G2.BACGamma (16) | BACDelta (8) | PowersTauDelta.h (8); inf[5] in that order.
 * The ranks exchange these 416-byte records (ncclAllGather as bytes), add them with gs_g1_sum_affine / gs_g2_sum_affine
 * and call gs_groth16_finish, which applies the O(1) tail of groth16.go:253-275. */
int gs_groth16_prove_partials(gs_handle pk, gs_handle w, gs_handle px, size_t shard_index, size_t shard_count,
                              uint64_t out_sums[48], int inf[5]);
/* Key slices: a rank that only ever runs gs_groth16_prove_partials for shard `shard_index` of `shard_count` needs only that
 * shard's entries of the proving key ("each GPU holds 1/8 of every pk array").  gs_groth16_pk_create_shard takes
 * base handles that hold exactly the slices -- At / G1.BACGamma / G2.BACGamma / BACDelta entries of the contiguous split of
 * [0, nvars), PowersTauDelta entries of the split of [0, nptd_total) (first ranges one longer when they do not divide; the
 * same split gs_groth16_prove_partials uses) -- plus the single elements and Z, which every rank keeps.
 * gs_groth16_pk_shard cuts such a slice out of a resident full key (then gs_free the full key).  A slice key is accepted
 * by gs_groth16_prove_partials (with its own shard), gs_groth16_finish and gs_groth16_pk_export; every other entry point
 * refuses it.  Window tables are built for the slice only: 1/shard_count of the key memory per GPU. */
int gs_groth16_pk_create_shard(gs_handle g1_at, gs_handle g1_bacgamma, gs_handle g2_bacgamma, gs_handle bacdelta, gs_handle ptd,
                               const uint64_t g1_alpha[12], const uint64_t g1_beta[12], const uint64_t g1_delta[12],
                               const uint64_t g2_beta[24], const uint64_t g2_delta[24], const uint64_t* z, size_t nz,
                               size_t nvars, size_t npublic, size_t nptd_total, size_t shard_index, size_t shard_count,
                               gs_handle* out);
int gs_groth16_pk_shard(gs_handle full_pk, size_t shard_index, size_t shard_count, gs_handle* out);
/* The same slice, created on logical device `target_device` (the full key may live on any device). */
int gs_groth16_pk_shard_to(gs_handle full_pk, size_t shard_index, size_t shard_count, int target_device, gs_handle* out);
int gs_groth16_finish(gs_handle pk, const uint64_t sums[48], const int inf_in[5], const uint64_t r[4], const uint64_t s[4],
                      uint64_t out_proof[32], int inf[3]);

/* groth16.GenerateTrustedSetup (groth16.go:94-222) for a SPARSE R1CS (A, B, C in CSR over n constraints x m
 * variables, as gs_r1cs_to_px), with the five toxic scalars injected (what Utils.FqR.Rand() returned at :99-119):
 * toxic = T | Kalpha | Kbeta | Kgamma | Kdelta (5 x 4 words).  Builds the proving key directly on the device --
 * Lagrange basis at tau over the nodes 1..n, transposed sparse mat-vecs for the per-variable evaluations, fixed-base
 * batch multiplications -- and returns it resident in *pk_out (same object as gs_groth16_pk_create).  If vk_out is not
 * NULL it receives the verification key as affine Jacobian triples: G1.Alpha (12 words) | G2.Beta (24) | G2.Gamma (24)
 * | G2.Delta (24) | IC[0..npublic] (12 each).  Shape contract: m in {n+1, n+2}. */
int gs_groth16_setup(size_t n, size_t m, size_t npublic,
                     const uint32_t* a_rowptr, const uint32_t* a_col, const uint64_t* a_val,
                     const uint32_t* b_rowptr, const uint32_t* b_col, const uint64_t* b_val,
                     const uint32_t* c_rowptr, const uint32_t* c_col, const uint64_t* c_val,
                     const uint64_t toxic[20], gs_handle* pk_out, uint64_t* vk_out);
/* snark.GenerateTrustedSetup (snark.go:98-251) for a sparse R1CS; toxic = T | Ka | Kb | Kc | Kbeta | Kgamma | RhoA | RhoB
 * (8 x 4 words; RhoC = RhoA RhoB, :149).  *pk_out: resident Pinocchio key (as gs_pinocchio_pk_create builds).  vk_out
 * (may be NULL), affine Jacobian triples: Vka (24 words, G2) | Vkb (12) | Vkc (24) | G1Kbg (12) | G2Kbg (24) | G2Kg (24)
 * | Vkz (24) | IC[0..npublic] (12 each). */
int gs_pinocchio_setup(size_t n, size_t m, size_t npublic,
                       const uint32_t* a_rowptr, const uint32_t* a_col, const uint64_t* a_val,
                       const uint32_t* b_rowptr, const uint32_t* b_col, const uint64_t* b_val,
                       const uint32_t* c_rowptr, const uint32_t* c_col, const uint64_t* c_val,
                       const uint64_t toxic[32], gs_handle* pk_out, uint64_t* vk_out);
/* Read one array of a resident Pinocchio key back (which = 0 A, 1 Ap, 2 B (G2, 24 words per point), 3 Bp, 4 C, 5 Cp,
 * 6 Kp, 7 G1T; 8 = pk.Z, count coefficients of 4 x u64; 9 = the evaluation-basis copy of G1T, n points or none; 10 = the
 * quotient-basis array, len(G1T) points or none).  Note A and Ap hold infinity for i <= NPublic (what the
 * prover sums, snark.go:265). */
int gs_pinocchio_pk_export(gs_handle pk, int which, uint64_t* jacobian, size_t count);
/* Read one array of a resident Groth16 key back as affine Jacobian triples: which = 0 G1.At, 1 G1.BACGamma,
 * 2 G2.BACGamma (24 words per point), 3 BACDelta, 4 PowersTauDelta; 5 = the single elements (count = 5: G1 Alpha, Beta,
 * Delta as 3 x 12 words, then G2 Beta, Delta as 2 x 24 words); 6 = pk.Z (count coefficients of 4 x u64); 7 = the
 * evaluation-basis copy of PowersTauDelta (n points, or 0 when the key has none); 10 = the quotient-basis array (len(PowersTauDelta)
 * points, or 0).  count must equal the array length.  With 0..6 a resident key can be written out in full (utils.GrothSetupToString). */
int gs_groth16_pk_export(gs_handle pk, int which, uint64_t* jacobian, size_t count);

/* ---- Pinocchio prover (snark.go) ------------------------------------------------------------ */
/* snark.Pk (snark.go:16-26): A, Ap, Bp, C, Cp, Kp: m G1 points; B: m G2 points; G1T: len(Z). */
int gs_pinocchio_pk_create(gs_handle a, gs_handle ap, gs_handle b_g2, gs_handle bp, gs_handle c, gs_handle cp,
                           gs_handle kp, gs_handle g1t, const uint64_t* z, size_t nz,
                           size_t nvars, size_t npublic, gs_handle* out);
/* snark.GenerateProofs (snark.go:254-289).  out_proof = PiA | PiAp | PiB(16) | PiBp | PiC |
 * PiCp | PiH | PiKp = 7*8 + 16 = 72 words; inf[8] in that order. */
int gs_pinocchio_prove(gs_handle pk, const uint64_t* w, size_t nw, const uint64_t* px, size_t npx,
                       uint64_t out_proof[72], int inf[8]);
/* Same with w and px already resident (gs_scalars_upload); what bench.py --workload prove_pinocchio times. */
int gs_pinocchio_prove_resident(gs_handle pk, gs_handle w, gs_handle px, uint64_t out_proof[72], int inf[8]);
/* snark.GenerateProofs from the witness alone (the Pinocchio twin of gs_groth16_prove_witness): H(x) straight from the constraint
 * values of the resident R1CS, no px; a witness that violates a constraint takes the exact px route (same result as the reference). */
int gs_pinocchio_prove_witness(gs_handle pk, gs_handle r1cs, gs_handle w, uint64_t out_proof[72], int inf[8]);
/* ... with the evaluation-basis copy of G1T (E[j-1] = l_j(tau) G over the nodes n+1..2n, so that sum_j H(n+j) E[j-1] = H(tau) G =
 * sum_i h_i G1T[i], snark.go:239-247, 284-286) when the key has one: gs_pinocchio_setup builds it, gs_pinocchio_pk_set_eval attaches
 * one, gs_pinocchio_pk_export which = 9 reads it back.  gs_pinocchio_prove_witness_begin: pipelined, collect with gs_pinocchio_prove_end. */
int gs_pinocchio_pk_set_eval(gs_handle pk, gs_handle bases);
/* ... and a quotient-basis array of G1T, Q[m] = sum_{d <= m} g_d G1T[m - d] (see gs_groth16_pk_set_quot): gs_pinocchio_setup builds it,
 * this attaches (bases = 0: detaches) one, gs_pinocchio_pk_export which = 10 reads it back. */
int gs_pinocchio_pk_set_quot(gs_handle pk, gs_handle bases);
int gs_pinocchio_pk_derive_quot(gs_handle pk);          /* as gs_groth16_pk_derive_quot, from G1T */
int gs_pinocchio_pk_derive_eval(gs_handle pk, size_t n_constraints);   /* as gs_groth16_pk_derive_eval, from G1T */
int gs_pinocchio_prove_witness_begin(gs_handle pk, gs_handle r1cs, gs_handle w, uint64_t* ticket);
/* Pipelined Pinocchio proving: same tickets as gs_groth16_prove_begin / _end (the three in-flight slots are shared between
 * Groth16 proofs, Pinocchio proofs and MSMs). */
int gs_pinocchio_prove_begin(gs_handle pk, gs_handle w, gs_handle px, uint64_t* ticket);
int gs_pinocchio_prove_end(uint64_t ticket, uint64_t out_proof[72], int inf[8]);
/* host-buffer tickets of snark.GenerateProofs (snark.go:254): as the Groth16 ones above; collect with gs_pinocchio_prove_end */
int gs_pinocchio_prove_host_begin(gs_handle pk, const uint64_t* w, size_t nw, const uint64_t* px, size_t npx, uint64_t* ticket);
int gs_pinocchio_prove_witness_host_begin(gs_handle pk, gs_handle r1cs, const uint64_t* w, size_t nw, uint64_t* ticket);
int gs_pinocchio_prove_witness_host(gs_handle pk, gs_handle r1cs, const uint64_t* w, size_t nw, uint64_t out_proof[72], int inf[8]);

/* ---- several GPUs (BASELINE configs[3] "MSM sharded across 8 GPUs" and configs[4] "one proof per GPU") ----------
 * The prover's sums run over independent terms (groth16.go:243-250,269-271): each device sums one contiguous shard of the
 * term ranges, and ONE record per device is exchanged -- the five partial sums of a proof (416 bytes: 48 words of affine
 * points | inf[5], shard index as u32) or one partial point (72 / 136 bytes).  RCCL cannot add curve points, so the exchange is
 * ncclAllGather of the records as ncclUint8 followed by N - 1 additions on the host core.
 *
 * Communicator.  gs_comm_init_local: every RCCL rank lives in this process, one per distinct physical device of gs_init's
 * list (ncclCommInitAll); the *_multi entry points then pass their records through ncclAllGather.  gs_comm_init_rank: one
 * process per GPU -- rank 0 obtains an id with gs_comm_unique_id, the host language distributes the 128 bytes, every process
 * calls gs_comm_init_rank(id, nranks, rank) (its current logical device joins); the *_sharded entry points gather over it.
 * gs_comm_allgather exposes the byte gather itself (host buffers; local mode: `send` holds one block per local rank and
 * `recv` receives rank 0's copy of all blocks).  *collectives counts the ncclAllGather calls completed so far. */
int gs_comm_unique_id(uint8_t out_id[128]);
int gs_comm_init_rank(const uint8_t id[128], int nranks, int rank);
int gs_comm_init_local(void);
void gs_comm_destroy(void);
int gs_comm_info(int* nranks, int* rank, int* is_local, uint64_t* collectives);
int gs_comm_allgather(const void* send, size_t bytes_per_rank, void* recv /* nranks x bytes_per_rank */);

/* One MSM over `ndev` logical devices of this process: bases[d] / scalars[d] hold shard d of the term range (the same
 * contiguous split of both, e.g. made with gs_g1_clone / gs_scalars_clone), resident on one logical device each.  The
 * devices run concurrently (one host thread each); *used_rccl (may be NULL) reports whether the partial points travelled
 * through ncclAllGather (a local communicator exists and the logical devices spread evenly over its ranks) or were simply
 * read from this process's memory.  Same result as one gs_msm_g1 over the whole range. */
int gs_msm_g1_multi(const gs_handle* bases, const gs_handle* scalars, int ndev, uint64_t out_affine[8], int* is_inf, int* used_rccl);
int gs_msm_g2_multi(const gs_handle* bases, const gs_handle* scalars, int ndev, uint64_t out_affine[16], int* is_inf, int* used_rccl);
/* One Groth16 proof over `ndev` logical devices: pk[d] = the full key or slice d of ndev (gs_groth16_pk_shard_to), w[d] / px[d]
 * = replicas of the witness and of P(x) on the same logical device (gs_scalars_clone).  Device d runs
 * gs_groth16_prove_partials for shard d; the records are exchanged as above and the O(1) tail runs once.  Same proof as
 * gs_groth16_prove_resident with the full key. */
int gs_groth16_prove_multi(const gs_handle* pk, const gs_handle* w, const gs_handle* px, int ndev, const uint64_t r[4], const uint64_t s[4],
                           uint64_t out_proof[32], int inf[3], int* used_rccl);
/* One process per GPU: this rank's shard (rank / nranks of the communicator made by gs_comm_init_rank), gathered inside the
 * library; every rank returns the complete result.  pk is the full key or this rank's slice; bases / scalars hold this
 * rank's shard of the term range. */
int gs_groth16_prove_sharded(gs_handle pk, gs_handle w, gs_handle px, const uint64_t r[4], const uint64_t s[4], uint64_t out_proof[32], int inf[3]);
/* Strong scaling WITHOUT a replicated polynomial stage ("run on GPU 0 and broadcast hx shards"), for keys with an
 * evaluation-basis array (gs_groth16_pk_set_eval; slices carry their share of it).  Per proof ONE rank -- the owner; over a stream of
 * proofs the ranks take turns -- runs gs_groth16_witness_values: resident sparse R1CS + witness -> the n values H(n+1), ..., H(2n)
 * as a resident scalar vector (*hv_inout: 0 = create; *violated = number of roots of Z at which the witness breaks a constraint: the
 * values are then meaningless and the proof must take gs_r1cs_px + the px entry points).  The owner scatters the vector -- slice k
 * of the contiguous split to rank k: gs_scalars_clone between the logical devices of one process, gs_scalars_scatter (ncclSend /
 * ncclRecv, one group) between processes -- and every rank sums ONLY its term ranges: gs_groth16_prove_partials_values (four sums
 * over its slice of w, the fifth over its slice of the values; record layout of gs_groth16_prove_partials), wrapped with the
 * exchange and the tail by gs_groth16_prove_multi_values / gs_groth16_prove_sharded_values.  Same proof as every other route. */
int gs_groth16_witness_values(gs_handle pk, gs_handle r1cs, gs_handle w, gs_handle* hv_inout, uint32_t* violated);
int gs_groth16_prove_partials_values(gs_handle pk, gs_handle w, gs_handle hv_slice, size_t shard_index, size_t shard_count,
                                     uint64_t out_sums[48], int inf[5]);
/* ... pipelined: a rank streams its shards of consecutive proofs through the three slots (begin enqueues, end collects the five sums). */
int gs_groth16_partials_values_begin(gs_handle pk, gs_handle w, gs_handle hv_slice, size_t shard_index, size_t shard_count, uint64_t* ticket);
int gs_groth16_partials_end(uint64_t ticket, uint64_t out_sums[48], int inf[5]);
int gs_groth16_prove_multi_values(const gs_handle* pk, const gs_handle* w, const gs_handle* hv_slices, int ndev, const uint64_t r[4], const uint64_t s[4],
                                  uint64_t out_proof[32], int inf[3], int* used_rccl);
int gs_groth16_prove_sharded_values(gs_handle pk, gs_handle w, gs_handle hv_slice, const uint64_t r[4], const uint64_t s[4], uint64_t out_proof[32], int inf[3]);
int gs_scalars_scatter(gs_handle full_on_root, size_t total, int root, gs_handle* slice_inout);
int gs_msm_g1_sharded(gs_handle bases, gs_handle scalars, uint64_t out_affine[8], int* is_inf);
int gs_msm_g2_sharded(gs_handle bases, gs_handle scalars, uint64_t out_affine[16], int* is_inf);
/* A batch of independent proofs (configs[4]; no collective): proof i reads w[i] / px[i], runs on the logical device those
 * handles live on with the key pk_of_device[that device] (0 for unused devices), through the pipelined prover (three in
 * flight per device, devices concurrently).  r, s: nproofs x 4 words; out_proofs: nproofs x 32 words; inf: nproofs x 3. */
int gs_groth16_prove_batch(const gs_handle* pk_of_device, int ndev, const gs_handle* w, const gs_handle* px, size_t nproofs,
                           const uint64_t* r, const uint64_t* s, uint64_t* out_proofs, int* inf);

/* ---- snark.GenerateProofs over several GPUs (snark.go:254-289; the scheme above applied to Pinocchio) ----
 * A Pinocchio proof IS its eight MSM sums -- PiA | PiAp | PiB (G2) | PiBp | PiC | PiCp | PiH | PiKp, snark.go:265-286, there is no
 * tail -- so rank k of N sums its term ranges and the eight partial points of the ranks add up to the proof (616-byte records).
 *   gs_pinocchio_pk_shard / _shard_to      a slice of a resident full key: entries [k/N, (k+1)/N) of the seven per-variable arrays,
 *                                          of G1T and of the evaluation-basis array; Z travels with every slice
 *   gs_pinocchio_prove_partials            the eight sums of shard k from resident w and px (full key or slice k), proof layout
 *   gs_pinocchio_witness_values            the proof owner's polynomial stage, as gs_groth16_witness_values (the same H)
 *   gs_pinocchio_prove_partials_values     the eight sums with PiH over this rank's slice of H's values (no polynomial work here)
 *   gs_pinocchio_combine                   n records (n x 72 words, n x 8 flags) -> the proof (host additions)
 *   gs_pinocchio_prove_multi[_values]      one process, ndev logical devices: partials on every device concurrently, exchange
 *                                          (RCCL when a local communicator spans the devices), addition
 *   gs_pinocchio_prove_sharded[_values]    one process per GPU: this rank's partials, ncclAllGather of the records, addition;
 *                                          every rank returns the complete proof
 *   gs_pinocchio_prove_batch               a batch of independent proofs, three in flight per device, no collective
 * Same proof as gs_pinocchio_prove_resident with the full key, whatever N. */
int gs_pinocchio_pk_shard(gs_handle full_pk, size_t shard_index, size_t shard_count, gs_handle* out);
int gs_pinocchio_pk_shard_to(gs_handle full_pk, size_t shard_index, size_t shard_count, int target_device, gs_handle* out);
int gs_pinocchio_prove_partials(gs_handle pk, gs_handle w, gs_handle px, size_t shard_index, size_t shard_count, uint64_t out_sums[72], int inf[8]);
int gs_pinocchio_witness_values(gs_handle pk, gs_handle r1cs, gs_handle w, gs_handle* hv_inout, uint32_t* violated);
int gs_pinocchio_prove_partials_values(gs_handle pk, gs_handle w, gs_handle hv_slice, size_t shard_index, size_t shard_count,
                                       uint64_t out_sums[72], int inf[8]);
int gs_pinocchio_combine(const uint64_t* sums /* n x 72 */, const int* inf_in /* n x 8 */, size_t n, uint64_t out_proof[72], int inf[8]);
int gs_pinocchio_prove_multi(const gs_handle* pk, const gs_handle* w, const gs_handle* px, int ndev, uint64_t out_proof[72], int inf[8], int* used_rccl);
int gs_pinocchio_prove_multi_values(const gs_handle* pk, const gs_handle* w, const gs_handle* hv_slices, int ndev, uint64_t out_proof[72], int inf[8],
                                    int* used_rccl);
int gs_pinocchio_prove_sharded(gs_handle pk, gs_handle w, gs_handle px, uint64_t out_proof[72], int inf[8]);
int gs_pinocchio_prove_sharded_values(gs_handle pk, gs_handle w, gs_handle hv_slice, uint64_t out_proof[72], int inf[8]);
int gs_pinocchio_prove_batch(const gs_handle* pk_of_device, int ndev, const gs_handle* w, const gs_handle* px, size_t nproofs,
                             uint64_t* out_proofs /* nproofs x 72 */, int* inf /* nproofs x 8 */);

/* ---- timing of the last prove / msm call (device time, HIP events on the library stream) --- */
typedef struct {
  float total_ms;        /* all device work of the call */
  float plan_ms;         /* scalar digit extraction + bucket sort */
  float accumulate_ms;   /* bucket accumulation kernels (dominant) */
  float reduce_ms;       /* bucket reduction + window combination + normalisation */
  float poly_ms;         /* H(x) = P(x)/Z(x) stage */
  float h2d_ms;          /* host-to-device copies inside the call */
  /* the dominant kernel alone (k_bucket_accumulate), summed over its launches in the call: */
  float acc_g1_ms;       /* G1 bucket-accumulation launches */
  float acc_g2_ms;       /* G2 bucket-accumulation launches */
  uint32_t acc_g1_launches, acc_g2_launches;
  uint64_t acc_g1_terms; /* (terms x base arrays) those G1 launches consumed */
  uint64_t acc_g2_terms;
  uint64_t acc_g1_adds;  /* mixed point additions those G1 launches performed = NON-ZERO digits of their plans x base arrays (counted by the plan) */
  uint64_t acc_g2_adds;
  uint32_t window_bits;  /* Pippenger window width c of the last plan; every term costs floor(254 / c) + 1 additions */
  uint32_t fallbacks;    /* witness-route calls that had to repeat on the exact px route because the witness violates a constraint */
  /* What the plans of the call found in their scalars (summed over the MSM groups, per base array): a term has one digit per window;
   * a ZERO digit costs nothing, every other one is one bucket addition.  Uniform scalars: plan_entries ~ plan_digits; a witness full
   * of 0 / 1 / small values: a fraction of it. */
  uint64_t plan_digits;   /* terms x windows x base arrays */
  uint64_t plan_entries;  /* non-zero digits x base arrays = mixed additions the accumulation kernels really performed */
  uint32_t heavy_buckets; /* buckets cut into more than 64 chunks (0/1-heavy witnesses), combined by a block-wide tree; summed per MSM GROUP
                           * (a proof's G2 and G1 groups over w share one plan: its heavy buckets count once for each) */
  uint32_t reserved;
} gs_timing;
int gs_last_timing(gs_timing* out);                         /* the calling thread's current logical device */
int gs_device_timing(int logical_device, gs_timing* out);

/* ---- device memory: accounting and eviction ---------------------------------------------------------------------------
 * The window tables (rows 2^(c j) P_i of every base array, built on a handle's first proof / MSM) are 15x the key data at
 * c = 17: 5.6 GiB per 2^20-constraint Groth16 key.  A host that keeps several keys resident can see what each one costs and
 * drop the tables of the idle ones; they are rebuilt on the handle's next use (~140 ms per 2^20 Groth16 key). */
typedef struct {
  uint64_t device_total_bytes, device_free_bytes;   /* hipMemGetInfo of the current logical device's GPU */
  uint64_t library_bytes;     /* every device byte this library holds, all logical devices of the process */
  uint64_t object_bytes;      /* the current logical device's handles: base arrays, keys (with their divisor caches), scalars, R1CS */
  uint64_t table_bytes;       /* window tables of those handles */
  uint64_t workspace_bytes;   /* bucket sets, chunk partials, result staging, fixed-base tables (plan / polynomial caches: in library_bytes) */
  uint64_t objects;           /* live handles on the current logical device */
  uint64_t evictions;         /* window tables this logical device dropped because an allocation found no memory (was `reserved`: same size) */
} gs_memory;
int gs_memory_query(gs_memory* out);
int gs_handle_bytes(gs_handle h, uint64_t* object_bytes, uint64_t* table_bytes);     /* either pointer may be NULL */
/* Free the window tables of a key or base array (queues behind outstanding tickets); results of later calls are unchanged. */
int gs_release_tables(gs_handle h);
/* WHEN a base array gets its window table (every logical device; results never depend on it):
 *   0 auto (default)  the reference proves once per key load (cli/main.go:330-349), and the tables of a 2^20 key cost ~140 ms and
 *                     5.6 GiB -- fifteen proofs' worth -- before the first proof.  An array without a table is summed TABLE-FREE
 *                     (a bucket set per window, every window adds the base point itself, the window sums recombined by Horner:
 *                     ~1.2x the additions); from its second use on its table is built in INSTALMENTS: every call buys slabs of
 *                     the table in proportion to its own work (~+60-100% of a table-free proof; GS_TABLE_BUDGET_PCT scales it),
 *                     enqueued ahead of its own accumulations, and the first call that finds the table complete switches over.
 *   1 always          the table is built inside the first call that needs it (rounds 1-4)
 *   2 never           table-free only (0.4 GiB per 2^20 key instead of 6; what 2^24 constraints on one GPU use)
 * gs_build_tables builds them NOW (blocking, whatever the policy): a server warming a key it will prove with for hours, and what
 * bench.py's steady-state numbers are measured on.  route: 0 = everything the key can use, 1 = only what the px routes need,
 * 2 = only what the witness routes need (the evaluation-basis array instead of PowersTauDelta / G1T); ignored for base arrays. */
int gs_set_table_policy(int policy);
int gs_build_tables(gs_handle h, int route);
/* Out of device memory is not fatal while window tables exist: an allocation that fails evicts least-recently-used tables of the
 * logical device (never one a ticket or the running call holds), retries once, and only then returns GS_ERR_HIP; an evicted table
 * comes back the way the policy says.  gs_memory.evictions counts them.  gs_set_memory_limit caps the device bytes the library may
 * hold (0 = no cap) -- a development / test hook that makes the condition reachable without filling 288 GB. */
int gs_set_memory_limit(uint64_t bytes);
/* hipMalloc / hipFree calls the library has made so far (process-wide): a stream of pipelined proofs -- resident or host-buffer
 * tickets -- moves neither in steady state.  Either pointer may be NULL. */
int gs_alloc_counters(uint64_t* allocs, uint64_t* frees);
/* sizeof(gs_timing), sizeof(gs_memory) of THIS library: both structs are written through caller pointers, and a binding compiled
 * against another revision of this header can tell before it passes a short buffer (gs_timing grew in round 4). */
int gs_abi_sizes(size_t* timing_bytes, size_t* memory_bytes);
/* Free every cached workspace of the current logical device (bucket sets, plan buffers, NTT twiddles, node trees, factorial
 * tables); rebuilt on demand.  Handles and their tables stay. */
int gs_trim(void);

/* Tunables (0 = automatic): Pippenger window bits. */
int gs_set_window_bits(int c);
/* Witness route of keys that carry an evaluation-basis array (gs_groth16_pk_set_eval): 1 (default) = h-MSM over H's values,
 * 0 = the coefficient route every other key takes.  Identical proofs; for measurements and tests. */
int gs_set_eval_basis(int enabled);

/* ---- verifier (host side) ---------------------------------------------------------------- */
/* The step after the prover.  These four entry points run on the calling host thread: a proof check is
 * O(1) work (a handful of pairings, a few thousand Fq products, latency bound), so there is nothing to offload.  They
 * need no gs_init, never touch the device and are not a fallback for anything above; they do not take the library
 * mutex, so a verifier thread runs beside in-flight proofs.
 *
 * bn128.Pairing(p1, p2) (bn128/bn128.go:179-186): the reduced optimal ate pairing MillerLoop^((q^12 - 1)/r) as the
 * reference's [2][3][2]*big.Int, 12 x 4 words in that nesting order, standard form.  Bit-identical to the reference's
 * value (same tower Fq2[u]/(u^2+1), Fq6 = Fq2[v]/(v^3-(9+u)), Fq12 = Fq6[w]/(w^2-v); lines differ only by a factor
 * the final exponentiation removes).  Either point at infinity gives 1.  GS_ERR_ARG if a point is off its curve. */
int gs_pairing(const uint64_t g1[12], const uint64_t g2[24], uint64_t out_fq12[48]);
/* *ok = [ prod_i e(g1_i, g2_i) == 1 ]: one multi-Miller loop (shared squarings, one batched inversion per step) and
 * ONE final exponentiation for all k pairs.  Points off the curve, or G2 points outside the order-r subgroup
 * (psi(Q) != [6x^2]Q; the twist has a large cofactor), give *ok = 0 (the reference would compute a meaningless Fq12
 * value and compare it).  gs_groth16_verify / gs_pinocchio_verify apply the subgroup check to the prover's G2 element
 * (PiB); the G2 elements of the verification key are key material, validated by whoever installs the key. */
int gs_pairing_check(const uint64_t* g1 /* k x 12 */, const uint64_t* g2 /* k x 24 */, size_t k, int* ok);
/* Input strictness of the two verifiers (process-wide).  0 (default) answers exactly like the reference's big.Int code: a
 * coordinate X and X + q, a public signal x and x + r name the same element, and fewer public signals than the vk has IC
 * points verify the statement with the missing inputs taken as 0 (groth16.go:283-286 loops over publicSignals only).  1 = strict:
 * coordinates must be < q and public signals < r (otherwise *ok = 0: no proof / input aliasing), and npublic must equal
 * nic - 1 (otherwise GS_ERR_SHAPE).  Deployments that accept proofs from untrusted parties should switch it on. */
int gs_verify_set_strict(int on);

/* groth16.VerifyProof(vk, proof, publicSignals, debug) (groth16/groth16.go:281-305):
 *   icPubl = IC[0] + sum_i publicSignals[i] * IC[i+1];   e(PiA, PiB) == e(Alpha, Beta) e(icPubl, Gamma) e(PiC, Delta)
 * as one 4-pair product check.  *ok = 1 accept / 0 reject.  GS_ERR_SHAPE when nic < npublic + 1 (the reference panics
 * on vk.IC[i+1] out of range). */
int gs_groth16_verify(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24],
                      const uint64_t vk_g2_delta[24], const uint64_t* vk_ic /* nic x 12 */, size_t nic,
                      const uint64_t* public_signals /* npublic x 4 */, size_t npublic,
                      const uint64_t pi_a[12], const uint64_t pi_b[24], const uint64_t pi_c[12], int* ok);
/* snark.VerifyProof (snark.go:292-368): the five Pinocchio checks in the reference's order, each a product check;
 * proof = PiA, PiAp (12 words each), PiB (24), PiBp, PiC, PiCp, PiH, PiKp (12 each) = 108 words (snark.go:59-69).
 * *failed_check (optional) = 0, or 1..5 for the first equation that does not hold (the reference's debug prints). */
int gs_pinocchio_verify(const uint64_t vka[24], const uint64_t vkb[12], const uint64_t vkc[24], const uint64_t g1kbg[12],
                        const uint64_t g2kbg[24], const uint64_t g2kg[24], const uint64_t vkz[24],
                        const uint64_t* vk_ic /* nic x 12 */, size_t nic, const uint64_t* public_signals, size_t npublic,
                        const uint64_t* proof /* 108 words */, int* ok, int* failed_check);

/* ---- pairing products on the device; Groth16 proofs verified in batches ------------------------------------------------------------ */
/* One proof check is O(1) work and stays on the host (above).  Thousands of proofs under one key are not: a host core checks one
 * proof in the time the device proves one and a half.  These two entry points need gs_init.
 *
 * gs_pairing_product: prod_{i<n} e(P[poff + i], Q[qoff + i]) for the points of a resident G1 and a resident G2 base array on the same
 * logical device, in gs_pairing's encoding and equal bit for bit to the product of the host's values.  *is_one = 1 iff the value is 1.
 * Either out-pointer may be NULL, not both.  n = 0 gives 1; a pair with an infinite member contributes 1.
 * PRECONDITION: the Q are in G2, the subgroup of order r.  The uploads guarantee the curve equation only; membership is the caller's
 * job -- gs_g2_subgroup_check on the same handle.  For a point of the twist outside the subgroup the call still returns, with a value
 * that means nothing (it runs the same instruction sequence whatever the points are).
 * One lane per pair runs the optimal ate Miller loop (inversion-free projective steps, the Fq12 accumulator in LDS), the values are
 * multiplied across each one-wave workgroup and then 64 to 1 per pass until at most 4 are left; those cross to the host, which
 * finishes the product and runs the ONE final exponentiation on the calling thread.
 * A range beyond an array is GS_ERR_SHAPE; a bad handle, a handle of the wrong kind or two null out-pointers GS_ERR_ARG; no device
 * GS_ERR_NOT_INIT.  Blocking; gs_last_timing().total_ms = device time.
 * go/gosnarkhip/pairing_device.go (PairingProduct) and tests/c/verify_batch.c are the plain call. */
int gs_pairing_product(gs_handle g1, size_t poff, gs_handle g2, size_t qoff, size_t n,
                       uint64_t out_fq12[48] /* may be NULL */, int* is_one /* may be NULL, not both */);
/* nproofs Groth16 proofs of ONE verification key in one randomised check: with s = challenge mod r and the weights z_i = s^i,
 *   *ok = 1  iff  prod_i e(-z_i A_i, B_i) . e((sum_i z_i) Alpha, Beta) . e(sum_i z_i vkx_i, Gamma) . e(sum_i z_i C_i, Delta) = 1,
 * vkx_i = IC[0] + sum_j publicSignals[i][j] IC[j+1].  The arguments are gs_groth16_verify's with one more dimension; the host checks are
 * the same (null arguments GS_ERR_ARG, nic < npublic + 1 GS_ERR_SHAPE, and under gs_verify_set_strict(1) nic != npublic + 1 is
 * GS_ERR_SHAPE and a non-canonical coordinate or signal in any proof gives *ok = 0).  A point off its curve gives *ok = 0, a B
 * outside the order-r subgroup (gs_g2_subgroup_check over all of them) gives *ok = 0.  nproofs = 0 gives *ok = 1 without touching
 * the device.
 * SOUNDNESS: a batch that holds an invalid proof passes with probability at most (nproofs - 1) / r over a challenge drawn uniformly
 * AFTER the proofs are fixed (the product is a polynomial of degree nproofs - 1 in s in the exponent).  The challenge is the
 * caller's randomness: a constant or a value the prover can predict voids the bound, and s = 0 or 1 mod r is GS_ERR_ARG.  *ok = 0 does
 * not say WHICH proof is bad: gs_groth16_verify finds it.
 * The device scales the A_i (gs_g1_scale_powers), sums the C_i (gs_msm_g1, table-free), tests the B_i and runs the nproofs Miller
 * loops with their product; the host forms the npublic + 1 scalars of the public-input sum, the three key pairs and the one final
 * exponentiation.  Every temporary array is freed on every path.  Blocking.
 * go-snark-study_amd/groth16.py (VerifyProofs), go/gosnarkhip/pairing_device.go (Groth16VerifyBatch) and tests/c/verify_batch.c. */
int gs_groth16_verify_batch(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24],
                            const uint64_t vk_g2_delta[24], const uint64_t* vk_ic, size_t nic,
                            const uint64_t* public_signals /* nproofs x npublic x 4 */, size_t npublic,
                            const uint64_t* pi_a /* nproofs x 12 */, const uint64_t* pi_b /* nproofs x 24 */,
                            const uint64_t* pi_c /* nproofs x 12 */, size_t nproofs, const uint64_t challenge[4], int* ok);
/* gs_groth16_verify_each: the verdict of gs_groth16_verify for EVERY proof of a batch under one key, on the device: ok_each[i] is exactly
 * what gs_groth16_verify writes to *ok for proof i with its signals, in both settings of gs_verify_set_strict.  No challenge, no
 * soundness caveat: the call is deterministic and never wrong.  *nbad (optional) = how many verdicts are 0.
 * The arguments are gs_groth16_verify_batch's without the challenge, and so are the shape errors: null arguments GS_ERR_ARG,
 * nic < npublic + 1 GS_ERR_SHAPE, under strict mode nic != npublic + 1 GS_ERR_SHAPE; in these cases nothing is written.  Not errors,
 * but verdicts: a proof with a point off its curve gets 0 (the host tests the 3n points first, a few products each, and the point at
 * infinity is uploaded in their place, because the uploads refuse a whole array for one such point); under strict mode a proof with a
 * non-canonical coordinate or signal gets 0; a B on the twist outside the order-r subgroup gets 0 (a per-point flags kernel); a key
 * point off its curve makes every verdict 0.  nproofs = 0 returns GS_OK with *nbad = 0 and needs no device; without a device every
 * other call returns GS_ERR_NOT_INIT and writes nothing.  There is no host fallback.
 * Per proof, one lane: vkx_i = IC_0 + sum_j pub_ij IC_{j+1} by a joint double-and-add (any 256-bit signal, the group law reduces it),
 * then ONE Miller accumulator over the three pairs (-A_i, B_i), (vkx_i, gamma), (C_i, delta) -- the lines of gamma and delta are
 * prepared once per call on the host and only evaluated per lane -- times the key's Miller value of e(alpha, beta), then the final
 * exponentiation kernel of gs_pairing_each.  Memory: 135 KB of workspace per 64 proofs (see gs_pairing_each).  Blocking;
 * gs_last_timing(): total_ms = device time, of which h2d_ms = signals, lines and the key value, poly_ms = membership, plan_ms = vkx,
 * accumulate_ms = Miller loops, reduce_ms = final exponentiations.
 * go-snark-study_amd/groth16.py (VerifyProofsEach), go/gosnarkhip/pairing_device.go (Groth16VerifyEach) and tests/c/verify_each.c. */
int gs_groth16_verify_each(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24],
                           const uint64_t vk_g2_delta[24], const uint64_t* vk_ic, size_t nic,
                           const uint64_t* public_signals /* nproofs x npublic x 4 */, size_t npublic,
                           const uint64_t* pi_a, const uint64_t* pi_b, const uint64_t* pi_c, size_t nproofs,
                           int* ok_each /* nproofs */, uint64_t* nbad /* may be null */);
/* ---- proofs of many keys in one call ----
 * gs_groth16_vk_create: a PREPARED verification key as a device object.  It does once what gs_groth16_verify_each does per call: the
 * curve tests of the five key points and the IC points, the Miller value of e(alpha, beta), the prepared lines of gamma and delta.  The
 * object keeps on the device the nic IC points, both prepared lists as limbs (29 KB), the 48 words of the Miller value, npublic =
 * nic - 1 and the two skip flags of an infinite gamma or delta (allowed, as in the single verifier).  gs_free, gs_handle_bytes,
 * gs_handle_device and gs_memory_query treat it like any other object.
 * A key that cannot verify anything is REFUSED when it is installed -- where gs_groth16_verify_each answers such a key with all-zero
 * verdicts on every call: a key point off its curve is GS_ERR_ARG and the message names the point (alpha, beta, gamma, delta, IC[j]);
 * a degenerate step in the Miller loop of beta or the prepared lines of gamma or delta (a point of the twist that is not of order r) is
 * GS_ERR_ARG naming the point.  nic = 0 is GS_ERR_SHAPE, a null argument GS_ERR_ARG; without a device GS_ERR_NOT_INIT.  On every
 * error nothing is written and nothing stays allocated. */
int gs_groth16_vk_create(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24],
                         const uint64_t vk_g2_delta[24], const uint64_t* vk_ic /* nic x 12 */, size_t nic, gs_handle* out);
/* gs_groth16_verify_each_keys: gs_groth16_verify_each for proofs that each NAME THEIR KEY: ok_each[i] is exactly what gs_groth16_verify
 * writes for (the key keys[key_of_proof[i]], proof i, its signals), in both settings of gs_verify_set_strict.  *nbad (optional) = how
 * many verdicts are 0.  Every proof brings exactly nic - 1 signals of its key in BOTH settings; the lax rule of the single verifier,
 * "missing signals count as 0", is what zero padding by the caller gives.
 * Verdicts, not errors, exactly as in gs_groth16_verify_each: a proof point off its curve gives 0 and infinity travels in its place;
 * under strict mode a non-canonical coordinate or signal gives 0; a B outside the order-r subgroup gives 0.
 * Errors, with nothing written: key_of_proof[i] >= nkeys, a bad handle or one of another kind, keys on different logical devices (or
 * not on the calling thread's: the proofs' arrays are created there), a null argument: GS_ERR_ARG; no device: GS_ERR_NOT_INIT, unless
 * nproofs = 0, which is GS_OK with *nbad = 0 and needs no device, keys or handles.  The same handle may appear twice in keys; a key may
 * have no proofs.  Every temporary is freed on every path.  There is no host fallback.  Blocking.
 * Layout: the Miller-loop kernel is fast because the 2 x 102 prepared lines of a key are the same words for every lane of a wave, so a
 * wave never mixes keys: the host groups the proofs by key, stably, pads every key's run to a multiple of 64 SLOTS, and one one-wave
 * workgroup is one key (csrc/verify_plan.h).  The three point arrays and the signals go up in slot order; padded slots hold the point
 * at infinity, compute on it and are never read back.  Each workgroup reads its group record and then its key record { lines, ic, ab,
 * npublic, skip_gamma, skip_delta } -- a table uploaded per call from the key objects -- at addresses that are uniform across the
 * wave; the kernels' bodies are those of gs_groth16_verify_each, and its membership and final-exponentiation kernels run unchanged
 * over all slots.
 * Memory: per key 29 KB of lines resident (plus its IC points); per call 135 KB of workspace and 25 KB of values and flags per GROUP
 * of 64 slots, and a group is started for every key with a proof: 256 keys with one proof each cost what 16384 proofs of one key
 * cost.  Slots are indexed with 32 bits: a call whose padded runs reach 2^32 slots is GS_ERR_SHAPE; pass the proofs in windows.
 * Limits, deliberately: no per-lane key (dense packing of keys with few proofs: the lines would become per-lane gathers and the
 * register budget of the loop is gone), no randomised multi-key batch, no Pinocchio.
 * gs_last_timing(): total_ms = device time, of which h2d_ms = signals and the two tables, poly_ms = membership, plan_ms = vkx,
 * accumulate_ms = Miller loops, reduce_ms = final exponentiations.
 * go-snark-study_amd/groth16.py (PrepareVerificationKey, VerifyProofsEachKeys), go/gosnarkhip/pairing_device.go (Groth16VkCreate,
 * Groth16VerifyEachKeys) and tests/c/verify_each_keys.c. */
int gs_groth16_verify_each_keys(const gs_handle* keys, size_t nkeys, const uint32_t* key_of_proof /* nproofs */,
                                const uint64_t* public_signals /* concatenated in proof order; proof i has nic(key_of_proof[i]) - 1 signals */,
                                const uint64_t* pi_a, const uint64_t* pi_b, const uint64_t* pi_c, size_t nproofs,
                                int* ok_each, uint64_t* nbad /* may be NULL */);
/* gs_pinocchio_verify_each: the verdict of gs_pinocchio_verify for EVERY proof of a batch under one key, on the device: ok_each[i] is
 * exactly what gs_pinocchio_verify writes to *ok for proof i with its signals and failed_each[i] (optional) what it writes to
 * *failed_check -- 0, or 1..5 for the first equation in the reference's order that does not hold -- in both settings of
 * gs_verify_set_strict.  Deterministic, no challenge.  *nbad (optional) = how many verdicts are 0.
 * The arguments are gs_pinocchio_verify's with one more dimension (proofs: nproofs x 108 words in its layout), the errors those of
 * gs_groth16_verify_each: null arguments GS_ERR_ARG, nic < npublic + 1 GS_ERR_SHAPE, under strict mode nic != npublic + 1 GS_ERR_SHAPE; in
 * these cases nothing is written.  nproofs = 0 returns GS_OK with *nbad = 0 and needs no device; without a device every other call
 * returns GS_ERR_NOT_INIT and writes nothing.  There is no host fallback.  Every temporary array is freed on every path.
 * Not errors, but verdicts, each with the equation number the host gives: under strict mode a proof with a non-canonical coordinate or
 * signal gets (0, 0).  A proof point off its curve fails the equations that use it (PiA 1, 4, 5; PiAp 1; PiB 2, 4, 5; PiBp 2; PiC 3,
 * 4, 5; PiCp 3; PiH 4; PiKp 5): the host tests the 8n points first, a few products each, and the point at infinity is uploaded in
 * their place, because the uploads refuse a whole array for one such point.  A PiB on the twist outside the order-r subgroup (a
 * per-point flags kernel) fails at equation 2 unless equation 1 failed already.  A key point off its curve fails every equation that
 * uses it, for every proof (an IC point: equations 4 and 5 of the proofs whose sum takes it); a key G2 point with a degenerate step in
 * prepare_g2_lines fails them where its partner in G1 is finite.
 * The host prepares the lines of the six G2 points that are the same for every proof (Vka, Vkc, Vkz, G2Kbg, G2Kg and the generator)
 * once per call.  Per proof, one lane: vkx_i by the joint double-and-add of gs_groth16_verify_each, then vkx_i + PiA_i and that sum
 * plus PiC_i by complete formulas; then one workgroup row per equation, (nproofs / 64, 5) workgroups of one wave: equations 1 and 3
 * only evaluate prepared lines (no G2 arithmetic), equations 2, 4 and 5 run PiB_i as the one live pair beside up to two prepared
 * pairs; then the final exponentiation kernel of gs_pairing_each over all 5 nproofs values.  The host folds the 5 nproofs flags,
 * the membership flags and its own screening into verdicts.
 * Memory: per 64 proofs 5 x 135 KB of workspace and 5 x 24 KB of exponentiated values and flags (52 MB at 4096 proofs): a caller with
 * millions of proofs passes them in windows.  Blocking; gs_last_timing(): total_ms = device time, of which h2d_ms = signals and lines,
 * poly_ms = membership, plan_ms = vkx and the two sums, accumulate_ms = Miller loops, reduce_ms = final exponentiations.
 * go-snark-study_amd/snark.py (VerifyProofsEach, VerifyProofsEachChecks), go/gosnarkhip/pairing_device.go (PinocchioVerifyEach) and
 * tests/c/pinocchio_verify_each.c. */
int gs_pinocchio_verify_each(const uint64_t vka[24], const uint64_t vkb[12], const uint64_t vkc[24], const uint64_t g1kbg[12],
                             const uint64_t g2kbg[24], const uint64_t g2kg[24], const uint64_t vkz[24],
                             const uint64_t* vk_ic /* nic x 12 */, size_t nic,
                             const uint64_t* public_signals /* nproofs x npublic x 4 */, size_t npublic,
                             const uint64_t* proofs /* nproofs x 108 words, gs_pinocchio_verify's layout */, size_t nproofs,
                             int* ok_each /* nproofs */, int* failed_each /* nproofs, may be NULL */, uint64_t* nbad /* may be NULL */);
/* gs_pairing_each: e(P[poff + i], Q[qoff + i]) for EVERY i < n, final exponentiation included, all of it on the device.  Value i
 * goes to out_fq12 + 48 i in gs_pairing's encoding and is equal bit for bit to gs_pairing on that pair; is_one[i] = 1 iff it is 1.
 * Either out-pointer may be NULL, not both.  A pair with an infinite member gives 1; n = 0 writes nothing (and still needs gs_init and
 * valid handles, like gs_pairing_product).
 * PRECONDITION (gs_pairing_product's): the Q are in G2, the subgroup of order r -- gs_g2_subgroup_check on the same handle.  For a
 * point of the twist outside the subgroup the call still returns, with a value that means nothing.
 * One lane per pair runs the Miller loop of gs_pairing_product and keeps its value (limb-major in a workspace of the one-wave
 * workgroup, never in the 96-word encoding); a second kernel runs the final exponentiation per lane: the easy part with one
 * inversion, three powers by the 63-bit BN parameter on cyclotomic squarings and the y0..y6 chain of the host verifier, the working
 * value in LDS and five temporaries in the workspace.  No step branches on a value.
 * Errors, locking and timing are gs_pairing_product's: a range beyond an array GS_ERR_SHAPE; a bad handle, a handle of the wrong kind
 * or two null out-pointers GS_ERR_ARG; no device GS_ERR_NOT_INIT (nothing is written).  Blocking; gs_last_timing().total_ms = device
 * time, of which accumulate_ms is the Miller kernel and reduce_ms the final exponentiation kernel.
 * Memory: the call allocates 5 x 27 KB of workspace per 64 pairs plus 384 B per pair for the whole range at once (8.6 MB at 4096
 * pairs, 2.2 GB at 2^20): a caller with millions of pairs passes them in windows (poff, qoff, n).
 * go/gosnarkhip/pairing_device.go (PairingEach) and tests/c/pairing_each.c are the plain call. */
int gs_pairing_each(gs_handle g1, size_t poff, gs_handle g2, size_t qoff, size_t n,
                    uint64_t* out_fq12 /* n x 48, may be NULL */, int* is_one /* n, may be NULL, not both */);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GOSNARK_HIP_H */
