// Internal: device-resident proving keys (described as data the prover engine in prove.hip reads; built in keys.hip) and what the
// other translation units need of the prover's staging and of the R1CS routines (capi_poly.hip, capi_r1cs.hip).
#pragma once
#include <vector>
#include <mutex>
#include "msm.h"
#include "poly.h"
#include "route.h"
#include "runtime.h"

namespace gs {

struct KeyArray {                 // one base array of a key: packed affine points (an owned copy) and their window table (built on the
  DevBuf pts;                     // first proofs, msm.h)
  BaseTable table;
};

// What a Groth16 and a Pinocchio proving key have in common -- which is everything the prover engine needs: a proof of either
// scheme is some G1 sums and one G2 sum over w sharing a plan, H(x) = px / Z, and one G1 sum over h.  The engine (prove.hip),
// the memory accounting (capi_mem.hip) and the evaluation-basis entry points (setup.hip) walk this description; none of them asks
// which scheme a key belongs to.
struct ProverKey : Object {
  const char* const scheme;       // "groth16" / "pinocchio": names the entry points in error messages (gs_<scheme>_prove_partials ...)
  const char* const hx_too_long;  // wording of "len(hx) exceeds the h array" (two %zu: len(hx), len_h)
  size_t nvars = 0, npublic = 0, nz = 0, len_h = 0;   // global counts (len_h = len(PowersTauDelta) / len(G1T))
  // Key slices (multi-GPU, SURVEY 8e "each GPU holds 1/8 of every pk array"): a key created by gs_groth16_pk_create_shard /
  // gs_*_pk_shard holds only the term ranges of shard `shard_index` of `shard_count`: entries [w_lo, w_lo + n_w) of the arrays over w
  // and entries [h_lo, h_lo + n_h) of the h array.  A full key has shard_count = 1, n_w = nvars, n_h = len_h.
  size_t shard_index = 0, shard_count = 1, w_lo = 0, n_w = 0, h_lo = 0, n_h = 0;
  // The arrays.  g1w[0 .. n_g1w): the G1 arrays summed over w, in the order of the sums (one launch over one plan of w); g1w[b_g1]
  // is the one that shares B's sparsity with the G2 array g2w; h is summed over hx = px / Z.
  static constexpr int kMaxG1w = 6;
  const int n_g1w, b_g1;
  KeyArray g1w[kMaxG1w], g2w, h;
  // Evaluation-basis twin of h (optional; the setups build it, gs_*_pk_set_eval attaches one): h_eval[j-1] = l_j(tau) * (what h[i]
  // multiplies tau^i with) * G,  l_j = Lagrange basis over the nodes n+1 .. 2n  (j = 1..n_eval = #constraints), so that
  //   sum_j H(n+j) h_eval[j-1] = sum_i h_i h[i]      (groth16.go:139-149, 269-271; snark.go:239-247, 284-286):
  // the witness route runs the h-MSM over H's VALUES and never interpolates H.  A slice holds entries [e_lo, e_lo + n_e).
  size_t n_eval = 0, e_lo = 0, n_e = 0;
  KeyArray h_eval;
  // Keys over a power-of-two domain (domain.h; snarkjs / circom Groth16 keys).  domain_log2 = k >= 1: a full key whose Z is exactly
  // x^m - 1, m = 2^k (read off Z on the host when the key is created; 0 otherwise) -- the only keys a domain R1CS proves with.
  // eval_domain_log2 says which basis h_eval holds: 0 = the Lagrange basis over the nodes n+1 .. 2n above, k = the coset
  // evaluation basis of the domain 2^k (m points, natural order).  The evaluation-basis route is taken only when it matches the R1CS.
  int domain_log2 = 0, eval_domain_log2 = 0;
  // A coset-only key (gs_groth16_pk_create_domain; what a snarkjs .zkey holds): domain_log2 = eval_domain_log2 = k, h_eval = the m coset
  // points, and NO monomial h array (len_h = n_h = 0, h.pts empty).  It proves from a witness on the evaluation-basis route and
  // nowhere else: whatever needs h -- the px routes, the derivations, the quotient basis, key slices -- refuses it (refuse_coset_only).
  bool coset_only = false;
  // Quotient-basis twin of h (optional; the setups build it, gs_*_pk_set_quot attaches one): with D = deg Z and g = 1 / rev(Z) as a
  // power series (z.inv_rev_mont),  h_quot[m] = sum_{d <= m} g_d h[m - d],  m < n_q = len_h.  floor(x^i / Z) = sum_d g_d x^(i-D-d), so
  // for every px with nh = len(px) - D >= 1 coefficients of floor(px / Z):
  //   sum_{j < nh} floor(px / Z)_j h[j] = sum_{m < nh} px[D + m] h_quot[m]:
  // the h-MSM runs over the top coefficients of px as they are and nothing is divided by Z (prove.hip, proof_enqueue).  A key that
  // holds the array serves the px routes from it and builds no window table of h for them.  Full keys only: the key slices
  // (gs_*_pk_shard*) carry no quotient-basis array and keep the division.
  size_t n_q = 0;
  KeyArray h_quot;
  // The workspace sets (of the eight a ticket slot owns; the G1 group over w takes set 0) of the G2 group, of the B' group of a
  // proof with split B, and of the h group.  They decide which grow-only buffers a proof touches, hence gs_memory.
  const int ws_g2, ws_b, ws_h;
  Divisor z;                      // pk.Z with cached 1/rev(Z) series + spectrum
  // Which of the held variables appear in B at all (round 5).  The reference's circuit compiler puts a variable into B only as the
  // second operand of a multiplication or a divisor (circuitcompiler/circuit.go:110-128: `+` / `-` / `in` rows have B = [one]), so for
  // its circuits most points of g1w[b_g1] / g2w are the point at infinity.  b_index lists the held variables of which either
  // point is finite (ascending, relative to the first held variable; on the device and on the host, where a call cuts its term range out
  // of it), b_finite is their number: when enough are missing the prover sums the two B arrays -- 3.8 of a Groth16 proof's 6.8
  // job-units -- over a SECOND plan of w that holds the listed terms only (prove.hip, proof_enqueue).  Scanned once, when the key is
  // created; keys without a missing point keep no list.
  DevBuf b_index;
  std::vector<uint32_t> b_index_host;
  size_t b_finite = 0;

  // every array with its held length, in the fixed order  g1w .. | h | g2w | h_eval | h_quot  (f(KeyArray&, size_t n, bool g2))
  template <class F> void for_each_array(F f) {
    for (int i = 0; i < n_g1w; ++i) f(g1w[i], n_w, false);
    f(h, n_h, false); f(g2w, n_w, true); f(h_eval, n_e, false); f(h_quot, n_q, false);
  }
  // the px routes of this key sum h over px's top coefficients against h_quot (GS_NO_QUOT_BASIS: divide by Z although the key has
  // the array -- same proofs, for A/B runs)
  bool serves_quot() const {
    static const bool off = run_flag("GS_NO_QUOT_BASIS");
    return n_q != 0 && !off;
  }
 protected:
  ProverKey(Kind k, const char* scheme_, const char* hx_too_long_, int n_g1w_, int b_g1_, int ws_g2_, int ws_b_, int ws_h_)
      : Object(k), scheme(scheme_), hx_too_long(hx_too_long_), n_g1w(n_g1w_), b_g1(b_g1_), ws_g2(ws_g2_), ws_b(ws_b_), ws_h(ws_h_) {}
};
inline ProverKey* as_prover_key(Object* o) {
  return o && (o->kind == Kind::GrothPk || o->kind == Kind::PinocchioPk) ? static_cast<ProverKey*>(o) : nullptr;
}
inline int refuse_coset_only(const char* fn) {
  return fail(GS_ERR_SHAPE, "%s: the key holds the coset evaluation basis only (it has no monomial h array): it proves from a witness "
              "with a domain R1CS on the evaluation-basis route, and nothing else", fn);
}
// what the route decision (route.h) reads of a key
inline KeyFacts key_facts(const ProverKey& pk) {
  return KeyFacts{pk.nz, pk.len_h, pk.shard_index, pk.shard_count, pk.h_lo, pk.n_h, pk.n_eval, pk.e_lo, pk.n_e, pk.n_q, pk.coset_only, pk.serves_quot()};
}
// keys.hip
void pk_scan_sparsity(Ctx& c, ProverKey& pk);      // fills b_index / b_finite (synchronises the stream)
bool bad_shard(size_t shard_index, size_t shard_count);
void force_infinity(Ctx& c, DevBuf& pts, size_t count, size_t words);   // zero the first `count` packed points (-> infinity)

struct GrothPkObj : ProverKey {   // groth16.Pk (groth16/groth16.go:15-32), resident
  static constexpr Kind kKind = Kind::GrothPk;
  enum { kAt = 0, kBacGamma1 = 1, kBacDelta = 2 };      // g1w: the sums over w in the order of gs_groth16_prove_partials
  DevBuf& at() { return g1w[kAt].pts; }
  DevBuf& bacgamma1() { return g1w[kBacGamma1].pts; }
  DevBuf& bacdelta() { return g1w[kBacDelta].pts; }
  DevBuf& bacgamma2() { return g2w.pts; }
  DevBuf& ptd() { return h.pts; }                       // PowersTauDelta
  DevBuf& ptd_eval() { return h_eval.pts; }             // l_j(tau) * Z(tau) / delta * G
  DevBuf& ptd_quot() { return h_quot.pts; }
  G1Affine alpha, beta, delta;             // host, Montgomery
  G2Affine beta2, delta2;
  // host-side window tables of delta / delta2 for the tail's result-independent products (built on the first proof of the key)
  std::once_flag fixed_once;
  HostFixedBase<FqTag> delta_fixed;
  HostFixedBase<Fq2Tag> delta2_fixed;
  GrothPkObj()
      : ProverKey(kKind, "groth16", "len(hx) = len(px) - len(Z) + 1 = %zu exceeds len(PowersTauDelta) = %zu (groth16.go:269-271)", 3, kBacGamma1,
                  4, 2, 3) {}
};

struct PinocchioPkObj : ProverKey {  // snark.Pk (snark.go:16-26), resident
  static constexpr Kind kKind = Kind::PinocchioPk;
  enum { kA = 0, kAp, kBp, kC, kCp, kKp };              // g1w: A, A', B', C, C', K' (snark.go:265-278)
  DevBuf& a() { return g1w[kA].pts; }
  DevBuf& ap() { return g1w[kAp].pts; }
  DevBuf& bp() { return g1w[kBp].pts; }
  DevBuf& c() { return g1w[kC].pts; }
  DevBuf& cp() { return g1w[kCp].pts; }
  DevBuf& kp() { return g1w[kKp].pts; }
  DevBuf& b2() { return g2w.pts; }
  DevBuf& g1t() { return h.pts; }
  DevBuf& g1t_eval() { return h_eval.pts; }             // l_j(tau) * G
  DevBuf& g1t_quot() { return h_quot.pts; }
  PinocchioPkObj() : ProverKey(kKind, "pinocchio", "len(hx) = %zu exceeds len(G1T) = %zu (snark.go:284-286)", 6, kBp, 6, 5, 7) {}
};

// ---- shared with capi_poly.hip / capi_r1cs.hip ----------------------------------------------------------------------------------
// Per-context staging of the prover and polynomial entry points (device memory belongs to one device).
struct ProveState {
  DevBuf hx[Ctx::kSlots];                       // hx = floor(px / Z) -- or H's values on the evaluation-basis route --, one per slot (standard form)
  DevBuf up_w, up_px, up_a, up_b, up_o;         // uploads of host operands / results (blocking entry points only)
  DevBuf exact_px[Ctx::kSlots];                 // px of the exact witness route, one per slot (allocated only if that route is ever taken)
  // Host-buffer tickets (gs_*_host_begin): every in-flight slot owns the device copies of ITS w / px.  Grow-only, so a stream of
  // proofs from host memory allocates nothing after its first lap over the slots (gs_alloc_counters); a slot is re-used only after
  // its ticket was collected, i.e. after every device read of these buffers.
  DevBuf slot_w[Ctx::kSlots], slot_px[Ctx::kSlots];
};
inline ProveState& prove_state(Ctx& c) { return c.state<ProveState>(c.prove_state); }
const uint32_t* upload_tmp(Ctx& c, DevBuf& buf, const uint64_t* host, size_t n);   // host scalars -> a scratch buffer (books h2d_ms)
void download(Ctx& c, uint64_t* host, const void* dev, size_t n);                  // n scalars to the host; synchronises c.stream
// An "inout" scalar vector of an entry point: *handle == 0 creates a resident vector of n scalars and stores its handle; otherwise the
// handle must hold exactly n, or the call fails with `wording` (a format of fn and n: one %s, one %zu).  nullptr = failed.
inline Scalars* inout_scalars(Ctx& c, gs_handle* handle, size_t n, const char* wording, const char* fn) {
  if (!*handle) {
    auto fresh = std::make_unique<Scalars>();
    fresh->n = n;
    fresh->buf.alloc(n * 32);
    *handle = c.put(std::move(fresh));
  }
  Scalars* s = c.get<Scalars>(*handle, Kind::Scalars);
  if (!s || s->n != n) { fail(GS_ERR_ARG, wording, fn, n); return nullptr; }
  return s;
}
// capi_r1cs.hip: w (standard form, m elements, device) -> o.vals = [A w | B w | C w], and -> o.coef = [ax | bx | cx] and px_out
void r1cs_values_dev(Ctx& c, R1csObj& o, const uint32_t* w_dev);
void r1cs_values_into_dev(Ctx& c, R1csObj& o, const uint32_t* w_dev, DevBuf& w_mont, DevBuf& vals);      // the same into the caller's workspaces
void r1cs_px_dev(Ctx& c, R1csObj& o, const uint32_t* w_dev, uint32_t* px_out);

}  // namespace gs
