// Verifier entry points: groth16.VerifyProof (groth16/groth16.go:281-305), snark.VerifyProof
// (snark.go:292-368) and the pairing seam under them (bn128/bn128.go:179-186), on the host.  They do not touch the
// device context and do not take its lock: a verifier thread can run beside in-flight proofs.  The batch and per-proof verifiers
// below them do their per-key and per-proof host work here and run the rest on the device through verify_device.h.
#include <atomic>

#include "runtime.h"
#include "verify_device.h"
#include "verify_plan.h"

using namespace gs;
using namespace gs::pairing;

namespace {

struct ShapeError { const char* msg; };

// gs_verify_set_strict: 0 (default) = the reference's big.Int behaviour, 1 = canonical encodings only
std::atomic<int> g_strict{0};
const uint64_t kRorder[4] = {0x43e1f593f0000001ULL, 0x2833e84879b97091ULL, 0xb85045b68181585dULL, 0x30644e72e131a029ULL};   // bn128.go:46 (R)

// every coordinate < q ?  (words: count of 4-limb field elements)
bool coords_canonical(const uint64_t* w, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (limbs_geq(w + 4 * i, kP)) return false;
  return true;
}
bool scalars_canonical(const uint64_t* w, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (limbs_geq(w + 4 * i, kRorder)) return false;
  return true;
}

// prod e(P_i, Q_i) == 1 with one shared final exponentiation.  Off-curve inputs and G2 inputs that hit a vertical
// line inside the loop (not of order r) make the check fail instead of producing a meaningless value.
// `untrusted_g2` lists the indices of G2 inputs that came from a prover (they get the subgroup check; key material is
// checked once by whoever installs the key, not per proof).
bool product_is_one(const std::vector<G1Aff>& ps, const std::vector<G2Aff>& qs, const std::vector<int>& untrusted_g2 = {}) {
  for (const G1Aff& p : ps)
    if (!g1_on_curve(p)) return false;
  for (const G2Aff& q : qs)
    if (!g2_on_curve(q)) return false;
  for (int i : untrusted_g2)
    if (!g2_in_subgroup(qs[(size_t)i])) return false;
  Fp12 f;
  if (!multi_miller_loop(ps, qs, f)) return false;
  return f12_eq(final_exponentiation(f), f12_one());
}

// What every verifier tests of its counts before any work.  The reference indexes vk.IC[i+1] for every public signal and panics past
// the end (groth16.go:285); strict mode wants exactly one signal per IC point (a short list would silently verify the statement "the
// missing inputs are 0").  GS_OK: *strict is the mode of this call.
int check_signal_count(const char* fn, size_t nic, size_t npublic, bool* strict) {
  if (nic < npublic + 1) return fail(GS_ERR_SHAPE, "%s: %zu public signals need %zu IC points, vk has %zu", fn, npublic, npublic + 1, nic);
  *strict = g_strict.load() != 0;
  if (*strict && nic != npublic + 1)
    return fail(GS_ERR_SHAPE, "%s (strict): vk has %zu IC points, so exactly %zu public signals are required (got %zu)", fn, nic, nic - 1, npublic);
  return GS_OK;
}

// vk.IC[0] + sum_i publicSignals[i] * vk.IC[i+1]   (groth16.go:283-286, snark.go:330-333)
G1Jac accumulate_ic(const uint64_t* ic, size_t nic, const uint64_t* pub, size_t npublic) {
  G1Jac acc = g1j_from(g1_from_jacobian_std(ic));
  for (size_t i = 0; i < npublic; ++i)
    acc = g1j_add(acc, g1j_mul(g1j_from(g1_from_jacobian_std(ic + 12 * (i + 1))), pub + 4 * i));
  return acc;
}

template <class F>
int host_guarded(F&& f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail(GS_ERR_HIP, "host allocation failed");
  } catch (const std::exception& e) {
    return fail(GS_ERR_ARG, "%s", e.what());
  }
}

const uint64_t kG2Gen[24] = {      // bn128.go:56-83 (Gg2), Z = (1, 0)
    0x46debd5cd992f6edULL, 0x674322d4f75edaddULL, 0x426a00665e5c4479ULL, 0x1800deef121f1e76ULL,
    0x97e485b7aef312c2ULL, 0xf1aa493335a9e712ULL, 0x7260bfb731fb5d25ULL, 0x198e9393920d483aULL,
    0x4ce6cc0166fa7daaULL, 0xe3d1e7690c43d37bULL, 0x4aab71808dcb408fULL, 0x12c85ea5db8c6debULL,
    0x55acdadcd122975bULL, 0xbc4b313370b38ef3ULL, 0xec9e99ad690c3395ULL, 0x090689d0585ff075ULL,
    1, 0, 0, 0, 0, 0, 0, 0};

}  // namespace

extern "C" {

int gs_pairing(const uint64_t g1[12], const uint64_t g2[24], uint64_t out_fq12[48]) {
  return host_guarded([&]() -> int {
    if (!g1 || !g2 || !out_fq12) return fail(GS_ERR_ARG, "gs_pairing: null argument");
    std::vector<G1Aff> ps{g1_from_jacobian_std(g1)};
    std::vector<G2Aff> qs{g2_from_jacobian_std(g2)};
    if (!g1_on_curve(ps[0]) || !g2_on_curve(qs[0])) return fail(GS_ERR_ARG, "gs_pairing: point not on the curve");
    Fp12 f;
    if (!multi_miller_loop(ps, qs, f)) return fail(GS_ERR_ARG, "gs_pairing: G2 point is not of order r");
    f12_to_std(final_exponentiation(f), out_fq12);
    return GS_OK;
  });
}

int gs_pairing_check(const uint64_t* g1, const uint64_t* g2, size_t k, int* ok) {
  return host_guarded([&]() -> int {
    if (!ok || (k && (!g1 || !g2))) return fail(GS_ERR_ARG, "gs_pairing_check: null argument");
    std::vector<G1Aff> ps(k);
    std::vector<G2Aff> qs(k);
    for (size_t i = 0; i < k; ++i) {
      ps[i] = g1_from_jacobian_std(g1 + 12 * i);
      qs[i] = g2_from_jacobian_std(g2 + 24 * i);
    }
    std::vector<int> all(k);
    for (size_t i = 0; i < k; ++i) all[i] = (int)i;
    *ok = product_is_one(ps, qs, all) ? 1 : 0;
    return GS_OK;
  });
}

int gs_verify_set_strict(int on) {
  g_strict.store(on ? 1 : 0);
  return GS_OK;
}

int gs_groth16_verify(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24],
                      const uint64_t vk_g2_delta[24], const uint64_t* vk_ic, size_t nic, const uint64_t* public_signals,
                      size_t npublic, const uint64_t pi_a[12], const uint64_t pi_b[24], const uint64_t pi_c[12], int* ok) {
  return host_guarded([&]() -> int {
    if (!vk_g1_alpha || !vk_g2_beta || !vk_g2_gamma || !vk_g2_delta || !vk_ic || !pi_a || !pi_b || !pi_c || !ok || (npublic && !public_signals))
      return fail(GS_ERR_ARG, "gs_groth16_verify: null argument");
    bool strict;
    if (const int rc = check_signal_count("gs_groth16_verify", nic, npublic, &strict)) return rc;
    // strict: canonical encodings only (x and x + r, X and X + q name the same element: accepting both makes proofs malleable)
    if (strict && (!scalars_canonical(public_signals, npublic) || !coords_canonical(pi_a, 3) || !coords_canonical(pi_b, 6) || !coords_canonical(pi_c, 3))) {
      *ok = 0;
      return GS_OK;
    }
    G1Aff ic = g1j_affine(accumulate_ic(vk_ic, nic, public_signals, npublic));
    // e(A, B) == e(alpha, beta) e(IC, gamma) e(C, delta)   <=>   e(-A, B) e(alpha, beta) e(IC, gamma) e(C, delta) == 1
    std::vector<G1Aff> ps{g1_neg(g1_from_jacobian_std(pi_a)), g1_from_jacobian_std(vk_g1_alpha), ic, g1_from_jacobian_std(pi_c)};
    std::vector<G2Aff> qs{g2_from_jacobian_std(pi_b), g2_from_jacobian_std(vk_g2_beta), g2_from_jacobian_std(vk_g2_gamma),
                          g2_from_jacobian_std(vk_g2_delta)};
    *ok = product_is_one(ps, qs, {0}) ? 1 : 0;                  // PiB is the prover's G2 element
    return GS_OK;
  });
}

int gs_pinocchio_verify(const uint64_t vka[24], const uint64_t vkb[12], const uint64_t vkc[24], const uint64_t g1kbg[12],
                        const uint64_t g2kbg[24], const uint64_t g2kg[24], const uint64_t vkz[24], const uint64_t* vk_ic, size_t nic,
                        const uint64_t* public_signals, size_t npublic, const uint64_t* proof, int* ok, int* failed_check) {
  return host_guarded([&]() -> int {
    if (!vka || !vkb || !vkc || !g1kbg || !g2kbg || !g2kg || !vkz || !vk_ic || !proof || !ok || (npublic && !public_signals))
      return fail(GS_ERR_ARG, "gs_pinocchio_verify: null argument");
    bool strict;
    if (const int rc = check_signal_count("gs_pinocchio_verify", nic, npublic, &strict)) return rc;
    if (strict && (!scalars_canonical(public_signals, npublic) || !coords_canonical(proof, 27))) {
      *ok = 0;
      if (failed_check) *failed_check = 0;
      return GS_OK;
    }
    // proof layout: PiA, PiAp (G1) | PiB (G2) | PiBp, PiC, PiCp, PiH, PiKp (G1)  -- snark.go:59-69
    const G1Aff piA = g1_from_jacobian_std(proof), piAp = g1_from_jacobian_std(proof + 12);
    const G2Aff piB = g2_from_jacobian_std(proof + 24);
    const G1Aff piBp = g1_from_jacobian_std(proof + 48), piC = g1_from_jacobian_std(proof + 60), piCp = g1_from_jacobian_std(proof + 72);
    const G1Aff piH = g1_from_jacobian_std(proof + 84), piKp = g1_from_jacobian_std(proof + 96);
    const G2Aff g2 = g2_from_jacobian_std(kG2Gen);
    const G2Aff Vka = g2_from_jacobian_std(vka), Vkc = g2_from_jacobian_std(vkc), G2Kbg = g2_from_jacobian_std(g2kbg);
    const G2Aff G2Kg = g2_from_jacobian_std(g2kg), Vkz = g2_from_jacobian_std(vkz);
    const G1Aff Vkb = g1_from_jacobian_std(vkb), G1Kbg = g1_from_jacobian_std(g1kbg);
    int bad = 0;
    auto check = [&](int which, std::vector<G1Aff> ps, std::vector<G2Aff> qs) {
      if (!bad && !product_is_one(ps, qs)) bad = which;
    };
    check(1, {piA, g1_neg(piAp)}, {Vka, g2});                       // e(piA, Va) == e(piA', g2)            snark.go:294-304
    if (!bad && (!g2_on_curve(piB) || !g2_in_subgroup(piB))) bad = 2;   // the prover's only G2 element, first used by equation 2
    check(2, {Vkb, g1_neg(piBp)}, {piB, g2});                       // e(Vb, piB) == e(piB', g2)            :306-316
    check(3, {piC, g1_neg(piCp)}, {Vkc, g2});                       // e(piC, Vc) == e(piC', g2)            :318-328
    if (!bad) {
      G1Jac vkx = accumulate_ic(vk_ic, nic, public_signals, npublic);
      G1Jac vkx_a = g1j_add(vkx, g1j_from(piA));
      G1Aff xa = g1j_affine(vkx_a);
      check(4, {xa, g1_neg(piH), g1_neg(piC)}, {piB, Vkz, g2});    // e(Vkx+piA, piB) == e(piH, Vkz) e(piC, g2)   :336-347
      G1Aff xac = g1j_affine(g1j_add(vkx_a, g1j_from(piC)));
      check(5, {xac, G1Kbg, g1_neg(piKp)}, {G2Kbg, piB, G2Kg});    // e(Vkx+piA+piC, g2Kbg) e(g1Kbg, piB) == e(piK, g2Kg)   :353-363
    }
    *ok = bad ? 0 : 1;
    if (failed_check) *failed_check = bad;
    return GS_OK;
  });
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ batch verification
// gs_groth16_verify_batch (include/gosnark_hip.h): many proofs of one key in one randomised product check.  The per-proof work --
// scaling A by the weights, the weighted sum of the C, the subgroup test of the B and the n Miller loops with their product -- runs on
// the device through the library's own entry points; the host forms the npublic + 1 scalars of the public-input sum, runs the three
// key pairs through the multi-Miller loop above and finishes with ONE final exponentiation.

namespace {

// Fr as 4 x 64-bit Montgomery words: the weights z_i = s^i and the sums over them (a few products per proof)
struct Fr { uint64_t v[4]; };
struct FrConsts { uint64_t n0; Fr r2, one; };
inline bool fr_geq_r(const uint64_t* a) { return limbs_geq(a, kRorder); }
inline Fr fr_add(const Fr& a, const Fr& b) {
  Fr r;
  u128 c = 0;
  for (int i = 0; i < 4; ++i) {
    c += (u128)a.v[i] + b.v[i];
    r.v[i] = (uint64_t)c;
    c >>= 64;
  }
  if (c || fr_geq_r(r.v)) limbs_sub(r.v, kRorder);
  return r;
}
const FrConsts& frc() {
  static const FrConsts c = [] {
    FrConsts k;
    uint64_t inv = 1;
    for (int i = 0; i < 6; ++i) inv *= 2 - kRorder[0] * inv;
    k.n0 = 0 - inv;
    Fr t = {{1, 0, 0, 0}};
    for (int i = 0; i < 256; ++i) t = fr_add(t, t);
    k.one = t;
    for (int i = 0; i < 256; ++i) t = fr_add(t, t);
    k.r2 = t;
    return k;
  }();
  return c;
}
// a b 2^-256 mod r (CIOS; a may be any 256-bit value, b < r)
Fr fr_mul(const Fr& a, const Fr& b) {
  const uint64_t n0 = frc().n0;
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; ++i) {
    u128 c = 0;
    for (int j = 0; j < 4; ++j) {
      c += (u128)a.v[j] * b.v[i] + t[j];
      t[j] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[4] = (uint64_t)c;
    t[5] = (uint64_t)(c >> 64);
    const uint64_t m = t[0] * n0;
    c = (u128)m * kRorder[0] + t[0];
    c >>= 64;
    for (int j = 1; j < 4; ++j) {
      c += (u128)m * kRorder[j] + t[j];
      t[j - 1] = (uint64_t)c;
      c >>= 64;
    }
    c += t[4];
    t[3] = (uint64_t)c;
    t[4] = t[5] + (uint64_t)(c >> 64);
  }
  Fr r = {{t[0], t[1], t[2], t[3]}};
  if (t[4] || fr_geq_r(r.v)) limbs_sub(r.v, kRorder);
  return r;
}
Fr fr_from_std(const uint64_t w[4]) {                 // any 256-bit value -> Montgomery residue mod r
  Fr a = {{w[0], w[1], w[2], w[3]}};
  return fr_mul(a, frc().r2);
}
void fr_to_std(const Fr& a, uint64_t w[4]) {
  const Fr one = {{1, 0, 0, 0}};
  const Fr r = fr_mul(a, one);
  memcpy(w, r.v, 32);
}
bool fr_eq(const Fr& a, const Fr& b) { return memcmp(a.v, b.v, 32) == 0; }

// temporary handles of one call: freed on every path
struct HandleBag {
  gs_handle hs[4] = {0, 0, 0, 0};
  ~HandleBag() { for (gs_handle h : hs) if (h) (void)gs_free(h); }
};

// what gs_groth16_verify tests of one proof before its pairings: under strict mode canonical signals and coordinates, and always the
// three points on their curves.  false: the proof's verdict is 0 and the point at infinity travels in place of its points.
bool groth16_proof_passes_screen(bool strict, const uint64_t* pub, size_t npublic, const uint64_t* a, const uint64_t* b, const uint64_t* c) {
  if (strict && (!scalars_canonical(pub, npublic) || !coords_canonical(a, 3) || !coords_canonical(b, 6) || !coords_canonical(c, 3))) return false;
  return g1_on_curve(g1_from_jacobian_std(a)) && g2_on_curve(g2_from_jacobian_std(b)) && g1_on_curve(g1_from_jacobian_std(c));
}

// The per-key host work of the per-proof Groth16 verifiers: the curve tests of the key, the Miller value of e(alpha, beta) and the
// prepared lines of gamma and delta.  False for a key that cannot verify anything, with the point and what is wrong with it.
struct KeyFault { const char *point, *why; };
bool prepare_groth16_key(const uint64_t alpha_w[12], const uint64_t beta_w[24], const uint64_t gamma_w[24], const uint64_t delta_w[24],
                         gs::Groth16KeyWords& out, KeyFault& fault) {
  const auto refuse = [&](const char* point, const char* why) { fault = KeyFault{point, why}; return false; };
  const G1Aff alpha = g1_from_jacobian_std(alpha_w);
  const G2Aff beta = g2_from_jacobian_std(beta_w), gamma = g2_from_jacobian_std(gamma_w), delta = g2_from_jacobian_std(delta_w);
  if (!g1_on_curve(alpha)) return refuse("alpha", "is not on the curve");
  if (!g2_on_curve(beta)) return refuse("beta", "is not on the twist");
  if (!g2_on_curve(gamma)) return refuse("gamma", "is not on the twist");
  if (!g2_on_curve(delta)) return refuse("delta", "is not on the twist");
  Fp12 fab;
  if (!multi_miller_loop({alpha}, {beta}, fab)) return refuse("beta", "is not of order r (a degenerate step in its Miller loop)");
  f12_to_std(fab, out.ab);
  out.lines.assign(2 * gs::kLineStd, 0);
  out.skip_gamma = gamma.inf;
  out.skip_delta = delta.inf;
  std::vector<uint64_t> list;
  if (!gamma.inf) {
    if (!prepare_g2_lines(gamma, list)) return refuse("gamma", "is not of order r (a degenerate step in its prepared lines)");
    memcpy(out.lines.data(), list.data(), gs::kLineStd * 8);
  }
  if (!delta.inf) {
    if (!prepare_g2_lines(delta, list)) return refuse("delta", "is not of order r (a degenerate step in its prepared lines)");
    memcpy(out.lines.data() + gs::kLineStd, list.data(), gs::kLineStd * 8);
  }
  return true;
}

// What the two per-proof Groth16 calls share once their keys stand: per proof what the single verifier tests before its pairings, the
// permutation into the slot order of verify_plan.h (one key per one-wave workgroup; infinity in bad and in padded slots, because the
// uploads refuse a whole array for one point off its curve), the device run and the fold into ok_each / nbad.  npublic: per key.
int groth16_verdicts(const char* fn, const gs::Groth16CallKeys& keys, const uint32_t* npublic, const uint32_t* key_of_proof, bool strict,
                     const uint64_t* public_signals, const uint64_t* pi_a, const uint64_t* pi_b, const uint64_t* pi_c, size_t n, int* ok_each,
                     uint64_t* nbad) {
  VerifyPlan plan;
  if (plan_verify_slots(key_of_proof, n, keys.keys ? keys.nkeys : 1, npublic, plan) != kVpOk)
    return fail(GS_ERR_SHAPE, "%s: %zu proofs need more than 2^32 slots (64 per key and started group): pass them in windows", fn, n);
  if (plan.nsignals && !public_signals) return fail(GS_ERR_ARG, "%s: null argument", fn);
  const size_t slots = plan.proof_of_slot.size();
  std::vector<uint64_t> a(12 * slots, 0), b(24 * slots, 0), c(12 * slots, 0), pub(plan.nsignals ? 4 * (size_t)plan.nsignals : 4, 0);
  std::vector<const uint64_t*> pub_of(n);
  {
    const uint64_t* at = public_signals;
    for (size_t i = 0; i < n; ++i) { pub_of[i] = at; at += 4 * (size_t)npublic[key_of_proof[i]]; }
  }
  std::vector<char> bad(n, 0);
  for (size_t g = 0; g < plan.groups.size(); ++g) {
    const size_t np = npublic[plan.groups[g].key];
    for (uint32_t l = 0; l < plan.groups[g].valid; ++l) {
      const size_t s = g * kVpLanes + l, i = plan.proof_of_slot[s];
      if (np) memcpy(pub.data() + 4 * ((size_t)plan.groups[g].sig_off + l * np), pub_of[i], 32 * np);
      if (!groth16_proof_passes_screen(strict, pub_of[i], np, pi_a + 12 * i, pi_b + 24 * i, pi_c + 12 * i)) { bad[i] = 1; continue; }
      memcpy(a.data() + 12 * s, pi_a + 12 * i, 96);
      memcpy(b.data() + 24 * s, pi_b + 24 * i, 192);
      memcpy(c.data() + 12 * s, pi_c + 12 * i, 96);
    }
  }
  HandleBag bag;
  gs_handle *ha = &bag.hs[0], *hb = &bag.hs[1], *hc = &bag.hs[2];
  int rc;
  if ((rc = gs_g1_upload(a.data(), slots, ha)) != GS_OK) return rc;
  if ((rc = gs_g2_upload(b.data(), slots, hb)) != GS_OK) return rc;
  if ((rc = gs_g1_upload(c.data(), slots, hc)) != GS_OK) return rc;
  std::vector<int> member(slots), one(slots);
  rc = gs::groth16_verify_slots_device(fn, keys, *ha, *hb, *hc, plan.groups.data(), plan.groups.size(), pub.data(), plan.nsignals, member.data(),
                                       one.data());
  if (rc != GS_OK) return rc;
  uint64_t count = 0;
  for (size_t i = 0; i < n; ++i) {
    const size_t s = plan.slot_of_proof[i];
    ok_each[i] = (!bad[i] && member[s] && one[s]) ? 1 : 0;
    count += ok_each[i] ? 0 : 1;
  }
  if (nbad) *nbad = count;
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_groth16_verify_batch(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24],
                            const uint64_t vk_g2_delta[24], const uint64_t* vk_ic, size_t nic, const uint64_t* public_signals, size_t npublic,
                            const uint64_t* pi_a, const uint64_t* pi_b, const uint64_t* pi_c, size_t nproofs, const uint64_t challenge[4], int* ok) {
  return host_guarded([&]() -> int {
    const char* fn = "gs_groth16_verify_batch";
    const size_t n = nproofs;
    if (!vk_g1_alpha || !vk_g2_beta || !vk_g2_gamma || !vk_g2_delta || !vk_ic || !challenge || !ok || (n && (!pi_a || !pi_b || !pi_c)) ||
        (n && npublic && !public_signals))
      return fail(GS_ERR_ARG, "%s: null argument", fn);
    bool strict;
    if (const int shape = check_signal_count(fn, nic, npublic, &strict)) return shape;
    const Fr s = fr_from_std(challenge);
    if (fr_eq(s, Fr{{0, 0, 0, 0}}) || fr_eq(s, frc().one))
      return fail(GS_ERR_ARG, "%s: the challenge is 0 or 1 mod r: every weight would be the same (draw it at random, after the proofs are fixed)", fn);
    if (!n) {
      *ok = 1;
      return GS_OK;
    }
    const auto reject = [&]() -> int { *ok = 0; return GS_OK; };        // *ok is written by the paths that return GS_OK, and only then
    if (strict && (!scalars_canonical(public_signals, n * npublic) || !coords_canonical(pi_a, 3 * n) || !coords_canonical(pi_b, 6 * n) ||
                   !coords_canonical(pi_c, 3 * n)))
      return reject();
    // the weights z_i = s^i in standard form, their sum, and sum_i z_i pub_ij per public input
    std::vector<uint64_t> z(4 * n);
    std::vector<Fr> wsum(npublic + 1, Fr{{0, 0, 0, 0}});
    Fr zi = frc().one;
    for (size_t i = 0; i < n; ++i) {
      fr_to_std(zi, z.data() + 4 * i);
      wsum[0] = fr_add(wsum[0], zi);
      for (size_t j = 0; j < npublic; ++j) wsum[j + 1] = fr_add(wsum[j + 1], fr_mul(fr_from_std(public_signals + 4 * (i * npublic + j)), zi));
      zi = fr_mul(zi, s);
    }
    // the proofs' points; a point off its curve is a rejected batch, as it is a rejected proof for the single verifier
    HandleBag bag;
    gs_handle *ha = &bag.hs[0], *hb = &bag.hs[1], *hc = &bag.hs[2], *hna = &bag.hs[3];
    int rc = gs_g1_upload(pi_a, n, ha);
    if (rc == GS_ERR_ARG) return reject();
    if (rc != GS_OK) return rc;
    rc = gs_g2_upload(pi_b, n, hb);
    if (rc == GS_ERR_ARG) return reject();
    if (rc != GS_OK) return rc;
    rc = gs_g1_upload(pi_c, n, hc);
    if (rc == GS_ERR_ARG) return reject();
    if (rc != GS_OK) return rc;
    uint64_t nbad = 0, first_bad = 0;
    if ((rc = gs_g2_subgroup_check(*hb, 0, n, &nbad, &first_bad)) != GS_OK) return rc;
    if (nbad) return reject();
    // -z_i A_i on the device, sum_i z_i C_i as one MSM
    uint64_t rm1[4], sw[4];
    memcpy(rm1, kRorder, 32);
    rm1[0] -= 1;
    fr_to_std(s, sw);
    if ((rc = gs_g1_scale_powers(*ha, 0, n, rm1, sw, hna)) != GS_OK) return rc;
    uint64_t csum[8];
    int cinf = 0;
    if ((rc = gs_msm_g1(*hc, z.data(), 0, n, csum, &cinf)) != GS_OK) return rc;
    // the key's three pairs on the host: (sum z) alpha | beta,  sum_j wsum_j IC[j] | gamma,  sum z_i C_i | delta
    uint64_t k[4];
    fr_to_std(wsum[0], k);
    const G1Aff alpha = g1j_affine(g1j_mul(g1j_from(g1_from_jacobian_std(vk_g1_alpha)), k));
    G1Jac vkx = g1j_mul(g1j_from(g1_from_jacobian_std(vk_ic)), k);
    for (size_t j = 0; j < npublic; ++j) {
      fr_to_std(wsum[j + 1], k);
      vkx = g1j_add(vkx, g1j_mul(g1j_from(g1_from_jacobian_std(vk_ic + 12 * (j + 1))), k));
    }
    const G1Aff csum_pt = cinf ? G1Aff{Fp{{0, 0, 0, 0}}, Fp{{0, 0, 0, 0}}, true} : G1Aff{fp_from_std(csum), fp_from_std(csum + 4), false};
    const std::vector<G1Aff> ps{alpha, g1j_affine(vkx), csum_pt};
    const std::vector<G2Aff> qs{g2_from_jacobian_std(vk_g2_beta), g2_from_jacobian_std(vk_g2_gamma), g2_from_jacobian_std(vk_g2_delta)};
    for (const G1Aff& p : ps)
      if (!g1_on_curve(p)) return reject();
    for (const G2Aff& q : qs)
      if (!g2_on_curve(q)) return reject();
    Fp12 fkey;
    if (!multi_miller_loop(ps, qs, fkey)) return reject();
    // the n Miller values of e(-z_i A_i, B_i) and their product on the device
    Fp12 f;
    if ((rc = gs::miller_product(fn, *hna, 0, *hb, 0, n, &f)) != GS_OK) return rc;
    *ok = f12_eq(final_exponentiation(f12_mul(f, fkey)), f12_one()) ? 1 : 0;
    return GS_OK;
  });
}

// gs_groth16_verify_each (include/gosnark_hip.h): the verdict of gs_groth16_verify for every proof of a batch, on the device.  The host
// does what is O(1) per call or a few products per proof: the key (prepare_groth16_key; it lives for this call only) and the screening
// of the 3n points (groth16_verdicts).
int gs_groth16_verify_each(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24],
                           const uint64_t vk_g2_delta[24], const uint64_t* vk_ic, size_t nic, const uint64_t* public_signals, size_t npublic,
                           const uint64_t* pi_a, const uint64_t* pi_b, const uint64_t* pi_c, size_t nproofs, int* ok_each, uint64_t* nbad) {
  return host_guarded([&]() -> int {
    const char* fn = "gs_groth16_verify_each";
    const size_t n = nproofs;
    if (!vk_g1_alpha || !vk_g2_beta || !vk_g2_gamma || !vk_g2_delta || !vk_ic || (n && (!pi_a || !pi_b || !pi_c || !ok_each)) ||
        (n && npublic && !public_signals))
      return fail(GS_ERR_ARG, "%s: null argument", fn);
    bool strict;
    if (const int shape = check_signal_count(fn, nic, npublic, &strict)) return shape;
    if (!n) {
      if (nbad) *nbad = 0;
      return GS_OK;
    }
    // the IC points go up first: without a device this is where the call ends, before any work and with nothing written
    HandleBag bag;
    gs_handle* hic = &bag.hs[0];
    const int rc = gs_g1_upload(vk_ic, nic, hic);
    if (rc != GS_OK && rc != GS_ERR_ARG) return rc;
    // the key: a point off its curve (GS_ERR_ARG for one of the IC) or a degenerate step makes every verdict 0, as it makes
    // gs_groth16_verify answer 0 for every proof
    gs::Groth16KeyWords words;
    KeyFault fault;
    if (rc == GS_ERR_ARG || !prepare_groth16_key(vk_g1_alpha, vk_g2_beta, vk_g2_gamma, vk_g2_delta, words, fault)) {
      for (size_t i = 0; i < n; ++i) ok_each[i] = 0;
      if (nbad) *nbad = n;
      return GS_OK;
    }
    if (npublic >= 0xffffffffull) return fail(GS_ERR_SHAPE, "%s: %zu proofs, indices are 32 bits", fn, n);
    gs::Groth16CallKeys key;
    key.ic = *hic;
    key.npublic = npublic;
    key.words = &words;
    const uint32_t np = (uint32_t)npublic;
    const std::vector<uint32_t> key_of_proof(n, 0);                     // one key: the trivial plan
    return groth16_verdicts(fn, key, &np, key_of_proof.data(), strict, public_signals, pi_a, pi_b, pi_c, n, ok_each, nbad);
  });
}

// gs_groth16_vk_create (include/gosnark_hip.h): the per-key host work of gs_groth16_verify_each, done once and kept on the device
// beside the IC points.  Where gs_groth16_verify_each answers a key that cannot verify anything with all-zero verdicts, this call
// refuses to install it.
int gs_groth16_vk_create(const uint64_t vk_g1_alpha[12], const uint64_t vk_g2_beta[24], const uint64_t vk_g2_gamma[24],
                         const uint64_t vk_g2_delta[24], const uint64_t* vk_ic, size_t nic, gs_handle* out) {
  return host_guarded([&]() -> int {
    const char* fn = "gs_groth16_vk_create";
    if (!vk_g1_alpha || !vk_g2_beta || !vk_g2_gamma || !vk_g2_delta || !out || (nic && !vk_ic)) return fail(GS_ERR_ARG, "%s: null argument", fn);
    if (!nic) return fail(GS_ERR_SHAPE, "%s: a key has at least IC[0]", fn);
    // the IC points go up first: without a device this is where the call ends, before any work and with nothing written
    HandleBag bag;
    gs_handle* hic = &bag.hs[0];
    int rc = gs_g1_upload(vk_ic, nic, hic);
    if (rc == GS_ERR_ARG) {
      for (size_t j = 0; j < nic; ++j)
        if (!g1_on_curve(g1_from_jacobian_std(vk_ic + 12 * j))) return fail(GS_ERR_ARG, "%s: IC[%zu] is not on the curve", fn, j);
    }
    if (rc != GS_OK) return rc;
    gs::Groth16KeyWords words;
    KeyFault fault;
    if (!prepare_groth16_key(vk_g1_alpha, vk_g2_beta, vk_g2_gamma, vk_g2_delta, words, fault))
      return fail(GS_ERR_ARG, "%s: %s %s", fn, fault.point, fault.why);
    gs_handle h = 0;
    if ((rc = gs::groth16_vk_install(fn, *hic, nic, words, &h)) != GS_OK) return rc;
    *out = h;
    return GS_OK;
  });
}

// gs_groth16_verify_each_keys (include/gosnark_hip.h): gs_groth16_verify_each for proofs that each name their key.  The keys are
// prepared objects, so what is left for the host is per proof (groth16_verdicts).
int gs_groth16_verify_each_keys(const gs_handle* keys, size_t nkeys, const uint32_t* key_of_proof, const uint64_t* public_signals,
                                const uint64_t* pi_a, const uint64_t* pi_b, const uint64_t* pi_c, size_t nproofs, int* ok_each, uint64_t* nbad) {
  return host_guarded([&]() -> int {
    const char* fn = "gs_groth16_verify_each_keys";
    const size_t n = nproofs;
    if ((nkeys && !keys) || (n && (!key_of_proof || !pi_a || !pi_b || !pi_c || !ok_each))) return fail(GS_ERR_ARG, "%s: null argument", fn);
    if (!n) {
      if (nbad) *nbad = 0;
      return GS_OK;
    }
    for (size_t i = 0; i < n; ++i)
      if (key_of_proof[i] >= nkeys) return fail(GS_ERR_ARG, "%s: key_of_proof[%zu] = %u, the call has %zu keys", fn, i, key_of_proof[i], nkeys);
    for (size_t k = 1; k < nkeys; ++k)
      if (handle_device(keys[k]) != handle_device(keys[0]))
        return fail(GS_ERR_ARG, "%s: keys[%zu] lives on logical device %d, keys[0] on %d", fn, k, handle_device(keys[k]), handle_device(keys[0]));
    // the keys' signal counts: without a device this is where the call ends, before any work and with nothing written
    std::vector<uint32_t> npublic(nkeys);
    const int rc = gs::groth16_vk_info(fn, keys, nkeys, npublic.data());
    if (rc != GS_OK) return rc;
    const int here = gs_get_device();                                   // the proofs' arrays are created where the calling thread works
    if (handle_device(keys[0]) != here)
      return fail(GS_ERR_ARG, "%s: the keys live on logical device %d, the calling thread works on %d (gs_set_device)", fn, handle_device(keys[0]), here);
    gs::Groth16CallKeys prepared;
    prepared.keys = keys;
    prepared.nkeys = nkeys;
    return groth16_verdicts(fn, prepared, npublic.data(), key_of_proof, g_strict.load() != 0, public_signals, pi_a, pi_b, pi_c, n, ok_each, nbad);
  });
}

// gs_pinocchio_verify_each (include/gosnark_hip.h): gs_pinocchio_verify's verdict and first failing equation for every proof of a batch,
// on the device.  The host does what is O(1) per call or a few products per proof: the key (curve tests, the six prepared lists) and the
// screening of the 8n proof points, because the uploads refuse a whole array for one point off its curve: the point at infinity travels in
// its place and the equations that use it are marked failed.  The device answers "is equation e of proof i one" and "is PiB_i in G2";
// the fold below puts them in the reference's order.
int gs_pinocchio_verify_each(const uint64_t vka[24], const uint64_t vkb[12], const uint64_t vkc[24], const uint64_t g1kbg[12], const uint64_t g2kbg[24],
                             const uint64_t g2kg[24], const uint64_t vkz[24], const uint64_t* vk_ic, size_t nic, const uint64_t* public_signals,
                             size_t npublic, const uint64_t* proofs, size_t nproofs, int* ok_each, int* failed_each, uint64_t* nbad) {
  return host_guarded([&]() -> int {
    const char* fn = "gs_pinocchio_verify_each";
    const size_t n = nproofs;
    if (!vka || !vkb || !vkc || !g1kbg || !g2kbg || !g2kg || !vkz || !vk_ic || (n && (!proofs || !ok_each)) || (n && npublic && !public_signals))
      return fail(GS_ERR_ARG, "%s: null argument", fn);
    bool strict;
    if (const int shape = check_signal_count(fn, nic, npublic, &strict)) return shape;
    if (!n) {
      if (nbad) *nbad = 0;
      return GS_OK;
    }
    const auto eq = [](int e) { return 1u << e; };                      // bit e = equation e (1..5) does not hold
    // the IC points go up first: without a device this is where the call ends, before any work and with nothing written.  The host
    // verifier sums them unchecked and then finds vkx + PiA off the curve: an IC point off its curve that a proof uses (IC_0, or
    // IC_{j+1} with a nonzero signal j) fails that proof's equations 4 and 5; infinity travels in its place.
    HandleBag bag;
    gs_handle *hg1 = &bag.hs[0], *hb = &bag.hs[1], *hic = &bag.hs[2], *hkey = &bag.hs[3];
    std::vector<uint64_t> ic(vk_ic, vk_ic + 12 * nic);
    std::vector<char> ic_bad(npublic + 1, 0);
    for (size_t j = 0; j <= npublic; ++j)
      if (!g1_on_curve(g1_from_jacobian_std(vk_ic + 12 * j))) {
        ic_bad[j] = 1;
        memset(ic.data() + 12 * j, 0, 96);
      }
    for (size_t j = npublic + 1; j < nic; ++j)                          // not used by any proof
      if (!g1_on_curve(g1_from_jacobian_std(vk_ic + 12 * j))) memset(ic.data() + 12 * j, 0, 96);
    int rc = gs_g1_upload(ic.data(), nic, hic);
    if (rc != GS_OK) return rc;
    // the key: a point off its curve fails every equation that uses it, for every proof.  A G2 point with a degenerate step (on the
    // twist, of small order) fails them where its partner in G1 is finite, as multi_miller_loop does; its list is left out.
    unsigned key_fail = 0, skip_mask = 0;
    uint64_t key_g1[24];
    memcpy(key_g1, vkb, 96);
    memcpy(key_g1 + 12, g1kbg, 96);
    if (!g1_on_curve(g1_from_jacobian_std(vkb))) { key_fail |= eq(2); memset(key_g1, 0, 96); }
    if (!g1_on_curve(g1_from_jacobian_std(g1kbg))) { key_fail |= eq(5); memset(key_g1 + 12, 0, 96); }
    enum { kVka = 0, kVkc, kVkz, kG2Kbg, kG2Kg, kGen, kLists };        // pairing_device.hip, the order of the lists
    const uint64_t* key_g2[kLists] = {vka, vkc, vkz, g2kbg, g2kg, kG2Gen};
    const unsigned uses[kLists] = {eq(1), eq(3), eq(4), eq(5), eq(5), 0};
    bool degenerate[kLists] = {false, false, false, false, false, false};
    std::vector<uint64_t> lines(kLists * kLineStd, 0), one_list;
    for (int l = 0; l < kLists; ++l) {
      const G2Aff q = g2_from_jacobian_std(key_g2[l]);
      if (q.inf) { skip_mask |= 1u << l; continue; }
      if (!g2_on_curve(q)) { key_fail |= uses[l]; skip_mask |= 1u << l; continue; }
      if (!prepare_g2_lines(q, one_list)) { degenerate[l] = true; skip_mask |= 1u << l; continue; }
      memcpy(lines.data() + l * kLineStd, one_list.data(), kLineStd * 8);
    }
    // the proofs: per proof what the single verifier tests before and inside its product checks
    static const struct { int at; unsigned uses; } kG1[7] = {{0, 1u << 1 | 1u << 4 | 1u << 5}, {12, 1u << 1}, {48, 1u << 2}, {60, 1u << 3 | 1u << 4 | 1u << 5},
                                                             {72, 1u << 3}, {84, 1u << 4}, {96, 1u << 5}};   // PiA PiAp PiBp PiC PiCp PiH PiKp
    std::vector<uint64_t> g1(7 * 12 * n), b(24 * n);
    std::vector<unsigned> forced(n, key_fail);
    std::vector<char> refused(n, 0);
    for (size_t i = 0; i < n; ++i) {
      const uint64_t* proof = proofs + 108 * i;
      const uint64_t* pub = public_signals + 4 * i * npublic;
      if (strict && (!scalars_canonical(pub, npublic) || !coords_canonical(proof, 27))) {
        refused[i] = 1;
        for (int k = 0; k < 7; ++k) memset(g1.data() + 12 * (k * n + i), 0, 96);
        memset(b.data() + 24 * i, 0, 192);
        continue;
      }
      bool finite[7];
      for (int k = 0; k < 7; ++k) {
        uint64_t* dst = g1.data() + 12 * (k * n + i);
        const G1Aff p = g1_from_jacobian_std(proof + kG1[k].at);
        finite[k] = !p.inf;
        if (g1_on_curve(p)) memcpy(dst, proof + kG1[k].at, 96);
        else { forced[i] |= kG1[k].uses; memset(dst, 0, 96); }
      }
      if (g2_on_curve(g2_from_jacobian_std(proof + 24))) memcpy(b.data() + 24 * i, proof + 24, 192);
      else { forced[i] |= eq(2) | eq(4) | eq(5); memset(b.data() + 24 * i, 0, 192); }
      bool ic_used = ic_bad[0] != 0;
      for (size_t j = 0; j < npublic; ++j)
        if (ic_bad[j + 1] && (pub[4 * j] | pub[4 * j + 1] | pub[4 * j + 2] | pub[4 * j + 3])) ic_used = true;
      if (ic_used) forced[i] |= eq(4) | eq(5);
      if (degenerate[kVka] && finite[0]) forced[i] |= eq(1);
      if (degenerate[kVkc] && finite[3]) forced[i] |= eq(3);
      if (degenerate[kVkz] && finite[5]) forced[i] |= eq(4);
      if (degenerate[kG2Kg] && finite[6]) forced[i] |= eq(5);
      if (degenerate[kG2Kbg] && !(forced[i] & eq(5))) {                 // its partner is vkx + PiA + PiC: formed here, on this path only
        const G1Jac sum = g1j_add(g1j_add(accumulate_ic(vk_ic, nic, pub, npublic), g1j_from(g1_from_jacobian_std(proof))),
                                  g1j_from(g1_from_jacobian_std(proof + 60)));
        if (!fp_is_zero(sum.z)) forced[i] |= eq(5);
      }
    }
    if ((rc = gs_g1_upload(g1.data(), 7 * n, hg1)) != GS_OK) return rc;
    if ((rc = gs_g2_upload(b.data(), n, hb)) != GS_OK) return rc;
    if ((rc = gs_g1_upload(key_g1, 2, hkey)) != GS_OK) return rc;
    std::vector<int> member(n), one(5 * n);
    rc = gs::pinocchio_verify_each_device(fn, *hg1, *hb, *hic, *hkey, public_signals, npublic, n, lines.data(), skip_mask, member.data(), one.data());
    if (rc != GS_OK) return rc;
    // the fold, in gs_pinocchio_verify's order: equation 1, PiB's membership (reported as 2), equations 2 .. 5
    uint64_t count = 0;
    for (size_t i = 0; i < n; ++i) {
      int bad = 0;
      if (!refused[i]) {
        unsigned fails = forced[i];
        for (int e = 1; e <= 5; ++e)
          if (!one[(size_t)(e - 1) * n + i]) fails |= eq(e);
        if (!member[i]) fails |= eq(2);
        for (int e = 5; e >= 1; --e)
          if (fails & eq(e)) bad = e;
      }
      ok_each[i] = (refused[i] || bad) ? 0 : 1;
      if (failed_each) failed_each[i] = bad;
      count += ok_each[i] ? 0 : 1;
    }
    if (nbad) *nbad = count;
    return GS_OK;
  });
}

}  // extern "C"
