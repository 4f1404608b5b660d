// Checking a Groth16 key against its circuit and a powers-of-tau transcript, and a transcript against itself (include/gosnark_hip.h,
// "checking a key and a transcript").  Every array of the key is a linear image of the transcript's points, so a random linear
// combination of a section -- one MSM over the challenge vector rho_i = s^(i+1) -- must equal a combination of transcript points whose
// scalars are the prover's own pipeline with rho in the witness's place: sparse rows times a vector (spmv_dev), values -> coefficients
// (domain_coeffs_dev), MSM.  Only scalars go through a transform.  The device code that is new here is small: the masks rho^pub / rho^prv,
// the twist c_t = (1/2) v^(-t) q_t of the H check, the vector compare; the weight is in kernels the library already had.
//   gs_groth16_key_check   coefs A, coefs B, A, B1, B2, IC, C, H against circuit and transcript
//   gs_ptau_check          the transcript's first 2^log2_n powers: one tau in both groups, geometric alpha / beta sections, betaG2
//   gs_g1 / g2_lagrange_levels_check   a prepared section (the Lagrange bases of every power-of-two domain) against its powers
// Every MSM is summed table-free whatever the table policy (each array is used once); the pairing comparisons run here, on the host
// (pairing.h), so a C or Go caller gets the whole answer from one call.
#include <algorithm>
#include <vector>

#include "domain.h"
#include "ec_stage.h"
#include "msm.h"
#include "pairing.h"
#include "poly.h"
#include "prove.h"

using namespace gs;

namespace {

GS_HD Fe<ModR, 6> zc_load(const uint32_t* __restrict__ p) {
  uint32_t w[8];
  load_words(p, w);
  return unpack32<ModR>(w);
}
GS_HD void zc_store(uint32_t* __restrict__ p, const Fe<ModR, 1>& a) {
  uint32_t w[8];
  pack32<ModR>(a, w);
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = w[j];
}

// pub[i] = i <= npublic ? rho[i] : 0,  prv[i] = rho[i] - pub[i]
__global__ void __launch_bounds__(256) k_zc_masks(const uint32_t* __restrict__ rho, uint32_t n, uint32_t npublic, uint32_t* __restrict__ pub,
                                                  uint32_t* __restrict__ prv) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const bool is_pub = i <= npublic;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const uint32_t w = rho[(size_t)i * 8 + j];
    pub[(size_t)i * 8 + j] = is_pub ? w : 0u;
    prv[(size_t)i * 8 + j] = is_pub ? 0u : w;
  }
}

// out[t] = q[t] * tw[t] (both standard form, any representative), canonical
__global__ void __launch_bounds__(256) k_zc_twist(const uint32_t* __restrict__ q, const uint32_t* __restrict__ tw, uint32_t n, uint32_t* __restrict__ out) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  zc_store(out + (size_t)t * 8, canon(mul(to_mont(zc_load(q + (size_t)t * 8)), zc_load(tw + (size_t)t * 8))));
}

// *count += the rows i < n with a[i] != b[i] mod r
__global__ void __launch_bounds__(256) k_zc_differ(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b, uint32_t n, uint32_t* __restrict__ count) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const Fe<ModR, 1> x = canon(zc_load(a + (size_t)i * 8)), y = canon(zc_load(b + (size_t)i * 8));
  bool differ = false;
#pragma unroll
  for (int l = 0; l < NL; ++l) differ = differ || x.l[l] != y.l[l];
  if (differ) atomicAdd(count, 1u);
}

// ---- the sums -----------------------------------------------------------------------------------------------------------------------
struct Job { Bases* b; size_t off; };

// A table-free plan over n scalars and the groups that share it: sum_i scal[i] * b[off + i] for every job, G1 jobs in one launch
// sequence (at most 4: the workspace sets of a blocking call), G2 jobs in another.
struct SharedPlan {
  Ctx& c;
  MsmPlan plan;
  uint32_t n;
  SharedPlan(Ctx& ctx, const uint32_t* scal, size_t n_, int g1_jobs, int g2_jobs) : c(ctx), n((uint32_t)n_) {
    if (!n) return;
    std::vector<LaunchShape> users;
    if (g1_jobs) users.push_back({g1_jobs, false});
    if (g2_jobs) users.push_back({g2_jobs, true});
    PhaseTimer tp(c.stream);
    build_plan(c, 2 * c.blocking_slot(), scal, n, plan, users, 0, true);
    tp.stop();
    c.timing.plan_ms += tp.ms();
  }
  template <class T>
  std::vector<Xyzz<T>> sum(const std::vector<Job>& jobs) {
    std::vector<Xyzz<T>> out(jobs.size(), xyzz_inf<T>());
    if (!n || jobs.empty()) return out;
    std::vector<MsmBase> bases;
    for (const Job& j : jobs) {
      if (j.off > j.b->n || n > j.b->n - j.off) throw HipError{hipErrorInvalidValue, "key check: a sum runs past its base array", __LINE__};
      bases.push_back(MsmBase{nullptr, j.off, j.b->buf.as<uint32_t>(), j.b->n});
    }
    if constexpr (T::kWords == 8) msm_run_g1(c, plan, bases, out); else msm_run_g2(c, plan, bases, out);
    return out;
  }
};

// ---- results ------------------------------------------------------------------------------------------------------------------------
void set_side(uint64_t (&w)[16], int32_t& inf, int32_t& g2, const G1Xyzz& p) {
  memset(w, 0, sizeof w);
  uint64_t a[8];
  inf = g1_to_affine_std(p, a) ? 1 : 0;
  g2 = 0;
  if (!inf) memcpy(w, a, sizeof a);
}
void set_side(uint64_t (&w)[16], int32_t& inf, int32_t& g2, const G2Xyzz& p) {
  memset(w, 0, sizeof w);
  uint64_t a[16];
  inf = g2_to_affine_std(p, a) ? 1 : 0;
  g2 = 1;
  if (!inf) memcpy(w, a, sizeof a);
}
using namespace gs::pairing;

void set_side(uint64_t (&w)[16], int32_t& inf, int32_t& g2, const G1Aff& p) {
  memset(w, 0, sizeof w);
  inf = p.inf ? 1 : 0;
  g2 = 0;
  if (!p.inf) { fp_to_std(p.x, w); fp_to_std(p.y, w + 4); }
}
void set_side(uint64_t (&w)[16], int32_t& inf, int32_t& g2, const G2Aff& p) {
  memset(w, 0, sizeof w);
  inf = p.inf ? 1 : 0;
  g2 = 1;
  if (!p.inf) { fp_to_std(p.x.c0, w); fp_to_std(p.x.c1, w + 4); fp_to_std(p.y.c0, w + 8); fp_to_std(p.y.c1, w + 12); }
}

template <class L, class Rt>
void set_points(gs_check_result& r, const L& lhs, const Rt& rhs) {
  set_side(r.lhs, r.lhs_inf, r.lhs_g2, lhs);
  set_side(r.rhs, r.rhs_inf, r.rhs_g2, rhs);
}
bool same_point(const gs_check_result& r) {
  return r.lhs_g2 == r.rhs_g2 && r.lhs_inf == r.rhs_inf && memcmp(r.lhs, r.rhs, sizeof r.lhs) == 0;
}

G1Aff pair_g1(const uint64_t* w, int inf) { return G1Aff{fp_from_std(w), fp_from_std(w + 4), inf != 0}; }
G2Aff pair_g2(const uint64_t* w, int inf) { return G2Aff{Fp2{fp_from_std(w), fp_from_std(w + 4)}, Fp2{fp_from_std(w + 8), fp_from_std(w + 12)}, inf != 0}; }
const uint64_t kG1GenAffine[8] = {1, 0, 0, 0, 2, 0, 0, 0};
const uint64_t kG2GenAffine[16] = {      // the generator of G2 (EIP-197), x.c0 | x.c1 | y.c0 | y.c1
    0x46debd5cd992f6edULL, 0x674322d4f75edaddULL, 0x426a00665e5c4479ULL, 0x1800deef121f1e76ULL,
    0x97e485b7aef312c2ULL, 0xf1aa493335a9e712ULL, 0x7260bfb731fb5d25ULL, 0x198e9393920d483aULL,
    0x4ce6cc0166fa7daaULL, 0xe3d1e7690c43d37bULL, 0x4aab71808dcb408fULL, 0x12c85ea5db8c6debULL,
    0x55acdadcd122975bULL, 0xbc4b313370b38ef3ULL, 0xec9e99ad690c3395ULL, 0x090689d0585ff075ULL};
// a G2 point that takes part in a pairing: on the twist and of order r (gs_pairing_check's rule)
bool g2_usable(const G2Aff& q) { return g2_on_curve(q) && g2_in_subgroup(q); }
// e(p1, q1) == e(p2, q2) for usable q1, q2: one product of two pairs with a shared final exponentiation
bool pairings_equal(const G1Aff& p1, const G2Aff& q1, const G1Aff& p2, const G2Aff& q2) {
  if (!g1_on_curve(p1) || !g1_on_curve(p2) || !g2_usable(q1) || !g2_usable(q2)) return false;
  Fp12 f;
  if (!multi_miller_loop({p1, g1_neg(p2)}, {q1, q2}, f)) return false;
  return f12_eq(final_exponentiation(f), f12_one());
}
void finish_report(gs_check_report& rep) {
  rep.failed = 0;
  for (uint32_t i = 0; i < rep.nchecks; ++i)
    if (!rep.check[i].ok) rep.failed |= 1u << i;
}

// a window table the handle owned goes: the check sums table-free and leaves none behind
void drop_table(Bases* b) { if (b->table) { b->table->release(); b->table.reset(); } }

bool challenge_words(const uint64_t s[4], uint64_t out[4]) {
  uint32_t w[8];
  fr_canon_words(s, w);
  bool zero = true;
  for (int i = 0; i < 4; ++i) { out[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32); zero = zero && out[i] == 0; }
  return !zero;
}

// ---- the key ------------------------------------------------------------------------------------------------------------------------
int key_check_impl(Ctx& c, const gs_key_check_input& in, gs_check_report& rep) {
  const char* fn = "gs_groth16_key_check";
  Bases* A = c.get<Bases>(in.a, Kind::G1Bases);
  Bases* B1 = c.get<Bases>(in.b1, Kind::G1Bases);
  Bases* B2 = c.get<Bases>(in.b2, Kind::G2Bases);
  Bases* IC = c.get<Bases>(in.ic, Kind::G1Bases);
  Bases* C = c.get<Bases>(in.c, Kind::G1Bases);
  Bases* H = c.get<Bases>(in.h, Kind::G1Bases);
  Bases* T1 = c.get<Bases>(in.tau_g1, Kind::G1Bases);
  Bases* T2 = c.get<Bases>(in.tau_g2, Kind::G2Bases);
  Bases* Ta = c.get<Bases>(in.alpha_tau_g1, Kind::G1Bases);
  Bases* Tb = c.get<Bases>(in.beta_tau_g1, Kind::G1Bases);
  R1csObj* ksys = c.get<R1csObj>(in.key_system, Kind::R1cs);
  R1csObj* csys = c.get<R1csObj>(in.circuit_system, Kind::R1cs);
  if (!A || !B1 || !B2 || !IC || !C || !H) return fail(GS_ERR_ARG, "%s: bad handle among the key's arrays (a, b1, ic, c, h: G1; b2: G2)", fn);
  if (!T1 || !T2 || !Ta || !Tb) return fail(GS_ERR_ARG, "%s: bad handle among the transcript's arrays (tau_g1, alpha_tau_g1, beta_tau_g1: G1; tau_g2: G2)", fn);
  if (!ksys || !csys) return fail(GS_ERR_ARG, "%s: bad R1CS handle", fn);
  uint64_t s[4];
  if (!challenge_words(in.challenge, s)) return fail(GS_ERR_ARG, "%s: the challenge is 0 mod r", fn);
  if (in.log2_domain < 1 || in.log2_domain > (uint64_t)kDomainMaxLog2) return fail(GS_ERR_ARG, "%s: log2_domain = %llu, must be 1 .. %d", fn, (unsigned long long)in.log2_domain, kDomainMaxLog2);
  const int k = (int)in.log2_domain;
  const size_t m = (size_t)1 << k, nvars = csys->m, npub = (size_t)in.npublic;
  if (!ksys->product || ksys->domain_log2 != k || ksys->m != nvars)
    return fail(GS_ERR_SHAPE, "%s: key_system must be a product system (gs_r1cs_upload_zkey) over 2^%d with the circuit's %zu variables", fn, k, nvars);
  if (csys->product || csys->domain_log2 != k)
    return fail(GS_ERR_SHAPE, "%s: circuit_system must be a domain R1CS with its C matrix (gs_r1cs_upload_domain) over 2^%d", fn, k);
  if (npub + 1 > nvars) return fail(GS_ERR_SHAPE, "%s: npublic + 1 = %zu exceeds the %zu variables", fn, npub + 1, nvars);
  if (A->n != nvars || B1->n != nvars || B2->n != nvars)
    return fail(GS_ERR_SHAPE, "%s: a, b1, b2 hold %zu, %zu, %zu points, the system has %zu variables", fn, A->n, B1->n, B2->n, nvars);
  if (IC->n != npub + 1) return fail(GS_ERR_SHAPE, "%s: ic holds %zu points, npublic + 1 = %zu", fn, IC->n, npub + 1);
  if (C->n != nvars - npub - 1) return fail(GS_ERR_SHAPE, "%s: c holds %zu points, nvars - npublic - 1 = %zu", fn, C->n, nvars - npub - 1);
  if (H->n != m) return fail(GS_ERR_SHAPE, "%s: h holds %zu points, the domain %zu", fn, H->n, m);
  if (T1->n < 2 * m - 1) return fail(GS_ERR_SHAPE, "%s: tau_g1 holds %zu points, the check needs 2m - 1 = %zu", fn, T1->n, 2 * m - 1);
  if (T2->n < m || Ta->n < m || Tb->n < m)
    return fail(GS_ERR_SHAPE, "%s: tau_g2, alpha_tau_g1, beta_tau_g1 hold %zu, %zu, %zu points, the check needs m = %zu", fn, T2->n, Ta->n, Tb->n, m);
  if (nvars > (size_t)kIndexMask || m > (size_t)kIndexMask) return fail(GS_ERR_ARG, "%s: at most 2^26 - 1 variables and domain points", fn);

  c.drain();
  reset_timing(c);
  for (Bases* b : {A, B1, B2, IC, C, H, T1, T2, Ta, Tb}) drop_table(b);
  // the value workspaces of the two systems are theirs to keep only if they had them before
  const bool had_ws[2] = {csys->vals.p != nullptr || csys->w_mont.p != nullptr, ksys->vals.p != nullptr || ksys->w_mont.p != nullptr};
  PhaseTimer total(c.stream);
  const size_t npow = std::max(nvars, m), cnt = T1->n >= 2 * m ? m : m - 1;
  const uint64_t two[4] = {2, 0, 0, 0};
  uint32_t differ[2] = {0, 0};
  // everything on the scalar side first: rho, its masks, the value vectors, the coefficient vectors, the twist
  DevBuf rho(npow * 32), pub(nvars * 32), prv(nvars * 32), coef_pub(3 * m * 32), coef_prv(3 * m * 32), coef_ab(2 * m * 32), hc(m * 32);
  {
    PhaseTimer tp(c.stream);
    scaled_powers_dev(c, s, s, npow, rho.as<uint32_t>());                                  // s^(i+1)
    hipLaunchKernelGGL(k_zc_masks, grid1(nvars), dim3(256), 0, c.stream, rho.as<uint32_t>(), (uint32_t)nvars, (uint32_t)npub, pub.as<uint32_t>(), prv.as<uint32_t>());
    GS_HIP(hipGetLastError());
    DevBuf cvals(2 * m * 32), dcount(8);
    GS_HIP(hipMemsetAsync(dcount.p, 0, 8, c.stream));
    // coefs A / coefs B: the circuit's rows and the key's own rows times rho
    r1cs_values_dev(c, *csys, rho.as<uint32_t>());
    GS_HIP(hipMemcpyAsync(cvals.p, csys->vals.p, 2 * m * 32, hipMemcpyDeviceToDevice, c.stream));
    r1cs_values_dev(c, *ksys, rho.as<uint32_t>());
    for (int v = 0; v < 2; ++v)
      hipLaunchKernelGGL(k_zc_differ, grid1(m), dim3(256), 0, c.stream, cvals.as<uint32_t>() + (size_t)v * m * 8, ksys->vals.as<uint32_t>() + (size_t)v * m * 8,
                         (uint32_t)m, dcount.as<uint32_t>() + v);
    GS_HIP(hipGetLastError());
    GS_HIP(hipMemcpyAsync(differ, dcount.p, 8, hipMemcpyDeviceToHost, c.stream));
    // p_A, p_B, p_C of rho^pub and rho^prv; those of rho are their sums
    r1cs_values_dev(c, *csys, pub.as<uint32_t>());
    domain_coeffs_dev(c, csys->vals.as<uint32_t>(), k, 3, coef_pub.as<uint32_t>());
    r1cs_values_dev(c, *csys, prv.as<uint32_t>());
    domain_coeffs_dev(c, csys->vals.as<uint32_t>(), k, 3, coef_prv.as<uint32_t>());
    poly_addsub_dev(c, coef_pub.as<uint32_t>(), 2 * m, coef_prv.as<uint32_t>(), 2 * m, false, coef_ab.as<uint32_t>());
    // c_t = (1/2) v^(-t) q_t: q from a copy of sigma (the transform works in place), times the powers of 1 / v scaled by 1 / 2
    DevBuf sig(m * 32), q(m * 32), tw(m * 32);
    GS_HIP(hipMemcpyAsync(sig.p, rho.p, m * 32, hipMemcpyDeviceToDevice, c.stream));
    domain_coeffs_dev(c, sig.as<uint32_t>(), k, 1, q.as<uint32_t>());
    uint64_t vinv[4], half[4];
    fr_words_from_mont(inv(dom_coset_gen(k)), vinv);
    fr_inv_words(two, half);
    scaled_powers_dev(c, vinv, half, m, tw.as<uint32_t>());
    hipLaunchKernelGGL(k_zc_twist, grid1(m), dim3(256), 0, c.stream, q.as<uint32_t>(), tw.as<uint32_t>(), (uint32_t)m, hc.as<uint32_t>());
    GS_HIP(hipGetLastError());
    tp.stop();
    GS_HIP(hipStreamSynchronize(c.stream));            // the scratch buffers go here
    c.timing.poly_ms += tp.ms();
  }
  const uint32_t* rho_w = rho.as<uint32_t>();
  // the key's side
  G1Xyzz lA, lB1, lIC, lC, lH;
  G2Xyzz lB2;
  {
    SharedPlan p(c, rho_w, nvars, 2, 1);
    auto g1 = p.sum<FqTag>({{A, 0}, {B1, 0}});
    lA = g1[0]; lB1 = g1[1];
    lB2 = p.sum<Fq2Tag>({{B2, 0}})[0];
  }
  { SharedPlan p(c, rho_w, npub + 1, 1, 0); lIC = p.sum<FqTag>({{IC, 0}})[0]; }
  { SharedPlan p(c, rho_w + (npub + 1) * 8, nvars - npub - 1, 1, 0); lC = p.sum<FqTag>({{C, 0}})[0]; }
  { SharedPlan p(c, rho_w, m, 1, 0); lH = p.sum<FqTag>({{H, 0}})[0]; }
  // the transcript's side
  G1Xyzz rA, rB1, rK[2], rH;
  G2Xyzz rB2;
  { SharedPlan p(c, coef_ab.as<uint32_t>(), m, 1, 0); rA = p.sum<FqTag>({{T1, 0}})[0]; }
  {
    SharedPlan p(c, coef_ab.as<uint32_t>() + m * 8, m, 1, 1);
    rB1 = p.sum<FqTag>({{T1, 0}})[0];
    rB2 = p.sum<Fq2Tag>({{T2, 0}})[0];
  }
  for (int half_ = 0; half_ < 2; ++half_) {
    const uint32_t* co = (half_ ? coef_prv : coef_pub).as<uint32_t>();
    Bases* over[3] = {Tb, Ta, T1};                                                          // beta p_A + alpha p_B + p_C
    rK[half_] = xyzz_inf<FqTag>();
    for (int v = 0; v < 3; ++v) {
      SharedPlan p(c, co + (size_t)v * m * 8, m, 1, 0);
      xyzz_add(rK[half_], p.sum<FqTag>({{over[v], 0}})[0]);
    }
  }
  if (cnt == m) {
    SharedPlan p(c, hc.as<uint32_t>(), m, 2, 0);
    auto g = p.sum<FqTag>({{T1, 0}, {T1, m}});
    rH = g[0];
    xyzz_add(rH, xyzz_neg(g[1]));
  } else {
    { SharedPlan p(c, hc.as<uint32_t>(), m, 1, 0); rH = p.sum<FqTag>({{T1, 0}})[0]; }
    SharedPlan p(c, hc.as<uint32_t>(), cnt, 1, 0);
    xyzz_add(rH, xyzz_neg(p.sum<FqTag>({{T1, m}})[0]));
  }
  total.stop();
  GS_HIP(hipStreamSynchronize(c.stream));
  c.timing.total_ms = total.ms();
  if (!had_ws[0]) { csys->w_mont.release(); csys->vals.release(); }
  if (!had_ws[1]) { ksys->w_mont.release(); ksys->vals.release(); }

  rep = gs_check_report{};
  rep.nchecks = 8;
  for (int v = 0; v < 2; ++v) {
    gs_check_result& r = rep.check[GS_KEY_COEFS_A + v];
    r.lhs[0] = differ[v];
    r.lhs_inf = r.rhs_inf = 1;
    r.ok = differ[v] == 0;
  }
  set_points(rep.check[GS_KEY_A], lA, rA);
  set_points(rep.check[GS_KEY_B1], lB1, rB1);
  set_points(rep.check[GS_KEY_B2], lB2, rB2);
  set_points(rep.check[GS_KEY_IC], lIC, rK[0]);
  set_points(rep.check[GS_KEY_C], lC, rK[1]);
  set_points(rep.check[GS_KEY_H], lH, rH);
  for (int i : {GS_KEY_A, GS_KEY_B1, GS_KEY_B2, GS_KEY_IC}) rep.check[i].ok = same_point(rep.check[i]);
  const G2Aff d2 = g2_from_jacobian_std(in.delta2), gen2 = pair_g2(kG2GenAffine, 0);
  const bool d2_ok = !d2.inf && g2_usable(d2);
  for (int i : {GS_KEY_C, GS_KEY_H}) {
    gs_check_result& r = rep.check[i];
    r.ok = d2_ok && pairings_equal(pair_g1(r.lhs, r.lhs_inf), d2, pair_g1(r.rhs, r.rhs_inf), gen2);
  }
  finish_report(rep);
  return GS_OK;
}

// ---- the transcript -----------------------------------------------------------------------------------------------------------------
template <class T>
void first_points(Ctx& c, Bases* b, size_t n, uint64_t* jac_std) {       // the first n points as Jacobian triples, standard form
  constexpr size_t cw = T::kWords;
  DevBuf tmp(n * 3 * cw * 4);
  if constexpr (T::kWords == 8) affine_to_jacobian_std_g1(c, b->buf.as<uint32_t>(), (uint32_t)n, tmp.as<uint32_t>());
  else affine_to_jacobian_std_g2(c, b->buf.as<uint32_t>(), (uint32_t)n, tmp.as<uint32_t>());
  GS_HIP(hipMemcpyAsync(jac_std, tmp.p, n * 3 * cw * 4, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
}
int ptau_check_impl(Ctx& c, gs_handle h1, gs_handle h2, gs_handle ha, gs_handle hb, const uint64_t beta_g2[24], size_t log2_n, const uint64_t challenge[4],
                    gs_check_report& rep) {
  const char* fn = "gs_ptau_check";
  Bases* T1 = c.get<Bases>(h1, Kind::G1Bases);
  Bases* T2 = c.get<Bases>(h2, Kind::G2Bases);
  Bases* Ta = c.get<Bases>(ha, Kind::G1Bases);
  Bases* Tb = c.get<Bases>(hb, Kind::G1Bases);
  if (!T1 || !T2 || !Ta || !Tb) return fail(GS_ERR_ARG, "%s: bad handle (tau_g1, alpha_tau_g1, beta_tau_g1: G1; tau_g2: G2)", fn);
  if (!beta_g2) return fail(GS_ERR_ARG, "%s: null argument", fn);
  uint64_t s[4];
  if (!challenge_words(challenge, s)) return fail(GS_ERR_ARG, "%s: the challenge is 0 mod r", fn);
  if (log2_n < 1 || log2_n > 25) return fail(GS_ERR_ARG, "%s: log2_n = %zu, must be 1 .. 25", fn, log2_n);
  const size_t N = (size_t)1 << log2_n, n1 = 2 * N - 2, n2 = N - 1;
  if (T1->n < 2 * N - 1) return fail(GS_ERR_SHAPE, "%s: tau_g1 holds %zu points, 2^%zu powers need 2N - 1 = %zu", fn, T1->n, log2_n, 2 * N - 1);
  if (T2->n < N || Ta->n < N || Tb->n < N)
    return fail(GS_ERR_SHAPE, "%s: tau_g2, alpha_tau_g1, beta_tau_g1 hold %zu, %zu, %zu points, 2^%zu powers need N = %zu", fn, T2->n, Ta->n, Tb->n, log2_n, N);
  c.drain();
  reset_timing(c);
  for (Bases* b : {T1, T2, Ta, Tb}) drop_table(b);
  PhaseTimer total(c.stream);
  DevBuf rho(n1 * 32);
  {
    PhaseTimer tp(c.stream);
    scaled_powers_dev(c, s, s, n1, rho.as<uint32_t>());
    tp.stop();
    c.timing.poly_ms += tp.ms();
  }
  std::vector<G1Xyzz> g1, ab;
  std::vector<G2Xyzz> g2;
  { SharedPlan p(c, rho.as<uint32_t>(), n1, 2, 0); g1 = p.sum<FqTag>({{T1, 0}, {T1, 1}}); }
  {
    SharedPlan p(c, rho.as<uint32_t>(), n2, 4, 2);
    ab = p.sum<FqTag>({{Ta, 0}, {Ta, 1}, {Tb, 0}, {Tb, 1}});
    g2 = p.sum<Fq2Tag>({{T2, 0}, {T2, 1}});
  }
  uint64_t t1w[24], t2w[48], bw[12];
  first_points<FqTag>(c, T1, 2, t1w);
  first_points<Fq2Tag>(c, T2, 2, t2w);
  first_points<FqTag>(c, Tb, 1, bw);
  total.stop();
  GS_HIP(hipStreamSynchronize(c.stream));
  c.timing.total_ms = total.ms();

  const G1Aff gen1 = pair_g1(kG1GenAffine, 0), tau1_0 = g1_from_jacobian_std(t1w), tau1_1 = g1_from_jacobian_std(t1w + 12), beta1 = g1_from_jacobian_std(bw);
  const G2Aff gen2 = pair_g2(kG2GenAffine, 0), tau2_0 = g2_from_jacobian_std(t2w), tau2_1 = g2_from_jacobian_std(t2w + 24), beta2 = g2_from_jacobian_std(beta_g2);
  rep = gs_check_report{};
  rep.nchecks = 8;
  set_points(rep.check[GS_PTAU_G1], tau1_0, gen1);
  set_points(rep.check[GS_PTAU_G2], tau2_0, gen2);
  rep.check[GS_PTAU_G1].ok = same_point(rep.check[GS_PTAU_G1]);
  rep.check[GS_PTAU_G2].ok = same_point(rep.check[GS_PTAU_G2]);
  set_points(rep.check[GS_PTAU_TAU], tau1_1, tau2_1);
  rep.check[GS_PTAU_TAU].ok = !tau1_1.inf && !tau2_1.inf && pairings_equal(tau1_1, gen2, gen1, tau2_1);
  auto g1_chain = [&](int which, const G1Xyzz& lhs, const G1Xyzz& rhs) {
    gs_check_result& r = rep.check[which];
    set_points(r, lhs, rhs);
    r.ok = !tau2_1.inf && pairings_equal(pair_g1(r.lhs, r.lhs_inf), tau2_1, pair_g1(r.rhs, r.rhs_inf), gen2);
  };
  g1_chain(GS_PTAU_TAU_G1, g1[0], g1[1]);
  g1_chain(GS_PTAU_ALPHA_TAU_G1, ab[0], ab[1]);
  g1_chain(GS_PTAU_BETA_TAU_G1, ab[2], ab[3]);
  {
    gs_check_result& r = rep.check[GS_PTAU_TAU_G2];
    set_points(r, g2[0], g2[1]);
    r.ok = !tau1_1.inf && pairings_equal(tau1_1, pair_g2(r.lhs, r.lhs_inf), gen1, pair_g2(r.rhs, r.rhs_inf));
  }
  set_points(rep.check[GS_PTAU_BETA_G2], beta1, beta2);
  rep.check[GS_PTAU_BETA_G2].ok = !beta1.inf && !beta2.inf && pairings_equal(beta1, gen2, gen1, beta2);
  finish_report(rep);
  return GS_OK;
}

// ---- the prepared sections of a transcript ------------------------------------------------------------------------------------------
// acc[i] += x[i] mod r, i < n (both standard form, any representative; the sum is < 2r)
__global__ void __launch_bounds__(256) k_zc_accumulate(uint32_t* __restrict__ acc, const uint32_t* __restrict__ x, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  zc_store(acc + (size_t)i * 8, canon(reduce2(add(zc_load(acc + (size_t)i * 8), zc_load(x + (size_t)i * 8)))));
}

constexpr int kLevelsCheckMaxLog2 = 25;      // 2^(hi+1) - 1 terms in one sum, and a sum takes at most 2^26 - 1 (kIndexMask)

// levels[2^p - 1 + j] = (1/2^p) sum_i w_p^(-ij) powers[i] for every p <= hi, as ONE equation of two sums: the coefficient of powers[i] in
// sum_p sum_j rho_(2^p-1+j) levels[2^p-1+j] is sum_p (1/2^p) sum_j rho_(2^p-1+j) w_p^(-ij) -- coefficient i of the interpolant of
// rho's slice for level p on that level's domain (domain_coeffs_dev: its 1/m is the 2^(-p)).
template <class T>
int levels_check_impl(Ctx& c, const char* fn, gs_handle hpow, gs_handle hlev, size_t hi_, const uint64_t challenge[4], gs_check_result& res) {
  constexpr Kind kind = T::kWords == 8 ? Kind::G1Bases : Kind::G2Bases;
  Bases* P = c.get<Bases>(hpow, kind);
  Bases* L = c.get<Bases>(hlev, kind);
  if (!P || !L) return fail(GS_ERR_ARG, "%s: bad base-array handle (powers, levels: both of this call's group)", fn);
  uint64_t s[4];
  if (!challenge_words(challenge, s)) return fail(GS_ERR_ARG, "%s: the challenge is 0 mod r", fn);
  if (hi_ > (size_t)kLevelsCheckMaxLog2)
    return fail(GS_ERR_ARG, "%s: hi = %zu, must be 0 .. %d (a sum takes at most 2^26 - 1 terms, the levels 0 .. hi are 2^(hi+1) - 1)", fn, hi_, kLevelsCheckMaxLog2);
  const int hi = (int)hi_;
  const size_t top = (size_t)1 << hi, nlev = 2 * top - 1;
  if (L->n < nlev) return fail(GS_ERR_SHAPE, "%s: levels holds %zu points, the levels 0 .. %d are %zu", fn, L->n, hi, nlev);
  if (P->n < top - 1)
    return fail(GS_ERR_SHAPE, "%s: powers holds %zu points, level %d needs %zu (or %zu and a last point at infinity)", fn, P->n, hi, top, top - 1);
  const size_t npow = std::min(P->n, top);
  c.drain();
  reset_timing(c);
  drop_table(P);
  drop_table(L);
  PhaseTimer total(c.stream);
  // rho lives from slot 1 of its buffer, so that level p's slice starts at slot 2^p: every transform runs on an aligned copy
  DevBuf rho(2 * top * 32), coef(top * 32);
  {
    PhaseTimer tp(c.stream);
    DevBuf vals(2 * top * 32), tmp(top * 32);
    GS_HIP(hipMemsetAsync(rho.p, 0, 32, c.stream));
    scaled_powers_dev(c, s, s, nlev, rho.as<uint32_t>() + 8);                              // s^(i+1)
    GS_HIP(hipMemcpyAsync(vals.p, rho.p, 2 * top * 32, hipMemcpyDeviceToDevice, c.stream));
    GS_HIP(hipMemsetAsync(coef.p, 0, top * 32, c.stream));
    for (int p = hi; p >= 0; --p) {                    // the largest first: the engine's twiddle table is made once
      const size_t m = (size_t)1 << p;
      domain_coeffs_dev(c, vals.as<uint32_t>() + m * 8, p, 1, tmp.as<uint32_t>());
      hipLaunchKernelGGL(k_zc_accumulate, grid1(m), dim3(256), 0, c.stream, coef.as<uint32_t>(), tmp.as<uint32_t>(), (uint32_t)m);
    }
    GS_HIP(hipGetLastError());
    tp.stop();
    GS_HIP(hipStreamSynchronize(c.stream));            // the scratch buffers go here
    c.timing.poly_ms += tp.ms();
  }
  Xyzz<T> lhs, rhs = xyzz_inf<T>();
  const int g1 = T::kWords == 8 ? 1 : 0;
  { SharedPlan p(c, rho.as<uint32_t>() + 8, nlev, g1, 1 - g1); lhs = p.sum<T>({{L, 0}})[0]; }
  if (npow) { SharedPlan p(c, coef.as<uint32_t>(), npow, g1, 1 - g1); rhs = p.sum<T>({{P, 0}})[0]; }
  total.stop();
  GS_HIP(hipStreamSynchronize(c.stream));
  c.timing.total_ms = total.ms();
  res = gs_check_result{};
  set_points(res, lhs, rhs);
  res.ok = same_point(res);
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_g1_lagrange_levels_check(gs_handle powers, gs_handle levels, size_t hi, const uint64_t challenge[4], gs_check_result* out) {
  return guarded([&](Ctx& c) -> int {
    if (!out || !challenge) return fail(GS_ERR_ARG, "gs_g1_lagrange_levels_check: null argument");
    return levels_check_impl<FqTag>(c, "gs_g1_lagrange_levels_check", powers, levels, hi, challenge, *out);
  }, true, false, powers);
}
int gs_g2_lagrange_levels_check(gs_handle powers, gs_handle levels, size_t hi, const uint64_t challenge[4], gs_check_result* out) {
  return guarded([&](Ctx& c) -> int {
    if (!out || !challenge) return fail(GS_ERR_ARG, "gs_g2_lagrange_levels_check: null argument");
    return levels_check_impl<Fq2Tag>(c, "gs_g2_lagrange_levels_check", powers, levels, hi, challenge, *out);
  }, true, false, powers);
}

int gs_groth16_key_check(const gs_key_check_input* in, gs_check_report* out) {
  return guarded([&](Ctx& c) -> int {
    if (!in || !out) return fail(GS_ERR_ARG, "gs_groth16_key_check: null argument");
    return key_check_impl(c, *in, *out);
  }, true, false, in ? in->a : 0);
}

int gs_ptau_check(gs_handle tau_g1, gs_handle tau_g2, gs_handle alpha_tau_g1, gs_handle beta_tau_g1, const uint64_t beta_g2[24], size_t log2_n,
                  const uint64_t challenge[4], gs_check_report* out) {
  return guarded([&](Ctx& c) -> int {
    if (!out || !challenge) return fail(GS_ERR_ARG, "gs_ptau_check: null argument");
    return ptau_check_impl(c, tau_g1, tau_g2, alpha_tau_g1, beta_tau_g1, beta_g2, log2_n, challenge, *out);
  }, true, false, tau_g1);
}

int gs_check_abi_sizes(size_t* input_bytes, size_t* report_bytes) {
  if (input_bytes) *input_bytes = sizeof(gs_key_check_input);
  if (report_bytes) *report_bytes = sizeof(gs_check_report);
  return GS_OK;
}

}  // extern "C"
