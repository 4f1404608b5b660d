// The quotient-basis array (prove.h, ProverKey::h_quot) of a key that was built elsewhere: nobody knows tau, the key has only its h
// array T, and  Q[m] = sum_{d <= m} g_d T[m - d]  (g = 1 / rev(Z)) is a convolution of a scalar series with a POINT sequence -- computed
// like any convolution, with the transform carried out in the group: T is zero-padded (points at infinity) to N = 2^ceil(log2(2 len_h - 1))
// XYZZ points, radix-2 stages whose butterflies are (P + Q, w (P - Q)) forwards and (P + w Q, P - w Q) backwards run over it in
// global memory (one butterfly is a 254-bit scalar multiplication, ~340 point operations: the stages are compute-bound), the spectrum
// is multiplied point by point with the spectrum of g (the polynomial engine's own transform of the divisor's series, 1 / N folded in),
// and the first len_h points of the result are normalised to affine.  The stages index exactly as ntt_forward / ntt_inverse_unscaled
// do (natural in, bit-reversed out, and back), so the two spectra meet without a permutation pass.  Every addition is the complete
// one: the padding is made of infinities, and a key may hold equal or opposite points.
// N / 2 * log2 N + N scalar multiplications -- seconds for a 2^20 key, once per key; explicit only (no policy derives the array).
// The same stages, run over many short blocks at once, carry the evaluation-basis array of such a key (ProverKey::h_eval) down a
// transposed subproduct tree: second half of this file, pk_derive_eval_impl.
#include <algorithm>

#include "domain.h"
#include "ec_stage.h"
#include "evaltree.h"
#include "point_io.h"
#include "prove.h"

using namespace gs;

namespace {

constexpr int kPw = PointIO<FqTag>::kXyzzWords;

// pts[i] = T[i] for i < n, the point at infinity for n <= i < total
__global__ void __launch_bounds__(256) k_ec_load(const uint32_t* __restrict__ affine, uint32_t n, uint32_t* __restrict__ pts, uint32_t total) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  G1Xyzz p = xyzz_inf<FqTag>();
  if (i < n) p = xyzz_from_affine(PointIO<FqTag>::load_affine(affine + (size_t)i * 16));
  store_xyzz<FqTag>(pts + (size_t)i * kPw, p);
}

// ---- the evaluation-basis array by a transposed subproduct tree in the group (pk_derive_eval_impl) ---------------------------------
// (k0 p, k1 p) with one window table: the two products of a spectrum point
GS_HD void xyzz_mul2_words_w4(const G1Xyzz& p, const uint32_t (&k0)[8], const uint32_t (&k1)[8], bool want0, bool want1, G1Xyzz& r0, G1Xyzz& r1) {
  G1Xyzz tab[16];
  tab[0] = xyzz_inf<FqTag>();
  tab[1] = p;
  for (int i = 2; i < 16; ++i) { tab[i] = tab[i - 1]; xyzz_add(tab[i], p); }
  r0 = xyzz_inf<FqTag>();
  r1 = xyzz_inf<FqTag>();
  for (int nib = 63; nib >= 0; --nib) {
    const int w = nib >> 3, sh = (nib & 7) * 4;
    if (want0) {
      for (int d = 0; d < 4; ++d) xyzz_dbl(r0);
      const uint32_t v = (k0[w] >> sh) & 15u;
      if (v) xyzz_add(r0, tab[v]);
    }
    if (want1) {
      for (int d = 0; d < 4; ++d) xyzz_dbl(r1);
      const uint32_t v = (k1[w] >> sh) & 15u;
      if (v) xyzz_add(r1, tab[v]);
    }
  }
}

// The point-wise step of one level: `src` holds the transformed sequences of the level's parents (slots of 2^level), `spec` the spectra
// of the children's reversed polynomials at that size (/ 2^level).  Spectrum point e of parent p is read once and written twice:
//   prod[slot of child 2p] = spec[slot of child 2p+1] * src,   prod[slot of child 2p+1] = spec[slot of child 2p] * src
// (each child in a slot of the parent's size).  A child without real leaves gets infinities and costs nothing.
__global__ void __launch_bounds__(64) k_ec_fork(const uint32_t* __restrict__ src, const uint32_t* __restrict__ spec, uint32_t* __restrict__ prod, uint32_t n, int level,
                                                uint32_t total) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const uint32_t p = e >> level, in = e & ((1u << level) - 1u);
  const size_t o0 = et_slot(level, et_child(p, 0)) + in, o1 = et_slot(level, et_child(p, 1)) + in;
  const G1Xyzz a = load_xyzz<FqTag>(src + (size_t)e * kPw);
  const bool want0 = !is_inf(a) && et_real(n, level - 1, et_child(p, 0)) != 0, want1 = !is_inf(a) && et_real(n, level - 1, et_child(p, 1)) != 0;
  G1Xyzz r0 = xyzz_inf<FqTag>(), r1 = r0;
  if (want0 || want1) {
    uint32_t k0[8], k1[8];
    load_words(spec + et_sibling_elem(level, o0) * 8, k0);
    load_words(spec + et_sibling_elem(level, o1) * 8, k1);
    xyzz_mul2_words_w4(a, k0, k1, want0, want1, r0, r1);
  }
  store_xyzz<FqTag>(prod + o0 * kPw, r0);
  store_xyzz<FqTag>(prod + o1 * kPw, r1);
}

// The windows of one level: child c of parent p takes elements [r_sibling, r_sibling + r_child) of its product (a slot of 2^level in
// `prod`) into its own slot of 2^(level-1) in `dst`; the rest of the slot is infinity.
__global__ void __launch_bounds__(256) k_ec_window(const uint32_t* __restrict__ prod, uint32_t* __restrict__ dst, uint32_t n, int level, uint32_t total) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const uint32_t child = i >> (level - 1), k = i & ((1u << (level - 1)) - 1u);
  G1Xyzz v = xyzz_inf<FqTag>();
  if (k < et_real(n, level - 1, child)) v = load_xyzz<FqTag>(prod + (et_slot(level, child) + et_window(n, level, child >> 1, (int)(child & 1u)) + k) * kPw);
  store_xyzz<FqTag>(dst + (size_t)i * kPw, v);
}

// The leaves: affine[j] = w[j] * pts[j], j < n  (w = 1 / M'(x_j), standard words)
__global__ void __launch_bounds__(64) k_ec_leaves(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ w, uint32_t n, uint32_t* __restrict__ affine) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  G1Xyzz p = load_xyzz<FqTag>(pts + (size_t)i * kPw);
  if (!is_inf(p)) {
    uint32_t k[8];
    load_words(w + (size_t)i * 8, k);
    p = xyzz_mul_words_w4(p, k);
  }
  PointIO<FqTag>::store_affine(affine + (size_t)i * 16, xyzz_to_affine(p));
}

int pk_derive_quot_impl(Ctx& c, const char* fn, Kind kind, gs_handle hpk) {
  ProverKey* pk = c.get<ProverKey>(hpk, kind);
  if (!pk) return fail(GS_ERR_ARG, "%s: bad proving-key handle", fn);
  if (pk->shard_count != 1) return fail(GS_ERR_ARG, "%s: the key is a slice (key slices carry no quotient-basis array)", fn);
  if (pk->coset_only) return refuse_coset_only(fn);
  const size_t n = pk->len_h;
  if (n == 0 || pk->nz == 0) return fail(GS_ERR_SHAPE, "%s: the key has no h array or no Z", fn);
  const int logn = ceil_log2(2 * n - 1);
  if (logn > ModR::kTwoAdicity) return fail(GS_ERR_ARG, "%s: key too large", fn);
  const size_t N = (size_t)1 << logn, half_n = std::max<size_t>(N / 2, 1);
  c.drain();
  // the scalar side, by the polynomial engine: spectrum of g (/ N, standard words) and the two twiddle tables
  divisor_ensure(c, pk->z, n);
  DevBuf gp(N * 32), spec(N * 32), twf(half_n * 32), twi(half_n * 32);
  GS_HIP(hipMemcpyAsync(gp.p, pk->z.inv_rev_mont.p, n * 32, hipMemcpyDeviceToDevice, c.stream));
  if (N > n) GS_HIP(hipMemsetAsync(gp.as<uint32_t>() + n * 8, 0, (N - n) * 32, c.stream));
  ntt_forward(c, gp.as<uint32_t>(), logn, logn);
  const uint64_t one[4] = {1, 0, 0, 0}, nn[4] = {(uint64_t)N, 0, 0, 0};
  uint64_t inv_n[4], w[4], wi[4];
  fr_inv_words(nn, inv_n);
  scale_mont_by_std_dev(c, gp.as<uint32_t>(), inv_n, N, spec.as<uint32_t>());
  ec_root_words(logn, false, w);
  ec_root_words(logn, true, wi);
  scaled_powers_dev(c, w, one, half_n, twf.as<uint32_t>());
  scaled_powers_dev(c, wi, one, half_n, twi.as<uint32_t>());
  // the group side
  DevBuf pts(N * kPw * 4);
  hipLaunchKernelGGL(k_ec_load, grid1(N), dim3(256), 0, c.stream, pk->h.pts.as<uint32_t>(), (uint32_t)n, pts.as<uint32_t>(), (uint32_t)N);
  const uint32_t nbf = (uint32_t)(N / 2);
  for (int s = 0; s < logn; ++s)                       // spans N/2, N/4, .., 1
    hipLaunchKernelGGL((k_ec_stage<FqTag, false>), grid1(nbf, 64), dim3(64), 0, c.stream, pts.as<uint32_t>(), nbf, (uint32_t)(N >> (s + 1)), 1u << s, twf.as<uint32_t>());
  hipLaunchKernelGGL(k_ec_scale<FqTag>, grid1(N, 64), dim3(64), 0, c.stream, pts.as<uint32_t>(), spec.as<uint32_t>(), (uint32_t)N);
  for (int s = logn - 1; s >= 0; --s)                  // spans 1, 2, .., N/2
    hipLaunchKernelGGL((k_ec_stage<FqTag, true>), grid1(nbf, 64), dim3(64), 0, c.stream, pts.as<uint32_t>(), nbf, (uint32_t)(N >> (s + 1)), 1u << s, twi.as<uint32_t>());
  GS_HIP(hipGetLastError());
  pk->h_quot.table.invalidate();
  pk->n_q = 0;
  pk->h_quot.pts.alloc(n * 64);
  hipLaunchKernelGGL(k_ec_to_affine<FqTag>, grid1(n), dim3(256), 0, c.stream, pts.as<uint32_t>(), (uint32_t)n, pk->h_quot.pts.as<uint32_t>());
  GS_HIP(hipGetLastError());
  GS_HIP(hipStreamSynchronize(c.stream));
  pk->n_q = n;
  return GS_OK;
}

// E[j-1] = sum_{i<n} coeff_i(l_j) h[i], l_j the Lagrange basis over the nodes x_j = n + j: the solution of the transposed Vandermonde
// system  sum_j E_j x_j^i = h[i], i < n,  by pushing h[0..n) down the node tree (evaltree.h).  A parent p with children L, R hands
//   c_L[k] = coefficient (r_R + k) of c_p rev(M_R), k < r_L,        c_R[k] = coefficient (r_L + k) of c_p rev(M_L), k < r_R
// down: middle products, which a cyclic convolution of the slot's length 2^level >= r_p gives exactly (the wrap-around lands below
// the window).  Per level: ONE batched forward transform of all parents, one fused point-wise step (k_ec_fork), one batched inverse
// transform of twice as many blocks, one window pass.  At a leaf c[0] = E_j M'(x_j).  The batched transforms are the last `level`
// stages of a transform of 2^L (forwards) and the first `level` of one of 2^(L+1) (backwards) with k_ec_stage as it is: its
// butterfly index already treats those stages as independent blocks.
// About 0.75 n log^2 n + 2 n log n scalar multiplications; explicit only, like the quotient-basis derivation.
int pk_derive_eval_impl(Ctx& c, const char* fn, Kind kind, gs_handle hpk, size_t n) {
  ProverKey* pk = c.get<ProverKey>(hpk, kind);
  if (!pk) return fail(GS_ERR_ARG, "%s: bad proving-key handle", fn);
  if (pk->shard_count != 1) return fail(GS_ERR_ARG, "%s: the key is a slice (derive the array on the full key, then cut it)", fn);
  if (pk->coset_only) return refuse_coset_only(fn);
  if (pk->len_h == 0 || pk->nz == 0) return fail(GS_ERR_SHAPE, "%s: the key has no h array or no Z", fn);
  if (n < 2 || n > pk->len_h || (pk->nz - 1 != n - 1 && pk->nz - 1 != n))
    return fail(GS_ERR_SHAPE, "%s: n = %zu, but deg Z = %zu needs n = deg Z or deg Z + 1 constraints (at least 2, at most the %zu points of the h array)", fn, n,
                pk->nz - 1, pk->len_h);
  const int L = ceil_log2(n);
  if (L + 1 > ModR::kTwoAdicity) return fail(GS_ERR_ARG, "%s: key too large", fn);
  const size_t total = (size_t)1 << L, half_n = std::max<size_t>(total / 2, 1);
  c.drain();
  // the scalar side, by the polynomial engine: the spectra of the reversed tree, 1 / M', the two twiddle tables of order 2^L
  std::vector<DevBuf> spec;
  DevBuf weights, twf(half_n * 32), twi(half_n * 32);
  shifted_tree_spectra_dev(c, n, spec, weights);
  const uint64_t one[4] = {1, 0, 0, 0};
  uint64_t w[4], wi[4];
  ec_root_words(L, false, w);
  ec_root_words(L, true, wi);
  scaled_powers_dev(c, w, one, half_n, twf.as<uint32_t>());
  scaled_powers_dev(c, wi, one, half_n, twi.as<uint32_t>());
  // the group side
  DevBuf cur(total * kPw * 4), prod(2 * total * kPw * 4);
  hipLaunchKernelGGL(k_ec_load, grid1(total), dim3(256), 0, c.stream, pk->h.pts.as<uint32_t>(), (uint32_t)n, cur.as<uint32_t>(), (uint32_t)total);
  const uint32_t nbf = (uint32_t)(total / 2);
  for (int level = L; level >= 1; --level) {
    const size_t blk = (size_t)1 << level;
    for (size_t half = blk / 2; half >= 1; half >>= 1)         // spans 2^(level-1) .. 1 within every slot
      hipLaunchKernelGGL((k_ec_stage<FqTag, false>), grid1(nbf, 64), dim3(64), 0, c.stream, cur.as<uint32_t>(), nbf, (uint32_t)half, (uint32_t)(total / (2 * half)), twf.as<uint32_t>());
    hipLaunchKernelGGL(k_ec_fork, grid1(total, 64), dim3(64), 0, c.stream, cur.as<uint32_t>(), spec[level - 1].as<uint32_t>(), prod.as<uint32_t>(), (uint32_t)n, level,
                       (uint32_t)total);
    for (size_t half = 1; half <= blk / 2; half <<= 1)         // spans 1 .. 2^(level-1), twice as many slots
      hipLaunchKernelGGL((k_ec_stage<FqTag, true>), grid1(2 * nbf, 64), dim3(64), 0, c.stream, prod.as<uint32_t>(), 2 * nbf, (uint32_t)half, (uint32_t)(total / (2 * half)),
                         twi.as<uint32_t>());
    hipLaunchKernelGGL(k_ec_window, grid1(total), dim3(256), 0, c.stream, prod.as<uint32_t>(), cur.as<uint32_t>(), (uint32_t)n, level, (uint32_t)total);
  }
  GS_HIP(hipGetLastError());
  pk->h_eval.table.invalidate();
  pk->n_eval = 0; pk->e_lo = 0; pk->n_e = 0;
  pk->h_eval.pts.alloc(n * 64);
  hipLaunchKernelGGL(k_ec_leaves, grid1(n, 64), dim3(64), 0, c.stream, cur.as<uint32_t>(), weights.as<uint32_t>(), (uint32_t)n, pk->h_eval.pts.as<uint32_t>());
  GS_HIP(hipGetLastError());
  GS_HIP(hipStreamSynchronize(c.stream));
  pk->n_eval = n; pk->n_e = n; pk->eval_domain_log2 = 0;
  return GS_OK;
}

// The coset evaluation-basis array of a key over the power-of-two domain 2^k (domain.h), from its h array T alone:
//   E_j = -(1/(2m)) sum_{i<m} (g omega^j)^(-i) T_i = sum_i omega^(-ij) [(-(1/(2m)) g^(-i)) T_i]:
// ONE transform of size m in the group with the root omega^(-1).  Term i is loaded into slot bitrev(i) and multiplied by its scalar,
// then the decimation-in-time stages leave E in natural order: m + m/2 * k scalar multiplications, every addition the complete one
// (T may hold infinities, equal and opposite points).  A key with only m - 1 points in T takes T[m-1] as infinity.
int pk_derive_eval_domain_impl(Ctx& c, gs_handle hpk, size_t log2_domain) {
  const char* fn = "gs_groth16_pk_derive_eval_domain";
  GrothPkObj* pk = c.get<GrothPkObj>(hpk, Kind::GrothPk);
  if (!pk) return fail(GS_ERR_ARG, "%s: bad proving-key handle", fn);
  if (pk->shard_count != 1) return fail(GS_ERR_ARG, "%s: the key is a slice", fn);
  if (pk->coset_only) return refuse_coset_only(fn);
  if (log2_domain < 1 || pk->domain_log2 == 0 || (size_t)pk->domain_log2 != log2_domain)
    return fail(GS_ERR_SHAPE, "%s: the key's Z (%zu coefficients) is not x^(2^%zu) - 1", fn, pk->nz, log2_domain);
  const int k = (int)log2_domain;
  const size_t m = (size_t)1 << k, half_m = m / 2;
  if (pk->len_h + 1 < m) return fail(GS_ERR_SHAPE, "%s: the key's h array has %zu points, the domain needs %zu", fn, pk->len_h, m - 1);
  c.drain();
  DevBuf scal(m * 32), twi(half_m * 32), pts(m * kPw * 4);
  const uint64_t one[4] = {1, 0, 0, 0};
  uint64_t wi[4];
  ec_root_words(k, true, wi);
  domain_derive_scalars_dev(c, k, scal.as<uint32_t>());
  scaled_powers_dev(c, wi, one, half_m, twi.as<uint32_t>());
  hipLaunchKernelGGL(k_ec_load_bitrev<FqTag>, grid1(m), dim3(256), 0, c.stream, pk->h.pts.as<uint32_t>(), (uint32_t)std::min(pk->len_h, m), pts.as<uint32_t>(), k);
  hipLaunchKernelGGL(k_ec_scale<FqTag>, grid1(m, 64), dim3(64), 0, c.stream, pts.as<uint32_t>(), scal.as<uint32_t>(), (uint32_t)m);
  const uint32_t nbf = (uint32_t)half_m;
  for (int s = k - 1; s >= 0; --s)                     // spans 1, 2, .., m/2
    hipLaunchKernelGGL((k_ec_stage<FqTag, true>), grid1(nbf, 64), dim3(64), 0, c.stream, pts.as<uint32_t>(), nbf, (uint32_t)(m >> (s + 1)), 1u << s, twi.as<uint32_t>());
  GS_HIP(hipGetLastError());
  pk->h_eval.table.invalidate();
  pk->n_eval = 0; pk->e_lo = 0; pk->n_e = 0;
  pk->h_eval.pts.alloc(m * 64);
  hipLaunchKernelGGL(k_ec_to_affine<FqTag>, grid1(m), dim3(256), 0, c.stream, pts.as<uint32_t>(), (uint32_t)m, pk->h_eval.pts.as<uint32_t>());
  GS_HIP(hipGetLastError());
  GS_HIP(hipStreamSynchronize(c.stream));
  pk->n_eval = m; pk->n_e = m; pk->eval_domain_log2 = k;
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_groth16_pk_derive_quot(gs_handle hpk) {
  return guarded([&](Ctx& c) -> int { return pk_derive_quot_impl(c, "gs_groth16_pk_derive_quot", Kind::GrothPk, hpk); }, true, false, hpk);
}
int gs_pinocchio_pk_derive_quot(gs_handle hpk) {
  return guarded([&](Ctx& c) -> int { return pk_derive_quot_impl(c, "gs_pinocchio_pk_derive_quot", Kind::PinocchioPk, hpk); }, true, false, hpk);
}
int gs_groth16_pk_derive_eval(gs_handle hpk, size_t n_constraints) {
  return guarded([&](Ctx& c) -> int { return pk_derive_eval_impl(c, "gs_groth16_pk_derive_eval", Kind::GrothPk, hpk, n_constraints); }, true, false, hpk);
}
int gs_groth16_pk_derive_eval_domain(gs_handle hpk, size_t log2_domain) {
  return guarded([&](Ctx& c) -> int { return pk_derive_eval_domain_impl(c, hpk, log2_domain); }, true, false, hpk);
}
int gs_pinocchio_pk_derive_eval(gs_handle hpk, size_t n_constraints) {
  return guarded([&](Ctx& c) -> int { return pk_derive_eval_impl(c, "gs_pinocchio_pk_derive_eval", Kind::PinocchioPk, hpk, n_constraints); }, true, false, hpk);
}

}  // extern "C"
