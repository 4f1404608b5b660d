// Building proving keys: full keys, coset-only keys and key slices of both schemes, from base arrays on the device (the arrays are
// copied, so a key owns what it sums over), and the once-per-key scans that go with it.  The prover engine that reads the keys is
// prove.hip; what a key is, prove.h.
#include "prove.h"

#include <algorithm>
#include <vector>

#include "domain.h"
#include "point_io.h"

using namespace gs;

namespace {

constexpr size_t kG1Aff = 16, kG2Aff = 32;      // u32 words per packed affine point

// copy n packed points [off, off+n) of a base handle into an owned buffer
void copy_points(Ctx& c, const Bases* b, size_t words, DevBuf& dst) {
  dst.alloc(std::max<size_t>(b->n, 1) * words * 4);
  if (b->n) GS_HIP(hipMemcpyAsync(dst.p, b->buf.p, b->n * words * 4, hipMemcpyDeviceToDevice, c.stream));
}

// the list of the variables with a finite point in either array: the device scans (one bit per variable), the host turns the bits
// into the ascending index list and uploads it
static size_t scan_finite_terms(Ctx& c, const uint32_t* g1_pts, const uint32_t* g2_pts, size_t n, DevBuf& index_dev, std::vector<uint32_t>& index_host) {
  index_host.clear();
  index_dev.release();
  if (n == 0) return 0;
  const size_t words = (n + 31) / 32;
  DevBuf mask(words * 4);
  const size_t finite = finite_mask_dev(c, g1_pts, g2_pts, (uint32_t)n, mask.as<uint32_t>());
  if (finite == n) return finite;                        // nothing missing: no list, no second plan
  std::vector<uint32_t> bits(words);
  GS_HIP(hipMemcpyAsync(bits.data(), mask.p, words * 4, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
  index_host.reserve(finite);
  for (size_t wd = 0; wd < words; ++wd)
    for (uint32_t m = bits[wd]; m; m &= m - 1) index_host.push_back((uint32_t)(wd * 32 + (size_t)__builtin_ctz(m)));
  index_dev.alloc(std::max<size_t>(index_host.size(), 1) * 4);
  if (!index_host.empty()) {
    GS_HIP(hipMemcpyAsync(index_dev.p, index_host.data(), index_host.size() * 4, hipMemcpyHostToDevice, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
  }
  return finite;
}

// Shared builder of full keys and key slices: copies [lo, lo + n) of each source array (device, packed affine).
struct PkSrc { const DevBuf* buf; size_t lo; };
// `from`: the context the source arrays live on (another GPU for gs_*_pk_shard_to)
static void copy_slice(Ctx& c, Ctx& from, const PkSrc& s, size_t n, size_t words, DevBuf& dst) {
  dst.alloc(std::max<size_t>(n, 1) * words * 4);
  copy_between(c, dst.p, from, static_cast<const char*>(s.buf->p) + s.lo * words * 4, n * words * 4);
}
// groth16.go:177-180 / :248: the C sum runs over i > NPublic; global entries [0, NPublic] of BACDelta become infinity
static void groth_force_public(Ctx& c, GrothPkObj& pk) {
  const size_t zero_hi = std::min(pk.npublic + 1, pk.w_lo + pk.n_w);
  if (zero_hi > pk.w_lo) force_infinity(c, pk.bacdelta(), zero_hi - pk.w_lo, kG1Aff);
}
static void set_shard(ProverKey& pk, size_t index, size_t count) {
  Shard sh; sh.index = index; sh.count = count;
  size_t lo, hi;
  pk.shard_index = index; pk.shard_count = count;
  shard_range(pk.nvars, sh, lo, hi);
  pk.w_lo = lo; pk.n_w = hi - lo;
  shard_range(pk.len_h, sh, lo, hi);
  pk.h_lo = lo; pk.n_h = hi - lo;
}
// what a slice takes over from the full key beside the arrays
static void shard_extras(Ctx& c, GrothPkObj& pk, const GrothPkObj& full) {
  groth_force_public(c, pk);
  pk.alpha = full.alpha; pk.beta = full.beta; pk.delta = full.delta; pk.beta2 = full.beta2; pk.delta2 = full.delta2;
}
// (A / Ap of the full key already hold infinity for i <= NPublic, snark.go:265: the slices inherit it)
static void shard_extras(Ctx&, PinocchioPkObj&, const PinocchioPkObj&) {}

// A slice of a resident full key (device-to-device copies): what each rank keeps when the full key was built or loaded
// locally; the caller then frees the full key.  `c` is the context the slice is created on -- the key's own, or another
// logical device's (gs_*_pk_shard_to: the copies then cross xGMI, or stay on the GPU when both share one).
template <class Pk>
static int pk_shard_impl(Ctx& c, Ctx& from, const char* scheme, Pk* full, size_t shard_index, size_t shard_count, gs_handle* out) {
  if (!full || !out) return fail(GS_ERR_ARG, "gs_%s_pk_shard: bad proving-key handle or null output", scheme);
  if (full->shard_count != 1) return fail(GS_ERR_ARG, "gs_%s_pk_shard: the source key is itself a slice", scheme);
  if (full->coset_only) return refuse_coset_only("gs_groth16_pk_shard");
  if (shard_count == 0 || shard_index >= shard_count) return fail(GS_ERR_ARG, "gs_%s_pk_shard: bad shard %zu of %zu", scheme, shard_index, shard_count);
  auto pk = std::make_unique<Pk>();
  pk->nvars = full->nvars; pk->npublic = full->npublic; pk->nz = full->nz; pk->len_h = full->len_h;
  set_shard(*pk, shard_index, shard_count);
  for (int i = 0; i < pk->n_g1w; ++i) copy_slice(c, from, PkSrc{&full->g1w[i].pts, pk->w_lo}, pk->n_w, kG1Aff, pk->g1w[i].pts);
  copy_slice(c, from, PkSrc{&full->h.pts, pk->h_lo}, pk->n_h, kG1Aff, pk->h.pts);
  copy_slice(c, from, PkSrc{&full->g2w.pts, pk->w_lo}, pk->n_w, kG2Aff, pk->g2w.pts);
  if (full->n_eval && !full->eval_domain_log2) {        // the evaluation-basis array is cut like the other term ranges (its own split of [0, n)); a coset basis (domain.h) stays behind
    Shard sh; sh.index = shard_index; sh.count = shard_count;
    size_t lo, hi;
    shard_range(full->n_eval, sh, lo, hi);
    pk->n_eval = full->n_eval; pk->e_lo = lo; pk->n_e = hi - lo;
    copy_slice(c, from, PkSrc{&full->h_eval.pts, lo}, pk->n_e, kG1Aff, pk->h_eval.pts);
  }
  shard_extras(c, *pk, *full);
  {                                                     // Z travels with every slice
    DevBuf zc(std::max<size_t>(full->nz, 1) * 32);
    copy_between(c, zc.p, from, full->z.b_std.p, full->nz * 32);
    divisor_init(c, pk->z, zc.as<uint32_t>(), full->nz);
    GS_HIP(hipStreamSynchronize(c.stream));             // `zc` is released here
  }
  GS_HIP(hipStreamSynchronize(c.stream));
  pk_scan_sparsity(c, *pk);
  *out = c.put(std::move(pk));
  return GS_OK;
}

}  // namespace

bool gs::bad_shard(size_t shard_index, size_t shard_count) { return shard_count == 0 || shard_index >= shard_count; }
void gs::force_infinity(Ctx& c, DevBuf& pts, size_t count, size_t words) {
  if (count) GS_HIP(hipMemsetAsync(pts.p, 0, count * words * 4, c.stream));
}
void gs::pk_scan_sparsity(Ctx& c, ProverKey& pk) {
  pk.b_finite = scan_finite_terms(c, pk.g1w[pk.b_g1].pts.as<uint32_t>(), pk.g2w.pts.as<uint32_t>(), pk.n_w, pk.b_index, pk.b_index_host);
}

extern "C" {

// ---- Groth16 ----------------------------------------------------------------------------------------------
// k >= 1 when Z (nz coefficients, any representatives mod r) is exactly x^m - 1 with m = 2^k <= 2^27, else 0: the keys of a QAP over a
// power-of-two domain (domain.h).  Host work, once per key.
static int z_domain_log2(const uint64_t* z, size_t nz) {
  if (nz < 3 || ((nz - 1) & (nz - 2)) != 0 || nz - 1 > ((size_t)1 << kDomainMaxLog2)) return 0;
  const size_t m = nz - 1;
  const uint64_t zero[4] = {0, 0, 0, 0}, one[4] = {1, 0, 0, 0};
  uint64_t d[4];
  fr_sub_words(z + 4 * m, one, d);
  if (!fr_is_zero_words(d)) return 0;
  fr_sub_words(zero, z, d);                              // -z[0] - 1
  fr_sub_words(d, one, d);
  if (!fr_is_zero_words(d)) return 0;
  for (size_t i = 1; i < m; ++i) {
    const uint64_t* v = z + 4 * i;
    if ((v[0] | v[1] | v[2] | v[3]) != 0 && !fr_is_zero_words(v)) return 0;
  }
  return ceil_log2(m);
}
// What gs_groth16_pk_create[_shard] and gs_groth16_pk_create_domain take alike: the four arrays over w, the array of the h side
// (PowersTauDelta, or the coset evaluation basis) and five points (Jacobian, standard form).
struct GrothKeyArgs {
  gs_handle g1_at, g1_bacgamma, g2_bacgamma, bacdelta, h_side;
  const uint64_t *g1_alpha, *g1_beta, *g1_delta, *g2_beta, *g2_delta;
  bool null_point() const { return !g1_alpha || !g1_beta || !g1_delta || !g2_beta || !g2_delta; }
};
struct GrothKeyBases {
  Bases *at, *b1, *b2, *cd, *h;
  GrothKeyBases(Ctx& c, const GrothKeyArgs& a)
      : at(c.get<Bases>(a.g1_at, Kind::G1Bases)), b1(c.get<Bases>(a.g1_bacgamma, Kind::G1Bases)), b2(c.get<Bases>(a.g2_bacgamma, Kind::G2Bases)),
        cd(c.get<Bases>(a.bacdelta, Kind::G1Bases)), h(c.get<Bases>(a.h_side, Kind::G1Bases)) {}
  bool ok() const { return at && b1 && b2 && cd && h; }
  bool all_over_w(size_t n) const { return at->n == n && b1->n == n && b2->n == n && cd->n == n; }
};
// five arrays in (the h-side array into `h_dst`), the public entries of BACDelta forced to infinity, five host points converted
static void groth_fill(Ctx& c, GrothPkObj& pk, const GrothKeyBases& b, DevBuf& h_dst, const GrothKeyArgs& a) {
  copy_points(c, b.at, kG1Aff, pk.at());
  copy_points(c, b.b1, kG1Aff, pk.bacgamma1());
  copy_points(c, b.cd, kG1Aff, pk.bacdelta());
  copy_points(c, b.b2, kG2Aff, pk.bacgamma2());
  copy_points(c, b.h, kG1Aff, h_dst);
  groth_force_public(c, pk);
  pk.alpha = g1_affine_from_jacobian_std(a.g1_alpha);
  pk.beta = g1_affine_from_jacobian_std(a.g1_beta);
  pk.delta = g1_affine_from_jacobian_std(a.g1_delta);
  pk.beta2 = g2_affine_from_jacobian_std(a.g2_beta);
  pk.delta2 = g2_affine_from_jacobian_std(a.g2_delta);
}

static int groth_pk_create_impl(Ctx& c, const GrothKeyArgs& a, const uint64_t* z, size_t nz, size_t nvars, size_t npublic, size_t nptd_total,
                                size_t shard_index, size_t shard_count, gs_handle* out) {
  const GrothKeyBases b(c, a);
  if (!b.ok()) return fail(GS_ERR_ARG, "gs_groth16_pk_create: bad base handle");
  if (a.null_point() || !z || !out || nz == 0) return fail(GS_ERR_ARG, "null argument");
  if (bad_shard(shard_index, shard_count)) return fail(GS_ERR_ARG, "gs_groth16_pk_create_shard: bad shard %zu of %zu", shard_index, shard_count);
  if (npublic + 1 > nvars) return fail(GS_ERR_SHAPE, "NPublic + 1 > NVars");
  bool lead_zero = true;
  for (int i = 0; i < 4; ++i) lead_zero = lead_zero && z[4 * (nz - 1) + i] == 0;
  if (lead_zero) return fail(GS_ERR_ARG, "leading coefficient of Z is zero");
  auto pk = std::make_unique<GrothPkObj>();
  pk->nvars = nvars; pk->npublic = npublic; pk->nz = nz; pk->len_h = shard_count == 1 ? b.h->n : nptd_total;
  set_shard(*pk, shard_index, shard_count);
  if (!b.all_over_w(pk->n_w))
    return fail(GS_ERR_SHAPE, "At/BACGamma/BACDelta must have %zu points (NVars = %zu, shard %zu of %zu), got %zu/%zu/%zu/%zu", pk->n_w, nvars,
                shard_index, shard_count, b.at->n, b.b1->n, b.b2->n, b.cd->n);
  if (b.h->n != pk->n_h)
    return fail(GS_ERR_SHAPE, "PowersTauDelta must have %zu points (total %zu, shard %zu of %zu), got %zu", pk->n_h, pk->len_h, shard_index, shard_count, b.h->n);
  groth_fill(c, *pk, b, pk->ptd(), a);
  if (shard_count == 1) pk->domain_log2 = z_domain_log2(z, nz);
  const uint32_t* dz = upload_tmp(c, prove_state(c).up_a, z, nz);
  divisor_init(c, pk->z, dz, nz);
  GS_HIP(hipStreamSynchronize(c.stream));
  pk_scan_sparsity(c, *pk);
  *out = c.put(std::move(pk));
  return GS_OK;
}

int gs_groth16_pk_create(gs_handle g1_at, gs_handle g1_bacgamma, gs_handle g2_bacgamma, gs_handle bacdelta, gs_handle ptd,
                         const uint64_t g1_alpha[12], const uint64_t g1_beta[12], const uint64_t g1_delta[12],
                         const uint64_t g2_beta[24], const uint64_t g2_delta[24], const uint64_t* z, size_t nz,
                         size_t nvars, size_t npublic, gs_handle* out) {
  return guarded([&](Ctx& c) -> int {
    const GrothKeyArgs a{g1_at, g1_bacgamma, g2_bacgamma, bacdelta, ptd, g1_alpha, g1_beta, g1_delta, g2_beta, g2_delta};
    return groth_pk_create_impl(c, a, z, nz, nvars, npublic, 0, 0, 1, out);
  }, true, false, g1_at);
}

int gs_groth16_pk_create_shard(gs_handle g1_at, gs_handle g1_bacgamma, gs_handle g2_bacgamma, gs_handle bacdelta, gs_handle ptd,
                               const uint64_t g1_alpha[12], const uint64_t g1_beta[12], const uint64_t g1_delta[12],
                               const uint64_t g2_beta[24], const uint64_t g2_delta[24], const uint64_t* z, size_t nz,
                               size_t nvars, size_t npublic, size_t nptd_total, size_t shard_index, size_t shard_count, gs_handle* out) {
  return guarded([&](Ctx& c) -> int {
    const GrothKeyArgs a{g1_at, g1_bacgamma, g2_bacgamma, bacdelta, ptd, g1_alpha, g1_beta, g1_delta, g2_beta, g2_delta};
    return groth_pk_create_impl(c, a, z, nz, nvars, npublic, nptd_total, shard_index, shard_count, out);
  }, true, false, g1_at);
}

// A coset-only key (prove.h): the five arrays and five points of gs_groth16_pk_create, but in place of PowersTauDelta the m = 2^log2_domain
// points of the coset evaluation basis E (domain.h) -- section 9 of a snarkjs .zkey.  Z = x^m - 1 is built here.
int gs_groth16_pk_create_domain(gs_handle g1_at, gs_handle g1_bacgamma, gs_handle g2_bacgamma, gs_handle bacdelta, gs_handle h_coset,
                                const uint64_t g1_alpha[12], const uint64_t g1_beta[12], const uint64_t g1_delta[12],
                                const uint64_t g2_beta[24], const uint64_t g2_delta[24], size_t log2_domain, size_t nvars, size_t npublic, gs_handle* out) {
  return guarded([&](Ctx& c) -> int {
    const char* fn = "gs_groth16_pk_create_domain";
    const GrothKeyArgs a{g1_at, g1_bacgamma, g2_bacgamma, bacdelta, h_coset, g1_alpha, g1_beta, g1_delta, g2_beta, g2_delta};
    const GrothKeyBases b(c, a);
    if (!b.ok()) return fail(GS_ERR_ARG, "%s: bad base handle", fn);
    if (a.null_point() || !out) return fail(GS_ERR_ARG, "%s: null argument", fn);
    if (log2_domain < 1 || log2_domain > (size_t)kDomainMaxLog2) return fail(GS_ERR_ARG, "%s: log2_domain = %zu, must be 1 .. %d", fn, log2_domain, kDomainMaxLog2);
    if (npublic + 1 > nvars) return fail(GS_ERR_SHAPE, "NPublic + 1 > NVars");
    const size_t m = (size_t)1 << log2_domain, nz = m + 1;
    if (!b.all_over_w(nvars))
      return fail(GS_ERR_SHAPE, "%s: At/BACGamma/BACDelta must have NVars = %zu points, got %zu/%zu/%zu/%zu", fn, nvars, b.at->n, b.b1->n, b.b2->n, b.cd->n);
    if (b.h->n != m) return fail(GS_ERR_SHAPE, "%s: the coset evaluation basis must have 2^%zu = %zu points, got %zu", fn, log2_domain, m, b.h->n);
    auto pk = std::make_unique<GrothPkObj>();
    pk->nvars = nvars; pk->npublic = npublic; pk->nz = nz; pk->len_h = 0;
    set_shard(*pk, 0, 1);                                  // a full key: n_w = nvars, n_h = 0
    pk->coset_only = true;
    groth_fill(c, *pk, b, pk->ptd_eval(), a);
    pk->domain_log2 = (int)log2_domain;
    pk->n_eval = m; pk->e_lo = 0; pk->n_e = m; pk->eval_domain_log2 = (int)log2_domain;
    {                                                      // Z = x^m - 1, standard form: r - 1, zeros, 1
      uint32_t lo[8], hi[8] = {1u, 0, 0, 0, 0, 0, 0, 0};
      for (int i = 0; i < 8; ++i) lo[i] = ModR::p32(i);
      lo[0] -= 1u;                                         // r is odd: no borrow
      DevBuf zc(nz * 32);
      GS_HIP(hipMemsetAsync(zc.p, 0, nz * 32, c.stream));
      GS_HIP(hipMemcpyAsync(zc.p, lo, 32, hipMemcpyHostToDevice, c.stream));
      GS_HIP(hipMemcpyAsync(zc.as<uint32_t>() + m * 8, hi, 32, hipMemcpyHostToDevice, c.stream));
      divisor_init(c, pk->z, zc.as<uint32_t>(), nz);
      GS_HIP(hipStreamSynchronize(c.stream));              // `zc` is released here
    }
    pk_scan_sparsity(c, *pk);
    *out = c.put(std::move(pk));
    return GS_OK;
  }, true, false, g1_at);
}

int gs_groth16_pk_shard(gs_handle hfull, size_t shard_index, size_t shard_count, gs_handle* out) {
  return guarded([&](Ctx& c) -> int {
    return pk_shard_impl(c, c, "groth16", c.get<GrothPkObj>(hfull, Kind::GrothPk), shard_index, shard_count, out);
  }, true, false, hfull);
}

int gs_groth16_pk_shard_to(gs_handle hfull, size_t shard_index, size_t shard_count, int target_device, gs_handle* out) {
  return guarded_pair(hfull, target_device, [&](Ctx& src, Ctx& dst) -> int {
    return pk_shard_impl(dst, src, "groth16", src.get<GrothPkObj>(hfull, Kind::GrothPk), shard_index, shard_count, out);
  });
}

// ---- Pinocchio ----------------------------------------------------------------------------------------------
int gs_pinocchio_pk_create(gs_handle a, gs_handle ap, gs_handle b_g2, gs_handle bp, gs_handle cc, gs_handle cp, gs_handle kp,
                           gs_handle g1t, const uint64_t* z, size_t nz, size_t nvars, size_t npublic, gs_handle* out) {
  return guarded([&](Ctx& c) -> int {
    Bases* A = c.get<Bases>(a, Kind::G1Bases);
    Bases* Ap = c.get<Bases>(ap, Kind::G1Bases);
    Bases* B = c.get<Bases>(b_g2, Kind::G2Bases);
    Bases* Bp = c.get<Bases>(bp, Kind::G1Bases);
    Bases* C = c.get<Bases>(cc, Kind::G1Bases);
    Bases* Cp = c.get<Bases>(cp, Kind::G1Bases);
    Bases* Kp = c.get<Bases>(kp, Kind::G1Bases);
    Bases* T = c.get<Bases>(g1t, Kind::G1Bases);
    if (!A || !Ap || !B || !Bp || !C || !Cp || !Kp || !T) return fail(GS_ERR_ARG, "gs_pinocchio_pk_create: bad base handle");
    if (!z || !out || nz == 0) return fail(GS_ERR_ARG, "null argument");
    for (Bases* x : {A, Ap, B, Bp, C, Cp, Kp})
      if (x->n != nvars) return fail(GS_ERR_SHAPE, "every per-variable key array must have NVars = %zu points (got %zu)", nvars, x->n);
    if (npublic + 1 > nvars) return fail(GS_ERR_SHAPE, "NPublic + 1 > NVars");
    auto pk = std::make_unique<PinocchioPkObj>();
    pk->nvars = nvars; pk->npublic = npublic; pk->nz = nz; pk->len_h = T->n;
    pk->n_w = nvars; pk->n_h = T->n;                                // a full key
    const Bases* g1src[6] = {A, Ap, Bp, C, Cp, Kp};                 // the order of PinocchioPkObj's g1w
    for (int i = 0; i < 6; ++i) copy_points(c, g1src[i], kG1Aff, pk->g1w[i].pts);
    copy_points(c, T, kG1Aff, pk->g1t());
    copy_points(c, B, kG2Aff, pk->b2());
    force_infinity(c, pk->a(), npublic + 1, kG1Aff);                 // snark.go:265
    force_infinity(c, pk->ap(), npublic + 1, kG1Aff);
    const uint32_t* dz = upload_tmp(c, prove_state(c).up_a, z, nz);
    divisor_init(c, pk->z, dz, nz);
    GS_HIP(hipStreamSynchronize(c.stream));
    pk_scan_sparsity(c, *pk);
    *out = c.put(std::move(pk));
    return GS_OK;
  }, true, false, a);
}

int gs_pinocchio_pk_shard(gs_handle hfull, size_t shard_index, size_t shard_count, gs_handle* out) {
  return guarded([&](Ctx& c) -> int {
    return pk_shard_impl(c, c, "pinocchio", c.get<PinocchioPkObj>(hfull, Kind::PinocchioPk), shard_index, shard_count, out);
  }, true, false, hfull);
}

int gs_pinocchio_pk_shard_to(gs_handle hfull, size_t shard_index, size_t shard_count, int target_device, gs_handle* out) {
  return guarded_pair(hfull, target_device, [&](Ctx& src, Ctx& dst) -> int {
    return pk_shard_impl(dst, src, "pinocchio", src.get<PinocchioPkObj>(hfull, Kind::PinocchioPk), shard_index, shard_count, out);
  });
}

}  // extern "C"
