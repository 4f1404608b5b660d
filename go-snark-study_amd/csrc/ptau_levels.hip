// Preparing a powers-of-tau transcript for phase 2 (include/gosnark_hip.h, "preparing a transcript"): the Lagrange bases of EVERY
// power-of-two domain of one section, levels lo .. hi, in shared launches.
//   gs_g1_lagrange_levels / gs_g2_lagrange_levels   out[2^p - 2^lo + j] = (1/2^p) sum_{i<2^p} w_p^(-ij) P[i], lo <= p <= hi
// Level by level through gs_g*_lagrange that is sum (p + 1) stage launches, and below about 2^17 butterflies a stage does not fill
// the chip: it costs one scalar multiplication's latency however small it is.  The levels are independent and the stage of span h
// has the same twiddles at every level (levels_plan.h), so here one launch carries the stage of that span for all levels with
// 2^p >= 2h: hi stage launches, one load, one scaling by 2^(-p), one normalisation over the one workspace that holds all levels.
// The kernels are those of ec_stage.h with the level arithmetic in front; every addition is the complete one.
#include <algorithm>

#include "ec_stage.h"
#include "levels_plan.h"
#include "msm.h"

using namespace gs;

namespace {

template <class T> constexpr Kind levels_kind_of() { return T::kWords == 8 ? Kind::G1Bases : Kind::G2Bases; }

// pts[q] = P[bitrev_p(i)] for the point i of level p at workspace index q; a point past the n the array holds is the point at infinity
template <class T>
__global__ void __launch_bounds__(256) k_lv_load_bitrev(const uint32_t* __restrict__ affine, uint32_t n, uint32_t* __restrict__ pts, int lo, uint32_t total) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  const uint32_t i = dom_bitrev(lv_point_level(lo, q), lv_point_within(lo, q));
  Xyzz<T> v = xyzz_inf<T>();
  if (i < n) v = xyzz_from_affine(PointIO<T>::load_affine(affine + (size_t)i * PointIO<T>::kAffineWords));
  store_xyzz<T>(pts + (size_t)q * PointIO<T>::kXyzzWords, v);
}

// pts[q] *= inv2[p] = 2^(-p) for the level p of q (level 0 is left alone)
template <class T>
__global__ void __launch_bounds__(64) k_lv_scale(uint32_t* __restrict__ pts, const uint32_t* __restrict__ inv2, int lo, uint32_t total) {
  constexpr int kPw = PointIO<T>::kXyzzWords;
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  const int p = lv_point_level(lo, q);
  if (p == 0) return;
  Xyzz<T> v = load_xyzz<T>(pts + (size_t)q * kPw);
  if (is_inf(v)) return;
  uint32_t k[8];
  load_words(inv2 + (size_t)p * 8, k);
  store_xyzz<T>(pts + (size_t)q * kPw, xyzz_mul_words_w4(v, k));
}

// The decimation-in-time stage of span 2^s over every level that has one: (a, b) -> (a + w b, a - w b), the body of k_ec_stage<T, true>.
// tw: the 2^(hi-1) powers of omega_(2^hi)^(-1), 8 standard-form words each (tw[0] = 1 is not multiplied).
template <class T>
__global__ void __launch_bounds__(64) k_lv_stage(uint32_t* __restrict__ pts, uint32_t nbf, int lo, int hi, int s, const uint32_t* __restrict__ tw) {
  constexpr int kPw = PointIO<T>::kXyzzWords;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nbf) return;
  const LvButterfly f = lv_butterfly(lo, hi, s, t);
  const size_t i0 = f.i0, i1 = f.i1;
  Xyzz<T> a = load_xyzz<T>(pts + i0 * kPw), b = load_xyzz<T>(pts + i1 * kPw);
  const uint32_t e = f.twiddle;
  uint32_t k[8];
  if (e) load_words(tw + (size_t)e * 8, k);
  if (e && !is_inf(b)) b = xyzz_mul_words_w4(b, k);
  Xyzz<T> d = a;
  xyzz_add(a, b);
  xyzz_add(d, xyzz_neg(b));
  store_xyzz<T>(pts + i0 * kPw, a);
  store_xyzz<T>(pts + i1 * kPw, d);
}

template <class T>
int lagrange_levels_impl(Ctx& c, const char* fn, gs_handle hp, size_t lo_, size_t hi_, gs_handle* out) {
  constexpr int kPw = PointIO<T>::kXyzzWords, kAw = PointIO<T>::kAffineWords;
  Bases* src = c.get<Bases>(hp, levels_kind_of<T>());
  if (!src || !out) return fail(GS_ERR_ARG, "%s: bad base-array handle", fn);
  if (lo_ > hi_ || hi_ > (size_t)kLevelsMaxLog2) return fail(GS_ERR_ARG, "%s: levels %zu .. %zu, must be 0 <= lo <= hi <= %d", fn, lo_, hi_, kLevelsMaxLog2);
  const int lo = (int)lo_, hi = (int)hi_;
  const size_t top = (size_t)1 << hi, half_top = top / 2, total = lv_total(lo, hi);
  if (src->n < top - 1)
    return fail(GS_ERR_SHAPE, "%s: the array has %zu points, level %d needs %zu (or %zu and a last point at infinity)", fn, src->n, hi, top, top - 1);
  c.drain();
  PhaseTimer t(c.stream);
  DevBuf inv2((size_t)(kLevelsMaxLog2 + 1) * 32), twi(std::max<size_t>(half_top, 1) * 32), pts(total * kPw * 4);
  const uint64_t one[4] = {1, 0, 0, 0}, two[4] = {2, 0, 0, 0};
  uint64_t wi[4], half[4];
  ec_root_words(hi, true, wi);
  scaled_powers_dev(c, wi, one, half_top, twi.as<uint32_t>());
  fr_inv_words(two, half);
  scaled_powers_dev(c, half, one, (size_t)kLevelsMaxLog2 + 1, inv2.as<uint32_t>());      // 2^(-p), p = 0 .. 27
  hipLaunchKernelGGL(k_lv_load_bitrev<T>, grid1(total), dim3(256), 0, c.stream, src->buf.as<uint32_t>(), (uint32_t)std::min(src->n, top), pts.as<uint32_t>(), lo,
                     (uint32_t)total);
  hipLaunchKernelGGL(k_lv_scale<T>, grid1(total, 64), dim3(64), 0, c.stream, pts.as<uint32_t>(), inv2.as<uint32_t>(), lo, (uint32_t)total);
  for (int s = 0; s < hi; ++s) {
    const uint32_t nbf = lv_stage_count(lo, hi, s);
    hipLaunchKernelGGL(k_lv_stage<T>, grid1(nbf, 64), dim3(64), 0, c.stream, pts.as<uint32_t>(), nbf, lo, hi, s, twi.as<uint32_t>());
  }
  std::unique_ptr<Bases> b = std::make_unique<Bases>(levels_kind_of<T>());
  b->n = total;
  b->buf.alloc(total * kAw * 4);
  hipLaunchKernelGGL(k_ec_to_affine<T>, grid1(total), dim3(256), 0, c.stream, pts.as<uint32_t>(), (uint32_t)total, b->buf.as<uint32_t>());
  GS_HIP(hipGetLastError());
  t.stop();
  GS_HIP(hipStreamSynchronize(c.stream));
  reset_timing(c);
  c.timing.total_ms = t.ms();
  *out = c.put(std::move(b));
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_g1_lagrange_levels(gs_handle powers, size_t lo, size_t hi, gs_handle* out) {
  return guarded([&](Ctx& c) -> int { return lagrange_levels_impl<FqTag>(c, "gs_g1_lagrange_levels", powers, lo, hi, out); }, true, false, powers);
}
int gs_g2_lagrange_levels(gs_handle powers, size_t lo, size_t hi, gs_handle* out) {
  return guarded([&](Ctx& c) -> int { return lagrange_levels_impl<Fq2Tag>(c, "gs_g2_lagrange_levels", powers, lo, hi, out); }, true, false, powers);
}

}  // extern "C"
