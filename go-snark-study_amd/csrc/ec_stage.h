// The kernels of a radix-2 transform carried out in the group, generic over the curve tag (FqTag: G1, Fq2Tag: G2): the permuting
// load, the point-wise scalar multiplication, one butterfly stage, the normalisation to affine.  ecntt.hip (the arrays a foreign key
// lacks) and zkey_setup.hip (the Lagrange bases of a powers-of-tau transcript) share them.  Every addition is the complete one.
#pragma once
#include "domain.h"
#include "point_io.h"
#include "poly.h"
#include "runtime.h"

namespace gs {

GS_HD void load_words(const uint32_t* __restrict__ p, uint32_t (&k)[8]) {
#pragma unroll
  for (int i = 0; i < 8; ++i) k[i] = p[i];
}

// pts[p] = T[bitrev(p)] for bitrev(p) < n, the point at infinity otherwise (p < 2^k)
template <class T>
__global__ void __launch_bounds__(256) k_ec_load_bitrev(const uint32_t* __restrict__ affine, uint32_t n, uint32_t* __restrict__ pts, int k) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= (1u << k)) return;
  const uint32_t i = dom_bitrev(k, p);
  Xyzz<T> v = xyzz_inf<T>();
  if (i < n) v = xyzz_from_affine(PointIO<T>::load_affine(affine + (size_t)i * PointIO<T>::kAffineWords));
  store_xyzz<T>(pts + (size_t)p * PointIO<T>::kXyzzWords, v);
}

// One radix-2 stage over `total` = 2 * nbf points, butterflies of span `half` (a power of two), twiddle of butterfly j within its
// block: tw[j * tstep] (8 standard-form words each; tw[0] = 1 is not multiplied).
//   forward (decimation in frequency):  (a, b) -> (a + b, (a - b) w)       inverse (decimation in time):  (a, b) -> (a + w b, a - w b)
template <class T, bool kInverse>
__global__ void __launch_bounds__(64) k_ec_stage(uint32_t* __restrict__ pts, uint32_t nbf, uint32_t half, uint32_t tstep, const uint32_t* __restrict__ tw) {
  constexpr int kPw = PointIO<T>::kXyzzWords;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= nbf) return;
  const uint32_t j = t & (half - 1);
  const size_t i0 = (size_t)(t - j) * 2 + j, i1 = i0 + half;
  Xyzz<T> a = load_xyzz<T>(pts + i0 * kPw), b = load_xyzz<T>(pts + i1 * kPw);
  const uint32_t e = j * tstep;
  uint32_t k[8];
  if (e) load_words(tw + (size_t)e * 8, k);
  if (kInverse) {
    if (e && !is_inf(b)) b = xyzz_mul_words_w4(b, k);
    Xyzz<T> d = a;
    xyzz_add(a, b);
    xyzz_add(d, xyzz_neg(b));
    store_xyzz<T>(pts + i0 * kPw, a);
    store_xyzz<T>(pts + i1 * kPw, d);
  } else {
    Xyzz<T> d = a;
    xyzz_add(a, b);
    xyzz_add(d, xyzz_neg(b));
    if (e && !is_inf(d)) d = xyzz_mul_words_w4(d, k);
    store_xyzz<T>(pts + i0 * kPw, a);
    store_xyzz<T>(pts + i1 * kPw, d);
  }
}

// pts[i] = spec[i] * pts[i]
template <class T>
__global__ void __launch_bounds__(64) k_ec_scale(uint32_t* __restrict__ pts, const uint32_t* __restrict__ spec, uint32_t total) {
  constexpr int kPw = PointIO<T>::kXyzzWords;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  Xyzz<T> p = load_xyzz<T>(pts + (size_t)i * kPw);
  if (is_inf(p)) return;
  uint32_t k[8];
  load_words(spec + (size_t)i * 8, k);
  store_xyzz<T>(pts + (size_t)i * kPw, xyzz_mul_words_w4(p, k));
}

template <class T>
__global__ void __launch_bounds__(256) k_ec_to_affine(const uint32_t* __restrict__ pts, uint32_t n, uint32_t* __restrict__ affine) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  PointIO<T>::store_affine(affine + (size_t)i * PointIO<T>::kAffineWords, xyzz_to_affine(load_xyzz<T>(pts + (size_t)i * PointIO<T>::kXyzzWords)));
}

// omega_N^(+-1) as standard-form words, N = 2^logn
inline void ec_root_words(int logn, bool inverse, uint64_t out[4]) {
  Fe<ModR, 2> w;
  for (int i = 0; i < NL; ++i) w.l[i] = inverse ? ModR::omega28_inv_mont(i) : ModR::omega28_mont(i);
  for (int i = 0; i < ModR::kTwoAdicity - logn; ++i) w = sqr(w);
  fr_words_from_mont(w, out);
}

// The decimation-in-time stages (spans 1, 2, .., m / 2) over m = 2^k points loaded in bit-reversed order: the result is in natural
// order.  twi: the m / 2 powers of omega_m^(-1), standard words.
template <class T>
void ec_dit_stages(Ctx& c, uint32_t* pts, int k, const uint32_t* twi) {
  const size_t m = (size_t)1 << k;
  const uint32_t nbf = (uint32_t)(m / 2);
  for (int s = k - 1; s >= 0; --s)
    hipLaunchKernelGGL((k_ec_stage<T, true>), grid1(nbf, 64), dim3(64), 0, c.stream, pts, nbf, (uint32_t)(m >> (s + 1)), 1u << s, twi);
  GS_HIP(hipGetLastError());
}

}  // namespace gs
