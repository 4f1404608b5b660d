// One phase-1 (powers-of-tau) contribution on the device (include/gosnark_hip.h, "contributing to a transcript"): nobody knows the tau of
// the transcript that comes in, so the new secret is multiplied in on the POINTS -- tauG1[i] *= tau^i, alphaTauG1[i] *= alpha tau^i, ..
//   gs_g1_scale_powers / gs_g2_scale_powers   out[i] = (c t^i mod r) P[off + i]: an array of points by a geometric series of scalars
// The series is built on the device (scaled_powers_dev: the scalars never exist on the host) and ONE kernel launch reads the affine
// input, multiplies with the 4-bit window of ec.h (xyzz_mul_words_w4: its 16-point table lives in private memory, as in k_ec_scale)
// and writes affine output; no XYZZ array goes through memory between kernels.  Every addition is the complete one: the input may hold
// infinities, equal and opposite points, and every scalar including 0 is legal.
//
// One inversion per point.  Sharing an inversion across the LANES of a wave saves nothing -- they run it in lock-step anyway -- so the
// only group worth trying is a thread's own points: 2 or 4 of them multiplied one after the other, normalised with Montgomery's trick
// over their ZZZ values.  Tried and measured SLOWER on one MI355X over 2^20 points (G1 28.7 -> 29.8 ms, G2 395 -> 407 ms,
// profiles/ptau_contribute_timing.txt).  The results that wait for the shared inversion live in private memory beside the table;
// whether that traffic is what eats the ~10 % of the products an inversion is was not measured.  Not adopted.
#include <algorithm>

#include "ec_stage.h"
#include "msm.h"

using namespace gs;

namespace {

constexpr int kPtauBlock = 64;

template <class T> constexpr Kind ptau_kind_of() { return T::kWords == 8 ? Kind::G1Bases : Kind::G2Bases; }

// out[i] = spec[i] * in[i], i < n
template <class T>
__global__ void __launch_bounds__(kPtauBlock) k_scale_powers(const uint32_t* __restrict__ in, const uint32_t* __restrict__ spec, uint32_t n,
                                                              uint32_t* __restrict__ out) {
  constexpr int kAw = PointIO<T>::kAffineWords;
  const size_t i = (size_t)blockIdx.x * kPtauBlock + threadIdx.x;
  if (i >= n) return;
  Xyzz<T> p = xyzz_from_affine(PointIO<T>::load_affine(in + i * kAw));
  if (!is_inf(p)) {
    uint32_t k[8];
    load_words(spec + i * 8, k);
    p = xyzz_mul_words_w4(p, k);
  }
  PointIO<T>::store_affine(out + i * kAw, xyzz_to_affine(p));
}

void canon_words(const uint64_t k[4], uint64_t out[4]) {
  uint32_t w[8];
  fr_canon_words(k, w);
  for (int i = 0; i < 4; ++i) out[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
}

template <class T>
int scale_powers_impl(Ctx& c, const char* fn, gs_handle hb, size_t off, size_t n, const uint64_t cc[4], const uint64_t tt[4], gs_handle* out) {
  constexpr int kAw = PointIO<T>::kAffineWords;
  Bases* src = c.get<Bases>(hb, ptau_kind_of<T>());
  if (!src || !out) return fail(GS_ERR_ARG, "%s: bad base-array handle", fn);
  if (!cc || !tt) return fail(GS_ERR_ARG, "%s: null argument", fn);
  if (off > src->n || src->n - off < n) return fail(GS_ERR_SHAPE, "%s: the array has %zu points, %zu were asked for from index %zu", fn, src->n, n, off);
  uint64_t cw[4], tw[4];
  canon_words(cc, cw);
  canon_words(tt, tw);
  c.drain();
  PhaseTimer t(c.stream);
  std::unique_ptr<Bases> b = std::make_unique<Bases>(ptau_kind_of<T>());
  b->n = n;
  b->buf.alloc(n * kAw * 4);
  if (n) {
    DevBuf scal(n * 32);
    scaled_powers_dev(c, tw, cw, n, scal.as<uint32_t>());                       // c t^i, canonical standard words
    hipLaunchKernelGGL(k_scale_powers<T>, grid1(n, kPtauBlock), dim3(kPtauBlock), 0, c.stream, src->buf.as<uint32_t>() + off * kAw, scal.as<uint32_t>(), (uint32_t)n,
                       b->buf.as<uint32_t>());
    GS_HIP(hipGetLastError());
    t.stop();
    GS_HIP(hipStreamSynchronize(c.stream));                                      // the series goes here
  } else {
    t.stop();
  }
  reset_timing(c);
  c.timing.total_ms = t.ms();
  *out = c.put(std::move(b));
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_g1_scale_powers(gs_handle bases, size_t off, size_t n, const uint64_t c[4], const uint64_t t[4], gs_handle* out) {
  return guarded([&](Ctx& ctx) -> int { return scale_powers_impl<FqTag>(ctx, "gs_g1_scale_powers", bases, off, n, c, t, out); }, true, false, bases);
}
int gs_g2_scale_powers(gs_handle bases, size_t off, size_t n, const uint64_t c[4], const uint64_t t[4], gs_handle* out) {
  return guarded([&](Ctx& ctx) -> int { return scale_powers_impl<Fq2Tag>(ctx, "gs_g2_scale_powers", bases, off, n, c, t, out); }, true, false, bases);
}

}  // extern "C"
