// gs_g1_decompress / gs_g2_decompress / gs_g1_compress / gs_g2_compress (include/gosnark_hip.h, "compressed points"): a point that
// arrives over a wire is an x coordinate and two flag bits -- which of the two roots y is, or that the point is the one at infinity.
// Decompression is y = sqrt(x^3 + b) (sqrt.h: one fixed-exponent power in Fq, two in Fq2, every lane of a wave on the same digit) and
// the sign rule; one thread per point, 64-thread workgroups, no workspace beyond the flag words.  A malformed entry -- a coordinate
// >= q, a right-hand side without a root, an inconsistent flag -- becomes the point at infinity with ok[i] = 0; the count and the
// smallest index come out of two atomics as in g2_subgroup.hip.  The result is an ordinary affine base array.  Compression is the
// way back: x out of Montgomery form and the sign of y.  Byte orders and flag positions of wire formats are host business
// (go-snark-study_amd/compressed.py): the kernels see little-endian words in standard form.
#include "hostcopy.h"
#include "point_io.h"
#include "runtime.h"
#include "sqrt.h"

using namespace gs;

namespace {

constexpr int kCodecBlock = 64;
constexpr uint32_t kFlagLargest = 1u, kFlagInfinity = 2u;      // GS_POINT_LARGEST_Y, GS_POINT_INFINITY

template <class T> constexpr Kind kind_of_tag() { return T::kWords == 8 ? Kind::G1Bases : Kind::G2Bases; }

// 8 little-endian words < q ?
GS_HD bool words_below_q(const uint32_t* w) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) borrow = (((uint64_t)w[i] - ModQ::p32(i) - borrow) >> 32) & 1u;
  return borrow != 0;
}

GS_HD bool coord_sqrt(const Fe<ModQ, 2>& a, Fe<ModQ, 2>& y) { return fq_sqrt(a, y); }
GS_HD bool coord_sqrt(const Fq2e<2>& a, Fq2e<2>& y) { return fq2_sqrt(a, y); }
template <int B> GS_HD bool coord_is_largest(const Fe<ModQ, B>& y) { return fq_is_largest(y); }
template <int B> GS_HD bool coord_is_largest(const Fq2e<B>& y) { return fq2_is_largest(y); }

// x: n x kWords standard-form words, flags: n bytes -> out: n packed affine points, ok: n bytes; bad[0] += bad entries, bad[1] = min(index)
template <class T>
__global__ void __launch_bounds__(kCodecBlock) k_decompress(const uint32_t* __restrict__ x, const uint8_t* __restrict__ flags, uint32_t n,
                                                            uint32_t* __restrict__ out, uint8_t* __restrict__ ok, uint32_t* __restrict__ bad) {
  constexpr int kAw = PointIO<T>::kAffineWords, kCw = PointIO<T>::kCoordWords;
  const size_t i = (size_t)blockIdx.x * kCodecBlock + threadIdx.x;
  if (i >= n) return;
  uint32_t w[kCw], any = 0;
#pragma unroll
  for (int j = 0; j < kCw; ++j) { w[j] = x[i * kCw + j]; any |= w[j]; }
  const uint32_t f = flags[i];
  bool in_range = true;
#pragma unroll
  for (int j = 0; j < kCw; j += 8) in_range = in_range && words_below_q(w + j);
  const auto xm = PointIO<T>::load_std(w);
  const auto rhs = reduce2(add(smul<T>(ssqr<T>(xm), xm), curve_b<T>()));
  typename T::template E<2> y;
  const bool has_root = coord_sqrt(rhs, y);
  const bool flip = coord_is_largest(y) != ((f & kFlagLargest) != 0);
  y = select(flip, reduce2(neg(y)), y);
  const bool inf = (f & kFlagInfinity) != 0;
  const bool good = (f & ~(kFlagLargest | kFlagInfinity)) == 0 && (inf ? (f == kFlagInfinity && any == 0) : (in_range && has_root));
  Affine<T> p;
  p.x = canon(xm);
  p.y = canon(y);
  if (inf || !good) { p.x = T::template zero<1>(); p.y = T::template zero<1>(); }
  PointIO<T>::store_affine(out + i * kAw, p);
  ok[i] = good ? 1 : 0;
  if (!good) {
    atomicAdd(bad, 1u);
    atomicMin(bad + 1, (uint32_t)i);
  }
}

template <class T>
__global__ void __launch_bounds__(kCodecBlock) k_compress(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ x, uint8_t* __restrict__ flags) {
  constexpr int kAw = PointIO<T>::kAffineWords, kCw = PointIO<T>::kCoordWords;
  const size_t i = (size_t)blockIdx.x * kCodecBlock + threadIdx.x;
  if (i >= n) return;
  const Affine<T> p = PointIO<T>::load_affine(in + i * kAw);
  PointIO<T>::store_std(x + i * kCw, p.x);                          // infinity is (0, 0): x = 0 comes out by itself
  flags[i] = is_inf(p) ? (uint8_t)kFlagInfinity : (coord_is_largest(p.y) ? (uint8_t)kFlagLargest : (uint8_t)0);
}

template <class T>
int decompress_impl(Ctx& c, const char* fn, const uint64_t* x, const uint8_t* flags, size_t n, gs_handle* out, uint8_t* ok, uint64_t* nbad, uint64_t* first_bad) {
  constexpr size_t kCoordBytes = PointIO<T>::kCoordWords * 4, kPointBytes = PointIO<T>::kAffineWords * 4;
  if (!out || !nbad || !first_bad || (n && (!x || !flags))) return fail(GS_ERR_ARG, "%s: null argument", fn);
  if (n >= 0xffffffffull) return fail(GS_ERR_SHAPE, "%s: %zu points, indices are 32 bits", fn, n);
  c.drain();
  std::unique_ptr<Bases> r = std::make_unique<Bases>(kind_of_tag<T>());
  r->n = n;
  r->buf.alloc(std::max<size_t>(n, 1) * kPointBytes);
  uint32_t res[2] = {0u, 0xffffffffu};
  float ms = 0;
  if (n) {
    DevBuf dx(n * kCoordBytes), df(n), dok(n), flag(8);
    staged_h2d(c, dx.p, x, n * kCoordBytes, c.stream);
    staged_h2d(c, df.p, flags, n, c.stream);
    GS_HIP(hipMemcpyAsync(flag.p, res, 8, hipMemcpyHostToDevice, c.stream));
    PhaseTimer t(c.stream);
    hipLaunchKernelGGL(k_decompress<T>, grid1(n, kCodecBlock), dim3(kCodecBlock), 0, c.stream, dx.as<uint32_t>(), df.as<uint8_t>(), (uint32_t)n,
                       r->buf.as<uint32_t>(), dok.as<uint8_t>(), flag.as<uint32_t>());
    GS_HIP(hipGetLastError());
    t.stop();
    GS_HIP(hipMemcpyAsync(res, flag.p, 8, hipMemcpyDeviceToHost, c.stream));
    if (ok) GS_HIP(hipMemcpyAsync(ok, dok.p, n, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    ms = t.ms();
  }
  reset_timing(c);
  c.timing.total_ms = ms;
  *nbad = res[0];
  *first_bad = res[0] ? (uint64_t)res[1] : UINT64_MAX;
  *out = c.put(std::move(r));
  return GS_OK;
}

template <class T>
int compress_impl(Ctx& c, const char* fn, gs_handle hb, size_t off, size_t n, uint64_t* x, uint8_t* flags) {
  constexpr size_t kCoordBytes = PointIO<T>::kCoordWords * 4;
  constexpr int kAw = PointIO<T>::kAffineWords;
  Bases* src = c.get<Bases>(hb, kind_of_tag<T>());
  if (!src) return fail(GS_ERR_ARG, "%s: bad base-array handle", fn);
  if (n && (!x || !flags)) return fail(GS_ERR_ARG, "%s: null argument", fn);
  if (off > src->n || src->n - off < n) return fail(GS_ERR_SHAPE, "%s: the array has %zu points, %zu were asked for from index %zu", fn, src->n, n, off);
  if (n >= 0xffffffffull) return fail(GS_ERR_SHAPE, "%s: %zu points, indices are 32 bits", fn, n);
  c.drain();
  float ms = 0;
  if (n) {
    DevBuf dx(n * kCoordBytes), df(n);
    PhaseTimer t(c.stream);
    hipLaunchKernelGGL(k_compress<T>, grid1(n, kCodecBlock), dim3(kCodecBlock), 0, c.stream, src->buf.as<uint32_t>() + off * kAw, (uint32_t)n, dx.as<uint32_t>(),
                       df.as<uint8_t>());
    GS_HIP(hipGetLastError());
    t.stop();
    GS_HIP(hipMemcpyAsync(x, dx.p, n * kCoordBytes, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipMemcpyAsync(flags, df.p, n, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    ms = t.ms();
  }
  reset_timing(c);
  c.timing.total_ms = ms;
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_g1_decompress(const uint64_t* x, const uint8_t* flags, size_t n, gs_handle* out, uint8_t* ok, uint64_t* nbad, uint64_t* first_bad) {
  return guarded([&](Ctx& c) -> int { return decompress_impl<FqTag>(c, "gs_g1_decompress", x, flags, n, out, ok, nbad, first_bad); });
}
int gs_g2_decompress(const uint64_t* x, const uint8_t* flags, size_t n, gs_handle* out, uint8_t* ok, uint64_t* nbad, uint64_t* first_bad) {
  return guarded([&](Ctx& c) -> int { return decompress_impl<Fq2Tag>(c, "gs_g2_decompress", x, flags, n, out, ok, nbad, first_bad); });
}
int gs_g1_compress(gs_handle bases, size_t off, size_t n, uint64_t* x, uint8_t* flags) {
  return guarded([&](Ctx& c) -> int { return compress_impl<FqTag>(c, "gs_g1_compress", bases, off, n, x, flags); }, true, false, bases);
}
int gs_g2_compress(gs_handle bases, size_t off, size_t n, uint64_t* x, uint8_t* flags) {
  return guarded([&](Ctx& c) -> int { return compress_impl<Fq2Tag>(c, "gs_g2_compress", bases, off, n, x, flags); }, true, false, bases);
}

}  // extern "C"
