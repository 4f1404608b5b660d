// gs_pairing_product (include/gosnark_hip.h, "pairing products on the device"): prod_i e(P_i, Q_i) over two resident arrays.
// One lane per pair runs the Miller loop of miller.h; the values are multiplied across the one-wave workgroup in LDS, one partial
// per workgroup, and k_f12_product folds the partials 64 to 1 per pass until at most kHostPartials are left.  Those cross to the
// host, which finishes the product and runs the ONE final exponentiation with pairing.h (a few thousand Fq products on one core:
// the same tail whatever n is).  Field products are exact and commutative, so the value does not depend on the reduction order.
//
// An Fq12 accumulator is 108 limbs per lane -- k_g2_subgroup already fills the register file with a G2 point -- so it lives in LDS,
// limb-major ([limb][lane]: a wave's access to one limb is 64 consecutive words, no bank conflict), 27 KB per one-wave workgroup.
// The running G2 point, the pair and the line stay in registers.  Partials travel in gs_pairing's standard encoding (96 words).
#include <vector>

#include "miller.h"
#include "pairing.h"
#include "point_io.h"
#include "runtime.h"

using namespace gs;

namespace {

constexpr int kPairBlock = 64;                 // one wave
constexpr int kF12Limbs = 12 * NL;
constexpr int kF12Words = 96;                  // standard encoding, 32-bit words
constexpr size_t kHostPartials = 4;            // at most this many values are downloaded (a host product is ~3 us, a pass ~a launch)

// the accumulator of one lane: limb k of coefficient i at lds[18 i + k][lane]
struct LdsF12 {
  uint32_t* base;
  __device__ __forceinline__ Fq2e<2> get(int i) const {
    Fq2e<2> r;
#pragma unroll
    for (int k = 0; k < NL; ++k) { r.c0.l[k] = base[(2 * NL * i + k) * kPairBlock]; r.c1.l[k] = base[(2 * NL * i + NL + k) * kPairBlock]; }
    return r;
  }
  __device__ __forceinline__ void set(int i, const Fq2e<2>& v) {
#pragma unroll
    for (int k = 0; k < NL; ++k) { base[(2 * NL * i + k) * kPairBlock] = v.c0.l[k]; base[(2 * NL * i + NL + k) * kPairBlock] = v.c1.l[k]; }
  }
};

// the product of the 64 accumulators of the workgroup, written by lane 0 as partial number blockIdx.x
__device__ __forceinline__ void wave_product_store(uint32_t (*lds)[kPairBlock], uint32_t* __restrict__ out) {
  const int lane = threadIdx.x;
#pragma unroll 1
  for (int s = kPairBlock / 2; s >= 1; s >>= 1) {
    __syncthreads();
    if (lane < s) {
      LdsF12 mine{&lds[0][lane]};
      const LdsF12 other{&lds[0][lane + s]};
      f12_mul(mine, other);
    }
  }
  __syncthreads();
  if (lane == 0) {
    const LdsF12 mine{&lds[0][0]};
    f12_to_std(mine, reinterpret_cast<uint64_t*>(out + (size_t)blockIdx.x * kF12Words));
  }
}

__global__ void __launch_bounds__(kPairBlock) k_miller_pairs(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2, uint32_t n,
                                                             uint32_t* __restrict__ partial) {
  __shared__ uint32_t lds[kF12Limbs][kPairBlock];
  const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
  const size_t at = i < n ? i : 0;                                     // lanes past the end read pair 0 and contribute one
  Affine<FqTag> p = PointIO<FqTag>::load_affine(g1 + at * PointIO<FqTag>::kAffineWords);
  const Affine<Fq2Tag> q = PointIO<Fq2Tag>::load_affine(g2 + at * PointIO<Fq2Tag>::kAffineWords);
  if (i >= n) { p.x = fe_zero<ModQ, 1>(); p.y = fe_zero<ModQ, 1>(); }
  LdsF12 f{&lds[0][threadIdx.x]};
  miller_loop(f, p, q);
  wave_product_store(lds, partial);
}

// out[b] = the product of in[64 b .. 64 b + 63] (as far as they exist)
__global__ void __launch_bounds__(kPairBlock) k_f12_product(const uint32_t* __restrict__ in, uint32_t m, uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[kF12Limbs][kPairBlock];
  const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
  LdsF12 f{&lds[0][threadIdx.x]};
  if (i < m) f12_from_std(f, reinterpret_cast<const uint64_t*>(in + i * kF12Words));
  else f12_set_one(f);
  wave_product_store(lds, out);
}

pairing::Fp12 host_f12(const uint64_t* w) {
  using namespace gs::pairing;
  Fp12 f;
  Fp2* c[6] = {&f.a0.c0, &f.a0.c1, &f.a0.c2, &f.a1.c0, &f.a1.c1, &f.a1.c2};
  for (int i = 0; i < 6; ++i) *c[i] = Fp2{fp_from_std(w + 8 * i), fp_from_std(w + 8 * i + 4)};
  return f;
}
void host_f12_to_std(const pairing::Fp12& f, uint64_t* out) {
  using namespace gs::pairing;
  const Fp2* c[6] = {&f.a0.c0, &f.a0.c1, &f.a0.c2, &f.a1.c0, &f.a1.c1, &f.a1.c2};
  for (int i = 0; i < 6; ++i) { fp_to_std(c[i]->c0, out + 8 * i); fp_to_std(c[i]->c1, out + 8 * i + 4); }
}

// the product of the n Miller values, before the final exponentiation
int miller_product_impl(Ctx& c, const char* fn, gs_handle h1, size_t poff, gs_handle h2, size_t qoff, size_t n, pairing::Fp12* out) {
  Bases* ps = c.get<Bases>(h1, Kind::G1Bases);
  Bases* qs = c.get<Bases>(h2, Kind::G2Bases);
  if (!ps) return fail(GS_ERR_ARG, "%s: bad G1 base-array handle", fn);
  if (!qs) return fail(GS_ERR_ARG, "%s: bad G2 base-array handle", fn);
  if (poff > ps->n || ps->n - poff < n) return fail(GS_ERR_SHAPE, "%s: the G1 array has %zu points, %zu were asked for from index %zu", fn, ps->n, n, poff);
  if (qoff > qs->n || qs->n - qoff < n) return fail(GS_ERR_SHAPE, "%s: the G2 array has %zu points, %zu were asked for from index %zu", fn, qs->n, n, qoff);
  if (n >= 0xffffffffull) return fail(GS_ERR_SHAPE, "%s: %zu pairs, indices are 32 bits", fn, n);
  c.drain();
  *out = pairing::f12_one();
  PhaseTimer t(c.stream);
  if (!n) {
    t.stop();
    reset_timing(c);
    c.timing.total_ms = t.ms();
    return GS_OK;
  }
  size_t count = (n + kPairBlock - 1) / kPairBlock;
  DevBuf a(count * kF12Words * 4), b(((count + kPairBlock - 1) / kPairBlock) * kF12Words * 4);
  hipLaunchKernelGGL(k_miller_pairs, dim3((unsigned)count), dim3(kPairBlock), 0, c.stream,
                     ps->buf.as<uint32_t>() + poff * PointIO<FqTag>::kAffineWords, qs->buf.as<uint32_t>() + qoff * PointIO<Fq2Tag>::kAffineWords,
                     (uint32_t)n, a.as<uint32_t>());
  GS_HIP(hipGetLastError());
  DevBuf* src = &a;
  DevBuf* dst = &b;
  while (count > kHostPartials) {
    const size_t next = (count + kPairBlock - 1) / kPairBlock;
    hipLaunchKernelGGL(k_f12_product, dim3((unsigned)next), dim3(kPairBlock), 0, c.stream, src->as<uint32_t>(), (uint32_t)count, dst->as<uint32_t>());
    GS_HIP(hipGetLastError());
    std::swap(src, dst);
    count = next;
  }
  t.stop();
  std::vector<uint64_t> host(count * (kF12Words / 2));
  GS_HIP(hipMemcpyAsync(host.data(), src->p, count * kF12Words * 4, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
  reset_timing(c);
  c.timing.total_ms = t.ms();
  pairing::Fp12 f = host_f12(host.data());
  for (size_t i = 1; i < count; ++i) f = pairing::f12_mul(f, host_f12(host.data() + i * (kF12Words / 2)));
  *out = f;
  return GS_OK;
}

}  // namespace

namespace gs {

// for gs_groth16_verify_batch (verify.hip): the product of the Miller values, the caller multiplies its own pairs in
int miller_product(const char* fn, gs_handle g1, size_t poff, gs_handle g2, size_t qoff, size_t n, pairing::Fp12* out) {
  return guarded([&](Ctx& ctx) -> int { return miller_product_impl(ctx, fn, g1, poff, g2, qoff, n, out); }, true, false, g1);
}

}  // namespace gs

extern "C" {

int gs_pairing_product(gs_handle g1, size_t poff, gs_handle g2, size_t qoff, size_t n, uint64_t out_fq12[48], int* is_one) {
  pairing::Fp12 f;
  const int rc = guarded([&](Ctx& ctx) -> int {
    if (!out_fq12 && !is_one) return fail(GS_ERR_ARG, "gs_pairing_product: both out-pointers are null");
    return miller_product_impl(ctx, "gs_pairing_product", g1, poff, g2, qoff, n, &f);
  }, true, false, g1);
  if (rc != GS_OK) return rc;
  const pairing::Fp12 v = n ? pairing::final_exponentiation(f) : f;   // on the calling thread, outside the context's lock
  if (out_fq12) host_f12_to_std(v, out_fq12);
  if (is_one) *is_one = pairing::f12_eq(v, pairing::f12_one()) ? 1 : 0;
  return GS_OK;
}

}  // extern "C"
