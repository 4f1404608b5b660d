// gs_g2_subgroup_check (include/gosnark_hip.h, "G2 subgroup membership of whole arrays"): which points of a resident G2 array lie
// outside the order-r subgroup?  The uploads test the curve equation only and the twist's cofactor has the factor 10069, so the random
// linear combinations of the transcript and key checks let a point tau^j G2 + S, ord(S) = 10069, through once in 10069 challenges.
// One thread per point runs g2_in_subgroup (g2_subgroup.h: a multiplication by the fixed 63-bit BN parameter along its non-adjacent
// form, three applications of psi, no inversion); the count and the smallest index come out of two atomics.  The kernel reads the
// affine array and nothing else: no window table, no workspace beyond the two result words.
#include "g2_subgroup.h"
#include "point_io.h"
#include "runtime.h"

using namespace gs;

namespace {

constexpr int kMemberBlock = 64;

// bad[0] += points outside the subgroup, bad[1] = min(their index + base)
__global__ void __launch_bounds__(kMemberBlock) k_g2_subgroup(const uint32_t* __restrict__ in, uint32_t n, uint32_t base, uint32_t* __restrict__ bad) {
  constexpr int kAw = PointIO<Fq2Tag>::kAffineWords;
  const size_t i = (size_t)blockIdx.x * kMemberBlock + threadIdx.x;
  if (i >= n) return;
  if (!g2_in_subgroup(PointIO<Fq2Tag>::load_affine(in + i * kAw))) {
    atomicAdd(bad, 1u);
    atomicMin(bad + 1, base + (uint32_t)i);
  }
}

int subgroup_check_impl(Ctx& c, gs_handle hb, size_t off, size_t n, uint64_t* nbad, uint64_t* first_bad) {
  constexpr int kAw = PointIO<Fq2Tag>::kAffineWords;
  const char* fn = "gs_g2_subgroup_check";
  Bases* src = c.get<Bases>(hb, Kind::G2Bases);
  if (!src) return fail(GS_ERR_ARG, "%s: bad G2 base-array handle", fn);
  if (!nbad || !first_bad) return fail(GS_ERR_ARG, "%s: null argument", fn);
  if (off > src->n || src->n - off < n) return fail(GS_ERR_SHAPE, "%s: the array has %zu points, %zu were asked for from index %zu", fn, src->n, n, off);
  if (src->n >= 0xffffffffull) return fail(GS_ERR_SHAPE, "%s: the array has %zu points, indices are 32 bits", fn, src->n);
  c.drain();
  uint32_t res[2] = {0u, 0xffffffffu};
  PhaseTimer t(c.stream);
  if (n) {
    DevBuf flag(8);
    GS_HIP(hipMemcpyAsync(flag.p, res, 8, hipMemcpyHostToDevice, c.stream));
    hipLaunchKernelGGL(k_g2_subgroup, grid1(n, kMemberBlock), dim3(kMemberBlock), 0, c.stream, src->buf.as<uint32_t>() + off * kAw, (uint32_t)n, (uint32_t)off,
                       flag.as<uint32_t>());
    GS_HIP(hipGetLastError());
    t.stop();
    GS_HIP(hipMemcpyAsync(res, flag.p, 8, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));                                      // the flag words go here
  } else {
    t.stop();
  }
  reset_timing(c);
  c.timing.total_ms = t.ms();
  *nbad = res[0];
  *first_bad = res[0] ? (uint64_t)res[1] : UINT64_MAX;
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_g2_subgroup_check(gs_handle points, size_t off, size_t n, uint64_t* nbad, uint64_t* first_bad) {
  return guarded([&](Ctx& ctx) -> int { return subgroup_check_impl(ctx, points, off, n, nbad, first_bad); }, true, false, points);
}

}  // extern "C"
