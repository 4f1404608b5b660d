// gs_pairing_product (include/gosnark_hip.h, "pairing products on the device"): prod_i e(P_i, Q_i) over two resident arrays.
// One lane per pair runs the Miller loop of miller.h; the values are multiplied across the one-wave workgroup in LDS, one partial
// per workgroup, and k_f12_product folds the partials 64 to 1 per pass until at most kHostPartials are left.  Those cross to the
// host, which finishes the product and runs the ONE final exponentiation with pairing.h (a few thousand Fq products on one core:
// the same tail whatever n is).  Field products are exact and commutative, so the value does not depend on the reduction order.
//
// An Fq12 accumulator is 108 limbs per lane -- k_g2_subgroup already fills the register file with a G2 point -- so it lives in LDS,
// limb-major ([limb][lane]: a wave's access to one limb is 64 consecutive words, no bank conflict), 27 KB per one-wave workgroup.
// The running G2 point, the pair and the line stay in registers.  Partials travel in gs_pairing's standard encoding (96 words).
//
// gs_pairing_each: e(P_i, Q_i) for EVERY i.  k_miller_each is the same loop without the product; k_final_exp runs the final
// exponentiation of finalexp.h per lane ("one value per pair" below).  The per-proof verifiers (verify.hip, through verify_device.h)
// put their own Miller kernels in front of the same k_final_exp ("the verify chain" below).
#include <vector>

#include "finalexp.h"
#include "miller.h"
#include "point_io.h"
#include "runtime.h"
#include "verify_device.h"
#include "verify_plan.h"

using namespace gs;

namespace {

constexpr int kPairBlock = 64;                 // one wave
constexpr int kF12Limbs = 12 * NL;
constexpr int kF12Words = 96;                  // standard encoding, 32-bit words
constexpr size_t kHostPartials = 4;            // at most this many values are downloaded (a host product is ~3 us, a pass ~a launch)

// the accumulator of one lane, in LDS or in a slot of the global workspace below: limb k of coefficient i at base[(18 i + k) * 64]
struct LaneF12 {
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
      LaneF12 mine{&lds[0][lane]};
      const LaneF12 other{&lds[0][lane + s]};
      f12_mul(mine, other);
    }
  }
  __syncthreads();
  if (lane == 0) {
    const LaneF12 mine{&lds[0][0]};
    f12_to_std(mine, reinterpret_cast<uint64_t*>(out + (size_t)blockIdx.x * kF12Words));
  }
}

// pair i of two resident arrays; past the end pair 0 with P at infinity, which contributes one
struct PairPQ { Affine<FqTag> p; Affine<Fq2Tag> q; };
__device__ __forceinline__ PairPQ load_pair_or_one(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2, size_t i, uint32_t n) {
  const size_t at = i < n ? i : 0;
  PairPQ r{PointIO<FqTag>::load_affine(g1 + at * PointIO<FqTag>::kAffineWords), PointIO<Fq2Tag>::load_affine(g2 + at * PointIO<Fq2Tag>::kAffineWords)};
  if (i >= n) { r.p.x = fe_zero<ModQ, 1>(); r.p.y = fe_zero<ModQ, 1>(); }
  return r;
}

__global__ void __launch_bounds__(kPairBlock) k_miller_pairs(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2, uint32_t n,
                                                             uint32_t* __restrict__ partial) {
  __shared__ uint32_t lds[kF12Limbs][kPairBlock];
  const PairPQ pq = load_pair_or_one(g1, g2, (size_t)blockIdx.x * kPairBlock + threadIdx.x, n);
  LaneF12 f{&lds[0][threadIdx.x]};
  miller_loop(f, pq.p, pq.q);
  wave_product_store(lds, partial);
}

// out[b] = the product of in[64 b .. 64 b + 63] (as far as they exist)
__global__ void __launch_bounds__(kPairBlock) k_f12_product(const uint32_t* __restrict__ in, uint32_t m, uint32_t* __restrict__ out) {
  __shared__ uint32_t lds[kF12Limbs][kPairBlock];
  const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
  LaneF12 f{&lds[0][threadIdx.x]};
  if (i < m) f12_from_std(f, reinterpret_cast<const uint64_t*>(in + i * kF12Words));
  else f12_set_one(f);
  wave_product_store(lds, out);
}

// ---- one value per pair: gs_pairing_each -------------------------------------------------------------------------------------
// The final exponentiation (finalexp.h) keeps the working value in LDS like the Miller loop and its five temporaries in a global
// workspace of the workgroup, each in the same limb-major [limb][lane] layout: a wave's access to one limb is 64 consecutive
// words.  Slot 0 is also where k_miller_each leaves lane i's Miller value, so nothing passes through the standard encoding.
constexpr size_t kSlotWords = (size_t)kF12Limbs * kPairBlock;
constexpr size_t kWorkspaceWords = kFeSlots * kSlotWords;             // per workgroup

struct GlbBank {
  uint32_t* base;                                                      // the workgroup's workspace + lane
  __device__ __forceinline__ LaneF12 slot(int i) const { return LaneF12{base + (size_t)i * kSlotWords}; }
};

// lane i's Miller value, kept: written to slot 0 of the workgroup's workspace (lanes past the end write one)
__global__ void __launch_bounds__(kPairBlock) k_miller_each(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ g2, uint32_t n,
                                                            uint32_t* __restrict__ workspace) {
  __shared__ uint32_t lds[kF12Limbs][kPairBlock];
  const PairPQ pq = load_pair_or_one(g1, g2, (size_t)blockIdx.x * kPairBlock + threadIdx.x, n);
  LaneF12 f{&lds[0][threadIdx.x]};
  miller_loop(f, pq.p, pq.q);
  LaneF12 out{workspace + (size_t)blockIdx.x * kWorkspaceWords + threadIdx.x};
  f12_copy(out, f);
}

// slot 0 of every lane -> its final exponentiation: whether it is one and, unless out_std is null, the value in the standard encoding
__global__ void __launch_bounds__(kPairBlock) k_final_exp(uint32_t* __restrict__ workspace, uint32_t n, uint32_t* __restrict__ out_std,
                                                          uint32_t* __restrict__ is_one) {
  __shared__ uint32_t lds[kF12Limbs][kPairBlock];
  const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
  LaneF12 w{&lds[0][threadIdx.x]};
  GlbBank bank{workspace + (size_t)blockIdx.x * kWorkspaceWords + threadIdx.x};
  f12_copy(w, bank.slot(0));
  final_exponentiation(w, bank);
  if (i < n) {
    if (out_std) f12_to_std(w, reinterpret_cast<uint64_t*>(out_std + i * kF12Words));
    is_one[i] = f12_is_one(w) ? 1u : 0u;
  }
}

// the window (offset, n) of two resident arrays that gs_pairing_product and gs_pairing_each work on
struct PairWindow { const uint32_t *g1, *g2; };
int pair_window(Ctx& c, const char* fn, gs_handle h1, size_t poff, gs_handle h2, size_t qoff, size_t n, PairWindow& w) {
  Bases* ps = c.get<Bases>(h1, Kind::G1Bases);
  Bases* qs = c.get<Bases>(h2, Kind::G2Bases);
  if (!ps) return fail(GS_ERR_ARG, "%s: bad G1 base-array handle", fn);
  if (!qs) return fail(GS_ERR_ARG, "%s: bad G2 base-array handle", fn);
  if (poff > ps->n || ps->n - poff < n) return fail(GS_ERR_SHAPE, "%s: the G1 array has %zu points, %zu were asked for from index %zu", fn, ps->n, n, poff);
  if (qoff > qs->n || qs->n - qoff < n) return fail(GS_ERR_SHAPE, "%s: the G2 array has %zu points, %zu were asked for from index %zu", fn, qs->n, n, qoff);
  if (n >= 0xffffffffull) return fail(GS_ERR_SHAPE, "%s: %zu pairs, indices are 32 bits", fn, n);
  w = PairWindow{ps->buf.as<uint32_t>() + poff * PointIO<FqTag>::kAffineWords, qs->buf.as<uint32_t>() + qoff * PointIO<Fq2Tag>::kAffineWords};
  return GS_OK;
}

int pairing_each_impl(Ctx& c, const char* fn, gs_handle h1, size_t poff, gs_handle h2, size_t qoff, size_t n, uint64_t* out_fq12, int* is_one) {
  if (!out_fq12 && !is_one) return fail(GS_ERR_ARG, "%s: both out-pointers are null", fn);
  PairWindow w;
  if (const int rc = pair_window(c, fn, h1, poff, h2, qoff, n, w)) return rc;
  c.drain();
  PhaseTimer t(c.stream);
  if (!n) {
    t.stop();
    reset_timing(c);
    c.timing.total_ms = t.ms();
    return GS_OK;
  }
  const size_t count = (n + kPairBlock - 1) / kPairBlock;
  DevBuf ws(count * kWorkspaceWords * 4), vals(out_fq12 ? n * kF12Words * 4 : 0), flags(n * 4);
  PhaseTimer tm(c.stream);
  hipLaunchKernelGGL(k_miller_each, dim3((unsigned)count), dim3(kPairBlock), 0, c.stream, w.g1, w.g2, (uint32_t)n, ws.as<uint32_t>());
  GS_HIP(hipGetLastError());
  tm.stop();
  PhaseTimer tf(c.stream);
  hipLaunchKernelGGL(k_final_exp, dim3((unsigned)count), dim3(kPairBlock), 0, c.stream, ws.as<uint32_t>(), (uint32_t)n,
                     out_fq12 ? vals.as<uint32_t>() : nullptr, flags.as<uint32_t>());
  GS_HIP(hipGetLastError());
  tf.stop();
  t.stop();
  std::vector<uint32_t> host_flags(is_one ? n : 0);
  if (out_fq12) GS_HIP(hipMemcpyAsync(out_fq12, vals.p, n * kF12Words * 4, hipMemcpyDeviceToHost, c.stream));
  if (is_one) GS_HIP(hipMemcpyAsync(host_flags.data(), flags.p, n * 4, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
  if (is_one) for (size_t i = 0; i < n; ++i) is_one[i] = (int)host_flags[i];
  reset_timing(c);
  c.timing.total_ms = t.ms();
  c.timing.accumulate_ms = tm.ms();                                    // the Miller loops
  c.timing.reduce_ms = tf.ms();                                        // the final exponentiations
  return GS_OK;
}

// ---- the verify chain: what gs_groth16_verify_each, gs_groth16_verify_each_keys and gs_pinocchio_verify_each run ------------------
constexpr int kLineWords = 4 * NL;                                     // lambda.c0, lambda.c1, c.c0, c.c1 as limbs
constexpr size_t kListLimbBytes = (size_t)kPreparedSteps * kLineWords * 4;   // one prepared list as limbs

// prepared lines arrive in standard form (pairing.h, prepare_g2_lines): one thread per field element makes limbs of them, once
__global__ void k_std_to_limbs(const uint32_t* __restrict__ in, uint32_t nfe, uint32_t* __restrict__ out) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nfe) return;
  uint32_t w[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) w[k] = in[(size_t)i * 8 + k];
  const Fe<ModQ, 1> v = canon(to_mont(unpack32<ModQ>(w)));
#pragma unroll
  for (int k = 0; k < NL; ++k) out[(size_t)i * NL + k] = v.l[k];
}

// nlists prepared lists in standard form on the host -> limbs at `out`, through `staging` (nlists * kLineStd * 8 bytes); the host
// words and the staging buffer are read by the stream: both live until it has run
void lists_to_limbs(Ctx& c, const uint64_t* std_lists, int nlists, const DevBuf& staging, uint32_t* out) {
  GS_HIP(hipMemcpyAsync(staging.p, std_lists, nlists * kLineStd * 8, hipMemcpyHostToDevice, c.stream));
  const uint32_t nfe = (uint32_t)nlists * kPreparedSteps * 4;
  hipLaunchKernelGGL(k_std_to_limbs, dim3((nfe + 63) / 64), dim3(64), 0, c.stream, staging.as<uint32_t>(), nfe, out);
  GS_HIP(hipGetLastError());
}

struct PreparedLines {                                                 // the same words for every lane: a broadcast load
  const uint32_t* __restrict__ base;
  __device__ __forceinline__ Fq2e<2> pair_at(const uint32_t* p) const {
    Fq2e<2> r;
#pragma unroll
    for (int k = 0; k < NL; ++k) { r.c0.l[k] = p[k]; r.c1.l[k] = p[NL + k]; }
    return r;
  }
  __device__ __forceinline__ Fq2e<2> lambda(int k) const { return pair_at(base + (size_t)k * kLineWords); }
  __device__ __forceinline__ Fq2e<2> c(int k) const { return pair_at(base + (size_t)k * kLineWords + 2 * NL); }
};

// flags[i] = is point i in G2?  (g2_subgroup.h; gs_g2_subgroup_check's kernel reports a count and the first index only)
__global__ void __launch_bounds__(kPairBlock) k_g2_member_flags(const uint32_t* __restrict__ in, uint32_t n, uint32_t* __restrict__ flags) {
  const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
  if (i >= n) return;
  flags[i] = g2_in_subgroup(PointIO<Fq2Tag>::load_affine(in + i * PointIO<Fq2Tag>::kAffineWords)) ? 1u : 0u;
}

// member[i] = is point i of bs in G2, one[l] = is the exponentiated Miller value of lane l one, for the 64 * groups lanes of the
// caller's Miller kernel.  upload() enqueues the caller's copies, points() its per-proof G1 sums and miller(workspace) its Miller
// kernel, which leaves lane l's value in slot 0 of its workgroup's workspace; the caller's buffers are allocated before the call.
template <class Upload, class Points, class Miller>
void run_verify_chain(Ctx& c, const Bases& bs, size_t groups, Upload&& upload, Points&& points, Miller&& miller, int* member, int* one) {
  const size_t nb = bs.n, lanes = groups * kPairBlock;
  DevBuf ws(groups * kWorkspaceWords * 4), flags(lanes * 4), members(nb * 4);
  PhaseTimer t(c.stream), tu(c.stream);
  upload();
  tu.stop();
  PhaseTimer tmem(c.stream);
  hipLaunchKernelGGL(k_g2_member_flags, dim3((unsigned)((nb + kPairBlock - 1) / kPairBlock)), dim3(kPairBlock), 0, c.stream, bs.buf.as<uint32_t>(),
                     (uint32_t)nb, members.as<uint32_t>());
  GS_HIP(hipGetLastError());
  tmem.stop();
  PhaseTimer tv(c.stream);
  points();
  GS_HIP(hipGetLastError());
  tv.stop();
  PhaseTimer tm(c.stream);
  miller(ws.as<uint32_t>());
  GS_HIP(hipGetLastError());
  tm.stop();
  PhaseTimer tf(c.stream);
  hipLaunchKernelGGL(k_final_exp, dim3((unsigned)groups), dim3(kPairBlock), 0, c.stream, ws.as<uint32_t>(), (uint32_t)lanes, (uint32_t*)nullptr,
                     flags.as<uint32_t>());
  GS_HIP(hipGetLastError());
  tf.stop();
  t.stop();
  std::vector<uint32_t> hf(lanes), hm(nb);
  GS_HIP(hipMemcpyAsync(hf.data(), flags.p, lanes * 4, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipMemcpyAsync(hm.data(), members.p, nb * 4, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));                               // the caller's pageable host tables are read by now
  for (size_t l = 0; l < lanes; ++l) one[l] = (int)hf[l];
  for (size_t i = 0; i < nb; ++i) member[i] = (int)hm[i];
  reset_timing(c);
  c.timing.total_ms = t.ms();
  c.timing.h2d_ms = tu.ms();                                           // signals, tables, prepared lists
  c.timing.poly_ms = tmem.ms();                                        // membership of the prover's G2 points
  c.timing.plan_ms = tv.ms();                                          // vkx (and Pinocchio's two sums)
  c.timing.accumulate_ms = tm.ms();                                    // the Miller loops
  c.timing.reduce_ms = tf.ms();                                        // the final exponentiations
}

// ---- a verdict per Groth16 proof: gs_groth16_verify_each, gs_groth16_vk_create, gs_groth16_verify_each_keys (verify.hip) -------------
// One key per one-wave workgroup (verify_plan.h): workgroup g reads its group record and through it its key record, both at addresses
// that depend on blockIdx.x alone, so the key's words -- the pointers here, and the lines, the IC points and the e(alpha, beta) value
// behind them -- are the same for every lane of the wave: broadcast loads.  Every slot exists (the groups are whole), padded slots hold
// the point at infinity and are not read back.
struct VkRecord {                                                      // the per-call key table, one per key of the call
  const uint32_t* lines;                                               // gamma's list, then delta's, as limbs
  const uint32_t* ic;
  const uint64_t* ab;
  uint32_t npublic, skip_gamma, skip_delta, reserved;
};

// vkx_i = IC_0 + sum_j pub_ij IC_{j+1}, one lane per proof (miller.h, groth16_vkx)
__global__ void __launch_bounds__(kPairBlock) k_groth16_vkx_keys(const VkRecord* __restrict__ keys, const VerifyGroup* __restrict__ groups,
                                                                 const uint32_t* __restrict__ pub, uint32_t* __restrict__ out) {
  constexpr int kAw = PointIO<FqTag>::kAffineWords;
  const VerifyGroup g = groups[blockIdx.x];
  const VkRecord key = keys[g.key];
  if (threadIdx.x >= g.valid) return;                                  // a padded slot keeps the infinity the buffer was cleared to
  const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
  const uint32_t* mine = pub + (g.sig_off + (uint64_t)threadIdx.x * key.npublic) * 8;
  const auto point = [&](int j) { return PointIO<FqTag>::load_affine(key.ic + (size_t)j * kAw); };
  const auto bit = [&](int j, int b) { return ((mine[(size_t)j * 8 + (b >> 5)] >> (b & 31)) & 1u) != 0; };
  PointIO<FqTag>::store_affine(out + i * kAw, groth16_vkx(point, bit, (int)key.npublic));
}

// lane i: the Miller value of e(-A_i, B_i) e(vkx_i, gamma) e(C_i, delta) in ONE accumulator, times the key's e(alpha, beta) Miller
// value (ab, standard encoding), into slot 0 of the workgroup's workspace for k_final_exp
__global__ void __launch_bounds__(kPairBlock) k_miller_groth16_keys(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                                    const uint32_t* __restrict__ c, const uint32_t* __restrict__ vkx,
                                                                    const VkRecord* __restrict__ keys, const VerifyGroup* __restrict__ groups,
                                                                    uint32_t* __restrict__ workspace) {
  __shared__ uint32_t lds[kF12Limbs][kPairBlock];
  constexpr int kA1 = PointIO<FqTag>::kAffineWords, kA2 = PointIO<Fq2Tag>::kAffineWords;
  const VkRecord key = keys[groups[blockIdx.x].key];
  const size_t at = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
  Affine<FqTag> p1 = PointIO<FqTag>::load_affine(a + at * kA1);
  const Affine<Fq2Tag> q1 = PointIO<Fq2Tag>::load_affine(b + at * kA2);
  const Affine<FqTag> p2 = PointIO<FqTag>::load_affine(vkx + at * kA1);
  const Affine<FqTag> p3 = PointIO<FqTag>::load_affine(c + at * kA1);
  p1.y = canon(neg(p1.y));                                             // -A; infinity (0, 0) stays infinity
  LaneF12 f{&lds[0][threadIdx.x]};
  miller_loop_groth16(f, p1, q1, p2, key.skip_gamma != 0, PreparedLines{key.lines}, p3, key.skip_delta != 0,
                      PreparedLines{key.lines + (size_t)kPreparedSteps * kLineWords});
  GlbBank bank{workspace + (size_t)blockIdx.x * kWorkspaceWords + threadIdx.x};
  LaneF12 keyval = bank.slot(1);
  f12_from_std(keyval, key.ab);
  f12_mul(f, keyval);
  LaneF12 out = bank.slot(0);
  f12_copy(out, f);
}

// the resident part of a key: the IC array (already uploaded, shared with its handle), the two lists as limbs, the key's Miller value
int vk_install_impl(Ctx& c, const char* fn, gs_handle hic, size_t nic, const Groth16KeyWords& words, gs_handle* out) {
  std::shared_ptr<Bases> ics = c.share<Bases>(hic, Kind::G1Bases);
  if (!ics || ics->n != nic || !nic) return fail(GS_ERR_ARG, "%s: bad IC array", fn);
  if (nic - 1 >= 0xffffffffull) return fail(GS_ERR_SHAPE, "%s: %zu IC points, indices are 32 bits", fn, nic);
  auto vk = std::make_shared<GrothVk>();
  vk->ic = ics;
  vk->npublic = nic - 1;
  vk->skip_gamma = words.skip_gamma;
  vk->skip_delta = words.skip_delta;
  vk->lines.alloc(2 * kListLimbBytes);
  vk->ab.alloc(48 * 8);
  DevBuf staging(2 * kLineStd * 8);
  GS_HIP(hipMemcpyAsync(vk->ab.p, words.ab, 48 * 8, hipMemcpyHostToDevice, c.stream));
  lists_to_limbs(c, words.lines.data(), 2, staging, vk->lines.as<uint32_t>());
  GS_HIP(hipStreamSynchronize(c.stream));                               // the host words and the staging buffer end with this call
  *out = c.put(std::move(vk));
  return GS_OK;
}

int vk_info_impl(Ctx& c, const char* fn, const gs_handle* keys, size_t nkeys, uint32_t* npublic) {
  for (size_t k = 0; k < nkeys; ++k) {
    GrothVk* vk = c.get<GrothVk>(keys[k], Kind::GrothVk);
    if (!vk) return fail(GS_ERR_ARG, "%s: keys[%zu] is not a prepared verification key (gs_groth16_vk_create)", fn, k);
    npublic[k] = (uint32_t)vk->npublic;
  }
  return GS_OK;
}

// member[s], is_one[s] for every SLOT s (64 per group); a, b, c hold the proofs' points in slot order, pub the signals in slot order
int verify_slots_impl(Ctx& c, const char* fn, const Groth16CallKeys& k, gs_handle ha, gs_handle hb, gs_handle hc, const VerifyGroup* groups,
                      size_t ngroups, const uint64_t* pub, uint64_t nsignals, int* member, int* is_one) {
  Bases* as = c.get<Bases>(ha, Kind::G1Bases);
  Bases* bs = c.get<Bases>(hb, Kind::G2Bases);
  Bases* cs = c.get<Bases>(hc, Kind::G1Bases);
  if (!as || !bs || !cs) return fail(GS_ERR_ARG, "%s: bad base-array handle", fn);
  const size_t n = ngroups * kPairBlock;                                // slots
  if (!ngroups || n >= 0xffffffffull) return fail(GS_ERR_SHAPE, "%s: %zu slots, indices are 32 bits", fn, n);
  if (as->n != n || bs->n != n || cs->n != n) return fail(GS_ERR_SHAPE, "%s: the arrays do not hold %zu slots", fn, n);
  // the call's key table: the prepared keys' words where they lie, or the one key of this call in buffers that end with it
  const size_t nkeys = k.keys ? k.nkeys : 1;
  std::vector<VkRecord> table(nkeys);
  DevBuf own_lines, own_ab, staging;
  for (size_t i = 0; k.keys && i < nkeys; ++i) {
    GrothVk* vk = c.get<GrothVk>(k.keys[i], Kind::GrothVk);
    if (!vk) return fail(GS_ERR_ARG, "%s: keys[%zu] is not a prepared verification key on logical device %d", fn, i, c.logical);
    table[i] = VkRecord{vk->lines.as<uint32_t>(), vk->ic->buf.as<uint32_t>(), vk->ab.as<uint64_t>(), (uint32_t)vk->npublic, vk->skip_gamma ? 1u : 0u,
                        vk->skip_delta ? 1u : 0u, 0u};
  }
  if (!k.keys) {
    Bases* ics = c.get<Bases>(k.ic, Kind::G1Bases);
    if (!ics) return fail(GS_ERR_ARG, "%s: bad base-array handle", fn);
    if (k.npublic >= 0xffffffffull || ics->n < k.npublic + 1) return fail(GS_ERR_SHAPE, "%s: the IC array does not hold %zu points", fn, k.npublic + 1);
    own_lines.alloc(2 * kListLimbBytes);
    own_ab.alloc(48 * 8);
    staging.alloc(2 * kLineStd * 8);
    table[0] = VkRecord{own_lines.as<uint32_t>(), ics->buf.as<uint32_t>(), own_ab.as<uint64_t>(), (uint32_t)k.npublic, k.words->skip_gamma ? 1u : 0u,
                        k.words->skip_delta ? 1u : 0u, 0u};
  }
  uint64_t expect = 0;                                                  // the plan against the keys as they are now, under the lock
  for (size_t g = 0; g < ngroups; ++g) {
    if (groups[g].key >= nkeys || !groups[g].valid || groups[g].valid > (uint32_t)kPairBlock || groups[g].sig_off != expect)
      return fail(GS_ERR_ARG, "%s: group %zu does not fit its key", fn, g);
    expect += (uint64_t)groups[g].valid * table[groups[g].key].npublic;
  }
  if (expect != nsignals) return fail(GS_ERR_ARG, "%s: %llu signals for slots that take %llu", fn, (unsigned long long)nsignals, (unsigned long long)expect);
  c.drain();
  constexpr int kAw = PointIO<FqTag>::kAffineWords;
  const size_t pub_bytes = (size_t)nsignals * 32;
  DevBuf vkx(n * kAw * 4), dpub(pub_bytes ? pub_bytes : 32), dkeys(nkeys * sizeof(VkRecord)), dgroups(ngroups * sizeof(VerifyGroup));
  run_verify_chain(
      c, *bs, ngroups,
      [&] {
        if (pub_bytes) GS_HIP(hipMemcpyAsync(dpub.p, pub, pub_bytes, hipMemcpyHostToDevice, c.stream));
        GS_HIP(hipMemcpyAsync(dkeys.p, table.data(), nkeys * sizeof(VkRecord), hipMemcpyHostToDevice, c.stream));
        GS_HIP(hipMemcpyAsync(dgroups.p, groups, ngroups * sizeof(VerifyGroup), hipMemcpyHostToDevice, c.stream));
        GS_HIP(hipMemsetAsync(vkx.p, 0, n * kAw * 4, c.stream));        // infinity in the padded slots
        if (!k.keys) {
          GS_HIP(hipMemcpyAsync(own_ab.p, k.words->ab, 48 * 8, hipMemcpyHostToDevice, c.stream));
          lists_to_limbs(c, k.words->lines.data(), 2, staging, own_lines.as<uint32_t>());
        }
      },
      [&] {
        hipLaunchKernelGGL(k_groth16_vkx_keys, dim3((unsigned)ngroups), dim3(kPairBlock), 0, c.stream, dkeys.as<VkRecord>(), dgroups.as<VerifyGroup>(),
                           dpub.as<uint32_t>(), vkx.as<uint32_t>());
      },
      [&](uint32_t* ws) {
        hipLaunchKernelGGL(k_miller_groth16_keys, dim3((unsigned)ngroups), dim3(kPairBlock), 0, c.stream, as->buf.as<uint32_t>(), bs->buf.as<uint32_t>(),
                           cs->buf.as<uint32_t>(), vkx.as<uint32_t>(), dkeys.as<VkRecord>(), dgroups.as<VerifyGroup>(), ws);
      },
      member, is_one);
  return GS_OK;
}

// ---- a verdict per Pinocchio proof: gs_pinocchio_verify_each (verify.hip) -------------------------------------------------------
// The five equations of snark.VerifyProof as products equal to one.  Six G2 points are the same in every lane and arrive as prepared
// lists, in this order:
enum { kListVka = 0, kListVkc, kListVkz, kListG2Kbg, kListG2Kg, kListGen, kPinLists };
constexpr int kPinEquations = 5;
// the proof's seven G1 points are one array of 7 slabs of n points:
enum { kPtA = 0, kPtAp, kPtBp, kPtC, kPtCp, kPtH, kPtKp, kPinG1 };

// lane i: vkx_i (groth16_vkx), then vkx_i + PiA_i and that sum + PiC_i, affine, for equations 4 and 5
__global__ void __launch_bounds__(kPairBlock) k_pinocchio_points(const uint32_t* __restrict__ ic, const uint32_t* __restrict__ pub, uint32_t npublic,
                                                                 const uint32_t* __restrict__ g1, uint32_t n, uint32_t* __restrict__ xa_out,
                                                                 uint32_t* __restrict__ xac_out) {
  constexpr int kAw = PointIO<FqTag>::kAffineWords;
  const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t* mine = pub + i * npublic * 8;
  const auto point = [&](int j) { return PointIO<FqTag>::load_affine(ic + (size_t)j * kAw); };
  const auto bit = [&](int j, int b) { return ((mine[(size_t)j * 8 + (b >> 5)] >> (b & 31)) & 1u) != 0; };
  const Affine<FqTag> vkx = groth16_vkx(point, bit, (int)npublic);
  Affine<FqTag> xa, xac;
  pinocchio_sums(vkx, PointIO<FqTag>::load_affine(g1 + ((size_t)kPtA * n + i) * kAw), PointIO<FqTag>::load_affine(g1 + ((size_t)kPtC * n + i) * kAw), xa, xac);
  PointIO<FqTag>::store_affine(xa_out + i * kAw, xa);
  PointIO<FqTag>::store_affine(xac_out + i * kAw, xac);
}

// workgroup (x, y): the Miller value of equation y + 1 for the 64 proofs of block x, into slot 0 of workspace y * gridDim.x + x.
//   1  (PiA, Vka) (-PiAp, g2)                         prepared lines only
//   2  (Vkb, PiB) (-PiBp, g2)                         PiB is the live pair
//   3  (PiC, Vkc) (-PiCp, g2)                         prepared lines only
//   4  (vkx + PiA, PiB) (-PiH, Vkz) (-PiC, g2)
//   5  (G1Kbg, PiB) (vkx + PiA + PiC, G2Kbg) (-PiKp, G2Kg)
// The equation is blockIdx.y, so every lane of a workgroup takes the same loop.  key_g1 = Vkb, G1Kbg; skip bit l = list l is absent
// (an infinite key point).
__global__ void __launch_bounds__(kPairBlock) k_miller_pinocchio(const uint32_t* __restrict__ g1, const uint32_t* __restrict__ b,
                                                                 const uint32_t* __restrict__ xa, const uint32_t* __restrict__ xac,
                                                                 const uint32_t* __restrict__ key_g1, uint32_t n, const uint32_t* __restrict__ lines,
                                                                 uint32_t skip_mask, uint32_t* __restrict__ workspace) {
  __shared__ uint32_t lds[kF12Limbs][kPairBlock];
  constexpr int kA1 = PointIO<FqTag>::kAffineWords, kA2 = PointIO<Fq2Tag>::kAffineWords;
  const int eq = blockIdx.y;
  const size_t i = (size_t)blockIdx.x * kPairBlock + threadIdx.x;
  const size_t at = i < n ? i : 0;                                     // lanes past the end run proof 0 and are not read back
  const auto slab = [&](int which) { return g1 + ((size_t)which * n + at) * kA1; };
  // where the three G1 points come from, which of them is negated, and the lists of the second and third pair (the first pair's
  // list for the prepared loop): the same for every lane
  const uint32_t *s1, *s2, *s3 = slab(kPtA);
  int l1 = kListGen, l2 = kListGen, l3 = kListGen;
  bool neg2 = true, no3 = false;
  switch (eq) {
    case 0: s1 = slab(kPtA); l1 = kListVka; s2 = slab(kPtAp); no3 = true; break;
    case 1: s1 = key_g1; s2 = slab(kPtBp); no3 = true; break;
    case 2: s1 = slab(kPtC); l1 = kListVkc; s2 = slab(kPtCp); no3 = true; break;
    case 3: s1 = xa + at * kA1; s2 = slab(kPtH); l2 = kListVkz; s3 = slab(kPtC); break;
    default: s1 = key_g1 + kA1; s2 = xac + at * kA1; l2 = kListG2Kbg; neg2 = false; s3 = slab(kPtKp); l3 = kListG2Kg; break;
  }
  const Affine<FqTag> p1 = PointIO<FqTag>::load_affine(s1);
  Affine<FqTag> p2 = PointIO<FqTag>::load_affine(s2), p3 = PointIO<FqTag>::load_affine(s3);
  if (neg2) p2.y = canon(neg(p2.y));                                   // infinity (0, 0) stays infinity
  p3.y = canon(neg(p3.y));
  const auto list = [&](int l) { return PreparedLines{lines + (size_t)l * kPreparedSteps * kLineWords}; };
  const auto absent = [&](int l) { return ((skip_mask >> l) & 1u) != 0; };
  LaneF12 f{&lds[0][threadIdx.x]};
  if (eq == 0 || eq == 2) {
    miller_loop_prepared(f, p1, absent(l1), list(l1), p2, absent(l2), list(l2), p3, true, list(l3));
  } else {
    const Affine<Fq2Tag> q1 = PointIO<Fq2Tag>::load_affine(b + at * kA2);
    miller_loop_groth16(f, p1, q1, p2, absent(l2), list(l2), p3, no3 || absent(l3), list(l3));
  }
  LaneF12 out{workspace + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kWorkspaceWords + threadIdx.x};
  f12_copy(out, f);
}

// member[i] = is PiB_i in G2, one[e * n + i] = is the exponentiated value of equation e + 1 of proof i one
int pinocchio_each_impl(Ctx& c, const char* fn, gs_handle hg1, gs_handle hb, gs_handle hic, gs_handle hkey, const uint64_t* pub, size_t npublic, size_t n,
                        const uint64_t* lines_std_host, unsigned skip_mask, int* member, int* one) {
  Bases* gs1 = c.get<Bases>(hg1, Kind::G1Bases);
  Bases* bs = c.get<Bases>(hb, Kind::G2Bases);
  Bases* ics = c.get<Bases>(hic, Kind::G1Bases);
  Bases* keys = c.get<Bases>(hkey, Kind::G1Bases);
  if (!gs1 || !bs || !ics || !keys) return fail(GS_ERR_ARG, "%s: bad base-array handle", fn);
  if (!n || n >= 0xffffffffull / (kPinEquations * 2) || npublic >= 0xffffffffull) return fail(GS_ERR_SHAPE, "%s: %zu proofs, indices are 32 bits", fn, n);
  if (gs1->n != kPinG1 * n || bs->n != n || keys->n != 2 || ics->n < npublic + 1) return fail(GS_ERR_SHAPE, "%s: the arrays do not hold %zu proofs", fn, n);
  c.drain();
  constexpr int kAw = PointIO<FqTag>::kAffineWords;
  const size_t count = (n + kPairBlock - 1) / kPairBlock;               // workgroups per equation: its lanes are padded to whole ones
  const size_t pub_bytes = n * npublic * 32;
  DevBuf xa(n * kAw * 4), xac(n * kAw * 4), dpub(pub_bytes ? pub_bytes : 32), staging(kPinLists * kLineStd * 8), lines(kPinLists * kListLimbBytes);
  std::vector<int> lane_one(kPinEquations * count * kPairBlock);
  run_verify_chain(
      c, *bs, kPinEquations * count,
      [&] {
        if (pub_bytes) GS_HIP(hipMemcpyAsync(dpub.p, pub, pub_bytes, hipMemcpyHostToDevice, c.stream));
        lists_to_limbs(c, lines_std_host, kPinLists, staging, lines.as<uint32_t>());
      },
      [&] {
        hipLaunchKernelGGL(k_pinocchio_points, dim3((unsigned)count), dim3(kPairBlock), 0, c.stream, ics->buf.as<uint32_t>(), dpub.as<uint32_t>(),
                           (uint32_t)npublic, gs1->buf.as<uint32_t>(), (uint32_t)n, xa.as<uint32_t>(), xac.as<uint32_t>());
      },
      [&](uint32_t* ws) {
        hipLaunchKernelGGL(k_miller_pinocchio, dim3((unsigned)count, kPinEquations), dim3(kPairBlock), 0, c.stream, gs1->buf.as<uint32_t>(),
                           bs->buf.as<uint32_t>(), xa.as<uint32_t>(), xac.as<uint32_t>(), keys->buf.as<uint32_t>(), (uint32_t)n, lines.as<uint32_t>(),
                           (uint32_t)skip_mask, ws);
      },
      member, lane_one.data());
  for (size_t e = 0; e < (size_t)kPinEquations; ++e)
    for (size_t i = 0; i < n; ++i) one[e * n + i] = lane_one[e * count * kPairBlock + i];
  return GS_OK;
}

// the product of the n Miller values, before the final exponentiation
int miller_product_impl(Ctx& c, const char* fn, gs_handle h1, size_t poff, gs_handle h2, size_t qoff, size_t n, pairing::Fp12* out) {
  PairWindow w;
  if (const int rc = pair_window(c, fn, h1, poff, h2, qoff, n, w)) return rc;
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
  hipLaunchKernelGGL(k_miller_pairs, dim3((unsigned)count), dim3(kPairBlock), 0, c.stream, w.g1, w.g2, (uint32_t)n, a.as<uint32_t>());
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
  pairing::Fp12 f = pairing::f12_from_std(host.data());
  for (size_t i = 1; i < count; ++i) f = pairing::f12_mul(f, pairing::f12_from_std(host.data() + i * (kF12Words / 2)));
  *out = f;
  return GS_OK;
}

}  // namespace

namespace gs {

int miller_product(const char* fn, gs_handle g1, size_t poff, gs_handle g2, size_t qoff, size_t n, pairing::Fp12* out) {
  return guarded([&](Ctx& ctx) -> int { return miller_product_impl(ctx, fn, g1, poff, g2, qoff, n, out); }, true, false, g1);
}
int groth16_vk_install(const char* fn, gs_handle hic, size_t nic, const Groth16KeyWords& words, gs_handle* out) {
  return guarded([&](Ctx& ctx) -> int { return vk_install_impl(ctx, fn, hic, nic, words, out); }, true, true, hic);
}
int groth16_vk_info(const char* fn, const gs_handle* keys, size_t nkeys, uint32_t* npublic) {
  return guarded([&](Ctx& ctx) -> int { return vk_info_impl(ctx, fn, keys, nkeys, npublic); }, true, true, nkeys ? keys[0] : 0);
}
int groth16_verify_slots_device(const char* fn, const Groth16CallKeys& keys, gs_handle ha, gs_handle hb, gs_handle hc, const VerifyGroup* groups,
                                size_t ngroups, const uint64_t* pub, uint64_t nsignals, int* member, int* is_one) {
  return guarded([&](Ctx& ctx) -> int { return verify_slots_impl(ctx, fn, keys, ha, hb, hc, groups, ngroups, pub, nsignals, member, is_one); }, true,
                 false, ha);
}
int pinocchio_verify_each_device(const char* fn, gs_handle g1, gs_handle hb, gs_handle hic, gs_handle key, const uint64_t* pub, size_t npublic, size_t n,
                                 const uint64_t* lines, unsigned skip_mask, int* member, int* one) {
  return guarded([&](Ctx& ctx) -> int { return pinocchio_each_impl(ctx, fn, g1, hb, hic, key, pub, npublic, n, lines, skip_mask, member, one); }, true,
                 false, g1);
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
  if (out_fq12) pairing::f12_to_std(v, out_fq12);
  if (is_one) *is_one = pairing::f12_eq(v, pairing::f12_one()) ? 1 : 0;
  return GS_OK;
}

int gs_pairing_each(gs_handle g1, size_t poff, gs_handle g2, size_t qoff, size_t n, uint64_t* out_fq12, int* is_one) {
  return guarded([&](Ctx& ctx) -> int { return pairing_each_impl(ctx, "gs_pairing_each", g1, poff, g2, qoff, n, out_fq12, is_one); }, true, false, g1);
}

}  // extern "C"
