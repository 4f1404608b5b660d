// snarkjs / circom .zkey sections onto the device as they lie in the file (include/gosnark_hip.h, "zkey"): base arrays of affine
// Montgomery points, and the coefficient records of section 4 -> the CSR arrays of A and B of a product system.  Nothing here becomes a
// host integer: the bytes are staged through the pinned buffers (hostcopy.h) and every number is converted by one Montgomery product
// on the device (zkey_convert.h).
#include <algorithm>
#include <cstring>

#include "domain.h"
#include "hostcopy.h"
#include "msm.h"
#include "point_io.h"
#include "runtime.h"
#include "scan.h"
#include "zkey_convert.h"

using namespace gs;

namespace {

template <class T>
int upload_affine_mont_bases(Ctx& c, const char* fn, Kind kind, const void* bytes, size_t n, gs_handle* out) {
  if (!out || (n && !bytes)) return fail(GS_ERR_ARG, "%s: null argument", fn);
  if (n >= (1ull << 31)) return fail(GS_ERR_ARG, "%s: too many points", fn);
  auto b = std::make_unique<Bases>(kind);
  b->n = n;
  b->buf.alloc(std::max<size_t>(n, 1) * PointIO<T>::kAffineWords * 4);
  if (n) {
    uint32_t first_bad = 0;
    const uint32_t bad = kind == Kind::G1Bases ? upload_affine_mont_g1(c, bytes, (uint32_t)n, b->buf.as<uint32_t>(), &first_bad)
                                               : upload_affine_mont_g2(c, bytes, (uint32_t)n, b->buf.as<uint32_t>(), &first_bad);
    if (bad) return fail(GS_ERR_ARG, "%s: %u of the %zu points have a coordinate >= q or are not on the curve (first at index %u)", fn, bad, n, first_bad);
  }
  *out = c.put(std::move(b));
  return GS_OK;
}

// ---- section 4: coefficient records -> CSR ---------------------------------------------------------------------------------------
// A record is 11 words: matrix (0 = A, 1 = B), row, signal, 8 words of value * 2^512 mod r.  Three passes over the records:
//   k_zkey_count     counts[matrix * m + row] += 1; a matrix id above 1, a row >= m, a signal >= nvars are counted and located in bad[0..1]
//   (exclusive scan of the 2m + 1 counters, three kernels below)
//   k_zkey_scatter   slot = cursor[matrix * m + row]++ ; col[slot] = signal, val[slot] = value * 2^-512
// The order inside a row is whatever the atomics give: the row's sum is a sum in a field.  Repeated (matrix, row, signal) records stay
// separate entries and add up in the product.
constexpr int kRecWords = 11;

__global__ void __launch_bounds__(256) k_zkey_count(const uint32_t* __restrict__ rec, uint32_t ncoefs, uint32_t m, uint32_t nvars, uint32_t* __restrict__ counts,
                                                     uint32_t* __restrict__ bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncoefs) return;
  const uint32_t* r = rec + (size_t)i * kRecWords;
  const uint32_t mat = r[0], row = r[1], sig = r[2];
  if (mat > 1u || row >= m || sig >= nvars) {
    atomicAdd(bad, 1u);
    atomicMin(bad + 1, i);
    return;
  }
  atomicAdd(&counts[(size_t)mat * m + row], 1u);
}
// offs = the scanned counters (2m + 1): the row pointers of A are offs[0..m], those of B offs[m..2m] less the entries of A
__global__ void __launch_bounds__(256) k_zkey_rowptr(const uint32_t* __restrict__ offs, uint32_t m, uint32_t* __restrict__ rp_a, uint32_t* __restrict__ rp_b) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i > m) return;
  rp_a[i] = offs[i];
  rp_b[i] = offs[(size_t)m + i] - offs[m];
}
// (the records passed k_zkey_count: every index is in range)
__global__ void __launch_bounds__(256) k_zkey_scatter(const uint32_t* __restrict__ rec, uint32_t ncoefs, uint32_t m, uint32_t nnz_a, uint32_t* __restrict__ cursor,
                                                       uint32_t* __restrict__ col_a, uint32_t* __restrict__ val_a, uint32_t* __restrict__ col_b,
                                                       uint32_t* __restrict__ val_b) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncoefs) return;
  const uint32_t* r = rec + (size_t)i * kRecWords;
  const uint32_t mat = r[0], row = r[1], sig = r[2];
  uint32_t w[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) w[j] = r[3 + j];
  const uint32_t slot = atomicAdd(&cursor[(size_t)mat * m + row], 1u);
  uint32_t* col = mat ? col_b : col_a;
  uint32_t* val = mat ? val_b : val_a;
  const uint32_t at = mat ? slot - nnz_a : slot;
  col[at] = sig;
  pack32<ModR>(zkey_coef_to_std(w), w);
#pragma unroll
  for (int j = 0; j < 8; ++j) val[(size_t)at * 8 + j] = w[j];
}

}  // namespace

extern "C" {

// n affine points of G1 / G2 as a .zkey holds them (sections 5-9; 64 / 128 bytes a point) -> an ordinary base-array handle
int gs_g1_upload_affine_mont(const void* bytes, size_t n, gs_handle* out) {
  return guarded([&](Ctx& c) { return upload_affine_mont_bases<FqTag>(c, "gs_g1_upload_affine_mont", Kind::G1Bases, bytes, n, out); });
}
int gs_g2_upload_affine_mont(const void* bytes, size_t n, gs_handle* out) {
  return guarded([&](Ctx& c) { return upload_affine_mont_bases<Fq2Tag>(c, "gs_g2_upload_affine_mont", Kind::G2Bases, bytes, n, out); });
}

// Section 4 of a .zkey (ncoefs records of 44 bytes, behind the count word) -> a domain R1CS over 2^log2_domain rows that is a product
// system: A and B only, c_j = a_j b_j (runtime.h, R1csObj::product).
int gs_r1cs_upload_zkey(size_t log2_domain, size_t nvars, const void* coefs, size_t ncoefs, gs_handle* out) {
  return guarded([&](Ctx& c) -> int {
    const char* fn = "gs_r1cs_upload_zkey";
    if (!out || (ncoefs && !coefs)) return fail(GS_ERR_ARG, "%s: null argument", fn);
    if (log2_domain < 1 || log2_domain > (size_t)kDomainMaxLog2) return fail(GS_ERR_ARG, "%s: log2_domain = %zu, must be 1 .. %d", fn, log2_domain, kDomainMaxLog2);
    if (nvars == 0 || nvars >= (1ull << 31)) return fail(GS_ERR_ARG, "%s: nvars = %zu, must be 1 .. 2^31 - 1", fn, nvars);
    if (ncoefs >= (1ull << 31)) return fail(GS_ERR_ARG, "%s: too many coefficient records", fn);
    const size_t m = (size_t)1 << log2_domain, ncnt = 2 * m + 1;
    const uint32_t ntiles = scan_tiles(ncnt);
    DevBuf rec(std::max<size_t>(ncoefs, 1) * kRecWords * 4), counts(ncnt * 4), tiles((size_t)ntiles * 4), flag(8);
    if (ncoefs) staged_h2d(c, rec.p, coefs, ncoefs * kRecWords * 4, c.stream);
    const uint32_t init[2] = {0u, 0xffffffffu};
    GS_HIP(hipMemcpyAsync(flag.p, init, 8, hipMemcpyHostToDevice, c.stream));
    GS_HIP(hipMemsetAsync(counts.p, 0, ncnt * 4, c.stream));
    if (ncoefs) hipLaunchKernelGGL(k_zkey_count, grid1(ncoefs), dim3(256), 0, c.stream, rec.as<uint32_t>(), (uint32_t)ncoefs, (uint32_t)m, (uint32_t)nvars,
                                   counts.as<uint32_t>(), flag.as<uint32_t>());
    scan_exclusive_dev(c, counts.as<uint32_t>(), ncnt, tiles.as<uint32_t>());
    GS_HIP(hipGetLastError());
    uint32_t res[2] = {0, 0}, nnz_a = 0;
    GS_HIP(hipMemcpyAsync(res, flag.p, 8, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipMemcpyAsync(&nnz_a, counts.as<uint32_t>() + m, 4, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    if (res[0]) {                                            // say what is wrong with the first one (the caller's bytes are still there)
      uint32_t r[3];
      memcpy(r, static_cast<const char*>(coefs) + (size_t)res[1] * kRecWords * 4, sizeof r);
      return fail(GS_ERR_ARG, "%s: %u of the %zu coefficient records are out of range; first at index %u: matrix %u (0 or 1), row %u (< %zu), signal %u (< %zu)",
                  fn, res[0], ncoefs, res[1], r[0], r[1], m, r[2], nvars);
    }
    auto o = std::make_unique<R1csObj>();
    o->n = m; o->m = nvars; o->domain_log2 = (int)log2_domain; o->product = true;
    o->nnz[0] = nnz_a; o->nnz[1] = ncoefs - nnz_a;
    for (int k = 0; k < 2; ++k) {
      o->rowptr[k].alloc((m + 1) * 4);
      o->col[k].alloc(std::max<size_t>(o->nnz[k], 1) * 4);
      o->val[k].alloc(std::max<size_t>(o->nnz[k], 1) * 32);
    }
    hipLaunchKernelGGL(k_zkey_rowptr, grid1(m + 1), dim3(256), 0, c.stream, counts.as<uint32_t>(), (uint32_t)m, o->rowptr[0].as<uint32_t>(), o->rowptr[1].as<uint32_t>());
    if (ncoefs) hipLaunchKernelGGL(k_zkey_scatter, grid1(ncoefs), dim3(256), 0, c.stream, rec.as<uint32_t>(), (uint32_t)ncoefs, (uint32_t)m, nnz_a, counts.as<uint32_t>(),
                                   o->col[0].as<uint32_t>(), o->val[0].as<uint32_t>(), o->col[1].as<uint32_t>(), o->val[1].as<uint32_t>());
    GS_HIP(hipGetLastError());
    GS_HIP(hipStreamSynchronize(c.stream));                  // the scratch buffers go here
    *out = c.put(std::move(o));
    return GS_OK;
  });
}

}  // extern "C"
