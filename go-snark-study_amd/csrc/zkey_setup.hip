// The device half of a Groth16 setup from a powers-of-tau transcript (include/gosnark_hip.h, "setup from a transcript"): nobody knows
// tau, so everything the reference's GenerateTrustedSetup does on scalars (setup.hip) happens on POINTS here.
//   gs_g1_lagrange / gs_g2_lagrange   the Lagrange basis of the domain at tau = one inverse transform of the tau-powers in the group
//                                     (ec_stage.h: the stages of ecntt.hip); odd_half: the odd entries of the transform of twice the size,
//                                     which is the coset evaluation basis of the quotient -- one transform of size n over P[i+n] - P[i]
//                                     with the scalars of the foreign-key derivation (domain.h)
//   gs_r1cs_colsum_g1 / _g2           out[s] = sum of coefficient x basis point over column s of the sparse matrices: the transposed
//                                     sparse mat-vec of setup.hip over points (colsum_plan.h: the index arithmetic)
//   gs_g1_scale                       k P[i]: a phase-2 contribution
//   gs_g1 / g2_download_affine_mont   a base array as the bytes a .zkey holds
// All arithmetic is exact and every addition the complete one: a transcript or a basis may hold infinities, equal and opposite points.
#include <algorithm>

#include "colsum_plan.h"
#include "ec_stage.h"
#include "scan.h"

using namespace gs;

namespace {

template <class T> constexpr Kind kind_of() { return T::kWords == 8 ? Kind::G1Bases : Kind::G2Bases; }

struct Words8 { uint32_t w[8]; };

// mag * p for a finite or infinite affine p, through the low `bits` bits of mag (bits = bitlen(mag) >= 1): double and add, the addend
// affine -- bits - 1 doublings and one mixed addition per set bit; -2 costs one doubling, not a 254-bit ladder
template <class T>
GS_HD Xyzz<T> mul_affine_bits(const Affine<T>& p, const uint32_t (&mag)[8], int bits) {
  Xyzz<T> acc = xyzz_from_affine(p);
  if (is_inf(p)) return acc;
  for (int b = bits - 2; b >= 0; --b) {
    xyzz_dbl(acc);
    if ((mag[b >> 5] >> (b & 31)) & 1u) xyzz_madd(acc, p);
  }
  return acc;
}

// ---- Lagrange bases ----------------------------------------------------------------------------------------------------------------
// pts[p] = P[i + n] - P[i], i = bitrev(p), n = 2^k; P has `avail` >= 2n - 1 points and a missing P[2n - 1] is the point at infinity
template <class T>
__global__ void __launch_bounds__(256) k_ls_load_diff(const uint32_t* __restrict__ affine, uint32_t avail, uint32_t* __restrict__ pts, int k) {
  constexpr int kAw = PointIO<T>::kAffineWords;
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x, n = 1u << k;
  if (p >= n) return;
  const uint32_t i = dom_bitrev(k, p);
  Xyzz<T> v = xyzz_inf<T>();
  if (i + n < avail) v = xyzz_from_affine(PointIO<T>::load_affine(affine + (size_t)(i + n) * kAw));
  xyzz_madd(v, PointIO<T>::load_affine(affine + (size_t)i * kAw), true);
  store_xyzz<T>(pts + (size_t)p * PointIO<T>::kXyzzWords, v);
}

template <class T>
int lagrange_impl(Ctx& c, const char* fn, gs_handle hp, size_t off, size_t log2_n, int odd_half, gs_handle* out) {
  constexpr int kPw = PointIO<T>::kXyzzWords, kAw = PointIO<T>::kAffineWords;
  Bases* src = c.get<Bases>(hp, kind_of<T>());
  if (!src || !out) return fail(GS_ERR_ARG, "%s: bad base-array handle", fn);
  if (odd_half != 0 && odd_half != 1) return fail(GS_ERR_ARG, "%s: odd_half = %d, must be 0 or 1", fn, odd_half);
  if (log2_n > (size_t)kDomainMaxLog2 || (odd_half && log2_n < 1))
    return fail(GS_ERR_ARG, "%s: log2_n = %zu, must be %d .. %d", fn, log2_n, odd_half ? 1 : 0, kDomainMaxLog2);
  const int k = (int)log2_n;
  const size_t n = (size_t)1 << k, need = odd_half ? 2 * n - 1 : n, half_n = n / 2;
  if (off > src->n || src->n - off < need)
    return fail(GS_ERR_SHAPE, "%s: the array has %zu points, the transform needs %zu from index %zu", fn, src->n, need, off);
  c.drain();
  PhaseTimer t(c.stream);
  DevBuf scal(n * 32), twi(std::max<size_t>(half_n, 1) * 32), pts(n * kPw * 4);
  const uint64_t one[4] = {1, 0, 0, 0};
  uint64_t wi[4];
  ec_root_words(k, true, wi);
  scaled_powers_dev(c, wi, one, half_n, twi.as<uint32_t>());
  const uint32_t* p = src->buf.as<uint32_t>() + off * kAw;
  if (odd_half) {
    // entry 2j + 1 of the transform of size 2n = sum_i omega^(-ij) [(1/(2n)) g^(-i) (P[i] - P[i+n])]: the derivation's scalars carry the minus
    domain_derive_scalars_dev(c, k, scal.as<uint32_t>());
    hipLaunchKernelGGL(k_ls_load_diff<T>, grid1(n), dim3(256), 0, c.stream, p, (uint32_t)std::min(src->n - off, 2 * n), pts.as<uint32_t>(), k);
  } else {
    const uint64_t nn[4] = {(uint64_t)n, 0, 0, 0};
    uint64_t inv_n[4];
    fr_inv_words(nn, inv_n);
    scaled_powers_dev(c, one, inv_n, n, scal.as<uint32_t>());                 // 1 / n in every slot
    hipLaunchKernelGGL(k_ec_load_bitrev<T>, grid1(n), dim3(256), 0, c.stream, p, (uint32_t)n, pts.as<uint32_t>(), k);
  }
  hipLaunchKernelGGL(k_ec_scale<T>, grid1(n, 64), dim3(64), 0, c.stream, pts.as<uint32_t>(), scal.as<uint32_t>(), (uint32_t)n);
  ec_dit_stages<T>(c, pts.as<uint32_t>(), k, twi.as<uint32_t>());
  std::unique_ptr<Bases> b = std::make_unique<Bases>(kind_of<T>());
  b->n = n;
  b->buf.alloc(n * kAw * 4);
  hipLaunchKernelGGL(k_ec_to_affine<T>, grid1(n), dim3(256), 0, c.stream, pts.as<uint32_t>(), (uint32_t)n, b->buf.as<uint32_t>());
  GS_HIP(hipGetLastError());
  t.stop();
  GS_HIP(hipStreamSynchronize(c.stream));
  reset_timing(c);
  c.timing.total_ms = t.ms();
  *out = c.put(std::move(b));
  return GS_OK;
}

// ---- column sums -------------------------------------------------------------------------------------------------------------------
// counts[signal] += 1 for every term of one matrix whose coefficient is not 0 mod r
__global__ void __launch_bounds__(256) k_cs_count(const uint32_t* __restrict__ col, const uint32_t* __restrict__ val, uint32_t nnz, uint32_t* __restrict__ counts) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  uint32_t v[8];
  load_words(val + (size_t)e * 8, v);
  cs_canon(v);
  if (cs_bitlen(v)) atomicAdd(&counts[col[e]], 1u);
}

// The terms of matrix `src` into the signal-sorted entry list (the order inside a column is whatever the atomics give: the sum is a sum in
// a group).  A unit term refers to its basis point; a general term takes the next number j of its list (short or long) and leaves its
// point reference and magnitude for k_cs_mul at slot j (short) or gcap - 1 - j (long) of the work arrays: two lists in one allocation.
// Its product will be entry j (short) or nshort + j (long) of the product array, which is as long as the two lists together.
__global__ void __launch_bounds__(256) k_cs_scatter(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col, const uint32_t* __restrict__ val,
                                                     uint32_t nnz, uint32_t nrows, uint32_t src, uint32_t* __restrict__ cursor, uint32_t* __restrict__ keys,
                                                     uint32_t* __restrict__ ent, uint32_t* __restrict__ gcnt, uint32_t gcap, uint32_t* __restrict__ gref,
                                                     uint32_t* __restrict__ gmag) {
  const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nnz) return;
  uint32_t v[8], mag[8];
  load_words(val + (size_t)e * 8, v);
  bool negate;
  int bits;
  const uint32_t cls = cs_classify(v, mag, negate, bits);
  if (cls == kCsZero) return;
  uint32_t lo = 0, hi = nrows;                               // the row: the last one with rowptr[row] <= e
  while (lo + 1 < hi) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (rowptr[mid] <= e) lo = mid; else hi = mid;
  }
  const uint32_t s = col[e], slot = atomicAdd(&cursor[s], 1u);
  keys[slot] = s;
  if (cls == kCsUnit) { ent[slot] = cs_entry(negate, src, lo); return; }
  const uint32_t j = atomicAdd(&gcnt[cls == kCsShort ? 0 : 1], 1u), g = cls == kCsShort ? j : gcap - 1u - j;
  gref[g] = (src << kCsSrcShift) | lo;
  gmag[(size_t)g * 9] = (uint32_t)bits;
#pragma unroll
  for (int j = 0; j < 8; ++j) gmag[(size_t)g * 9 + 1 + j] = mag[j];
  ent[slot] = cs_entry(negate, kCsSrcGeneral, cls == kCsShort ? j : kCsLongFlag | j);
}

struct CsSources { const uint32_t* p[4]; };
GS_HD const uint32_t* cs_source(const CsSources& s, uint32_t which) { return which == 0 ? s.p[0] : which == 1 ? s.p[1] : which == 2 ? s.p[2] : s.p[3]; }

// prod[t] = magnitude x basis point of the general term in slot g = from_top ? gcap - 1 - t : t of the work arrays, affine, t < count
template <class T>
__global__ void __launch_bounds__(64) k_cs_mul(CsSources srcs, const uint32_t* __restrict__ gref, const uint32_t* __restrict__ gmag, uint32_t gcap, bool from_top,
                                                uint32_t count, uint32_t* __restrict__ prod) {
  constexpr int kAw = PointIO<T>::kAffineWords;
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const uint32_t g = from_top ? gcap - 1u - t : t, ref = gref[g];
  uint32_t mag[8];
  load_words(gmag + (size_t)g * 9 + 1, mag);
  const Affine<T> p = PointIO<T>::load_affine(cs_source(srcs, ref >> kCsSrcShift) + (size_t)(ref & kCsIdxMask) * kAw);
  PointIO<T>::store_affine(prod + (size_t)t * kAw, xyzz_to_affine(mul_affine_bits<T>(p, mag, (int)gmag[(size_t)g * 9])));
}

template <class T>
struct CsSinkBase {
  static constexpr int kPw = PointIO<T>::kXyzzWords;
  Xyzz<T> acc;
  uint32_t* result;
  uint32_t* part_keys;
  uint32_t* part_pts;
  GS_HD void begin() { acc = xyzz_inf<T>(); }
  GS_HD void out(uint32_t key) { store_xyzz<T>(result + (size_t)key * kPw, acc); }
  GS_HD void partial(uint32_t slot, uint32_t key) { part_keys[slot] = key; store_xyzz<T>(part_pts + (size_t)slot * kPw, acc); }
  GS_HD void empty(uint32_t slot, uint32_t key) { part_keys[slot] = key; store_xyzz<T>(part_pts + (size_t)slot * kPw, xyzz_inf<T>()); }
};
template <class T>
struct CsSinkFirst : CsSinkBase<T> {          // the first level: entries refer to affine points
  CsSources srcs;
  const uint32_t* ent;
  uint32_t nshort;
  GS_HD void add(uint32_t i) {
    const uint32_t e = ent[i], src = (e >> kCsSrcShift) & 3u;
    uint32_t idx = e & kCsIdxMask;
    if (src == kCsSrcGeneral && (idx & kCsLongFlag)) idx = nshort + (idx ^ kCsLongFlag);
    xyzz_madd(this->acc, PointIO<T>::load_affine(cs_source(srcs, src) + (size_t)idx * PointIO<T>::kAffineWords), (e & kCsSignBit) != 0u);
  }
};
template <class T>
struct CsSinkNext : CsSinkBase<T> {           // the levels above: entries are the partial sums of the level below
  const uint32_t* pts;
  GS_HD void add(uint32_t i) { xyzz_add_mem<T>(this->acc, pts + (size_t)i * CsSinkBase<T>::kPw); }
};

template <class T>
__global__ void __launch_bounds__(64) k_cs_reduce_first(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ ent, uint32_t n, CsSources srcs,
                                                         uint32_t nshort, uint32_t* __restrict__ out, uint32_t* __restrict__ part_keys, uint32_t* __restrict__ part_pts) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cs_chunks(n)) return;
  CsSinkFirst<T> s;
  s.result = out; s.part_keys = part_keys; s.part_pts = part_pts; s.srcs = srcs; s.ent = ent; s.nshort = nshort;
  cs_reduce_chunk(keys, n, c, s);
}
template <class T>
__global__ void __launch_bounds__(64) k_cs_reduce_next(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ pts, uint32_t n, uint32_t* __restrict__ out,
                                                        uint32_t* __restrict__ part_keys, uint32_t* __restrict__ part_pts) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cs_chunks(n)) return;
  CsSinkNext<T> s;
  s.result = out; s.part_keys = part_keys; s.part_pts = part_pts; s.pts = pts;
  cs_reduce_chunk(keys, n, c, s);
}

template <class T>
int colsum_impl(Ctx& c, const char* fn, gs_handle hr, const gs_handle hb[3], gs_handle* out) {
  constexpr int kPw = PointIO<T>::kXyzzWords, kAw = PointIO<T>::kAffineWords;
  R1csObj* o = c.get<R1csObj>(hr, Kind::R1cs);
  if (!o || !out) return fail(GS_ERR_ARG, "%s: bad R1CS handle", fn);
  if (o->product && hb[2]) return fail(GS_ERR_SHAPE, "%s: the system is a product system (gs_r1cs_upload_zkey): it has no C matrix, basis_c must be 0", fn);
  Bases* b[3] = {nullptr, nullptr, nullptr};
  size_t terms = 0;
  for (int k = 0; k < 3; ++k) {
    if (!hb[k]) continue;
    b[k] = c.get<Bases>(hb[k], kind_of<T>());
    if (!b[k]) return fail(GS_ERR_ARG, "%s: bad base-array handle for matrix %c", fn, "ABC"[k]);
    if (b[k]->n < o->n) return fail(GS_ERR_SHAPE, "%s: the basis of matrix %c has %zu points, the system %zu rows", fn, "ABC"[k], b[k]->n, o->n);
    terms += o->nnz[k];
  }
  if (terms >= kCsMaxEntries || o->n >= kCsMaxEntries) return fail(GS_ERR_ARG, "%s: %zu terms, at most 2^28 - 1 in one call", fn, terms);
  c.drain();
  PhaseTimer t(c.stream);
  const size_t nvars = o->m, ncnt = nvars + 1;
  const uint32_t gcap = (uint32_t)terms;
  // count, scan: the column pointers (used up as the scatter's cursors)
  DevBuf counts(ncnt * 4), tiles((size_t)scan_tiles(ncnt) * 4), gcnt(8);
  GS_HIP(hipMemsetAsync(counts.p, 0, ncnt * 4, c.stream));
  GS_HIP(hipMemsetAsync(gcnt.p, 0, 8, c.stream));
  for (int k = 0; k < 3; ++k)
    if (b[k] && o->nnz[k])
      hipLaunchKernelGGL(k_cs_count, grid1(o->nnz[k]), dim3(256), 0, c.stream, o->col[k].as<uint32_t>(), o->val[k].as<uint32_t>(), (uint32_t)o->nnz[k], counts.as<uint32_t>());
  scan_exclusive_dev(c, counts.as<uint32_t>(), ncnt, tiles.as<uint32_t>());
  uint32_t nent = 0;
  GS_HIP(hipMemcpyAsync(&nent, counts.as<uint32_t>() + nvars, 4, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
  DevBuf acc(nvars * kPw * 4);
  GS_HIP(hipMemsetAsync(acc.p, 0, nvars * kPw * 4, c.stream));                          // all limbs zero: the point at infinity
  if (nent) {
    // scatter and classify; multiply the general terms
    DevBuf keys((size_t)nent * 4), ent((size_t)nent * 4), gref((size_t)gcap * 4), gmag((size_t)gcap * 36);
    for (int k = 0; k < 3; ++k)
      if (b[k] && o->nnz[k])
        hipLaunchKernelGGL(k_cs_scatter, grid1(o->nnz[k]), dim3(256), 0, c.stream, o->rowptr[k].as<uint32_t>(), o->col[k].as<uint32_t>(), o->val[k].as<uint32_t>(),
                           (uint32_t)o->nnz[k], (uint32_t)o->n, (uint32_t)k, counts.as<uint32_t>(), keys.as<uint32_t>(), ent.as<uint32_t>(), gcnt.as<uint32_t>(), gcap,
                           gref.as<uint32_t>(), gmag.as<uint32_t>());
    GS_HIP(hipGetLastError());
    uint32_t ng[2] = {0, 0};
    GS_HIP(hipMemcpyAsync(ng, gcnt.p, 8, hipMemcpyDeviceToHost, c.stream));
    GS_HIP(hipStreamSynchronize(c.stream));
    DevBuf prod(std::max<size_t>((size_t)ng[0] + ng[1], 1) * kAw * 4);
    CsSources srcs;
    for (int k = 0; k < 3; ++k) srcs.p[k] = b[k] ? b[k]->buf.as<uint32_t>() : nullptr;
    srcs.p[3] = prod.as<uint32_t>();
    if (ng[0]) hipLaunchKernelGGL(k_cs_mul<T>, grid1(ng[0], 64), dim3(64), 0, c.stream, srcs, gref.as<uint32_t>(), gmag.as<uint32_t>(), gcap, false, ng[0],
                                  prod.as<uint32_t>());
    if (ng[1]) hipLaunchKernelGGL(k_cs_mul<T>, grid1(ng[1], 64), dim3(64), 0, c.stream, srcs, gref.as<uint32_t>(), gmag.as<uint32_t>(), gcap, true, ng[1],
                                  prod.as<uint32_t>() + (size_t)ng[0] * kAw);
    GS_HIP(hipGetLastError());
    // the levels of the segmented reduction
    const uint32_t n1 = cs_next_len(nent), n2 = cs_next_len(n1);
    DevBuf pk[2], pp[2];
    pk[0].alloc((size_t)n1 * 4); pp[0].alloc((size_t)n1 * kPw * 4);
    pk[1].alloc((size_t)n2 * 4); pp[1].alloc((size_t)n2 * kPw * 4);
    hipLaunchKernelGGL(k_cs_reduce_first<T>, grid1(cs_chunks(nent), 64), dim3(64), 0, c.stream, keys.as<uint32_t>(), ent.as<uint32_t>(), nent, srcs, ng[0], acc.as<uint32_t>(),
                       pk[0].as<uint32_t>(), pp[0].as<uint32_t>());
    int cur = 0;
    for (uint32_t n = nent; !cs_last_level(n); cur ^= 1) {
      n = cs_next_len(n);                                  // the list the level below left in pk / pp[cur]
      hipLaunchKernelGGL(k_cs_reduce_next<T>, grid1(cs_chunks(n), 64), dim3(64), 0, c.stream, pk[cur].as<uint32_t>(), pp[cur].as<uint32_t>(), n, acc.as<uint32_t>(),
                         pk[cur ^ 1].as<uint32_t>(), pp[cur ^ 1].as<uint32_t>());
    }
    GS_HIP(hipGetLastError());
    GS_HIP(hipStreamSynchronize(c.stream));                // the scratch buffers go here
  }
  std::unique_ptr<Bases> r = std::make_unique<Bases>(kind_of<T>());
  r->n = nvars;
  r->buf.alloc(nvars * kAw * 4);
  hipLaunchKernelGGL(k_ec_to_affine<T>, grid1(nvars), dim3(256), 0, c.stream, acc.as<uint32_t>(), (uint32_t)nvars, r->buf.as<uint32_t>());
  GS_HIP(hipGetLastError());
  t.stop();
  GS_HIP(hipStreamSynchronize(c.stream));
  reset_timing(c);
  c.timing.total_ms = t.ms();
  *out = c.put(std::move(r));
  return GS_OK;
}

// ---- scale, download ---------------------------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(64) k_pt_scale(const uint32_t* __restrict__ in, uint32_t n, Words8 k, int bits, uint32_t* __restrict__ out) {
  constexpr int kAw = PointIO<T>::kAffineWords;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Xyzz<T> r = xyzz_inf<T>();
  if (bits) r = mul_affine_bits<T>(PointIO<T>::load_affine(in + (size_t)i * kAw), k.w, bits);
  PointIO<T>::store_affine(out + (size_t)i * kAw, xyzz_to_affine(r));
}

GS_HD Fe<ModQ, 1> zkey_coord_back_const() {      // 2^256 mod q: mont_mul(x 2^261, 2^256) = x 2^256
  const uint32_t k[NL] = {0x058f0d9du, 0x1aea1c6eu, 0x11c2cf74u, 0x11d651ebu, 0x1462c0a7u, 0x11b7bc3cu, 0x1cbd99bau, 0x183340fbu, 0x000e0a77u};
  Fe<ModQ, 1> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = k[i];
  return r;
}
// the engine's packed affine points -> the .zkey encoding, coordinate by coordinate (zero stays zero: infinity is all-zero in both)
__global__ void __launch_bounds__(256) k_coords_to_zkey(const uint32_t* __restrict__ in, size_t ncoords, uint32_t* __restrict__ out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ncoords) return;
  uint32_t w[8];
  pack32<ModQ>(canon(mul(load_fq(in + i * 8), zkey_coord_back_const())), w);
#pragma unroll
  for (int j = 0; j < 8; ++j) out[i * 8 + j] = w[j];
}

template <class T>
int download_affine_mont_impl(Ctx& c, const char* fn, gs_handle h, void* bytes, size_t n) {
  constexpr size_t kPointBytes = PointIO<T>::kAffineWords * 4;
  Bases* b = c.get<Bases>(h, kind_of<T>());
  if (!b) return fail(GS_ERR_ARG, "%s: bad base-array handle", fn);
  if (n && !bytes) return fail(GS_ERR_ARG, "%s: null argument", fn);
  if (n > b->n) return fail(GS_ERR_SHAPE, "%s: the array has %zu points, %zu were asked for", fn, b->n, n);
  if (!n) return GS_OK;
  c.drain();
  DevBuf tmp(n * kPointBytes);
  hipLaunchKernelGGL(k_coords_to_zkey, grid1(n * kPointBytes / 32), dim3(256), 0, c.stream, b->buf.as<uint32_t>(), n * kPointBytes / 32, tmp.as<uint32_t>());
  GS_HIP(hipGetLastError());
  // the caller's bytes may be a memory-mapped file: they are written by memcpy from a pinned buffer, never by the DMA engine
  const size_t piece = std::min<size_t>(n * kPointBytes, (size_t)8 << 20);
  void* pin = nullptr;
  GS_HIP(hipHostMalloc(&pin, piece, hipHostMallocDefault));
  hipError_t e = hipSuccess;
  for (size_t off = 0; off < n * kPointBytes && e == hipSuccess; off += piece) {
    const size_t len = std::min(piece, n * kPointBytes - off);
    e = hipMemcpyAsync(pin, tmp.as<char>() + off, len, hipMemcpyDeviceToHost, c.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
    if (e == hipSuccess) memcpy(static_cast<char*>(bytes) + off, pin, len);
  }
  (void)hipHostFree(pin);
  GS_HIP(e);
  return GS_OK;
}

}  // namespace

extern "C" {

int gs_g1_lagrange(gs_handle powers, size_t off, size_t log2_n, int odd_half, gs_handle* out) {
  return guarded([&](Ctx& c) -> int { return lagrange_impl<FqTag>(c, "gs_g1_lagrange", powers, off, log2_n, odd_half, out); }, true, false, powers);
}
int gs_g2_lagrange(gs_handle powers, size_t off, size_t log2_n, gs_handle* out) {
  return guarded([&](Ctx& c) -> int { return lagrange_impl<Fq2Tag>(c, "gs_g2_lagrange", powers, off, log2_n, 0, out); }, true, false, powers);
}

int gs_r1cs_colsum_g1(gs_handle r1cs, gs_handle basis_a, gs_handle basis_b, gs_handle basis_c, gs_handle* out) {
  const gs_handle hb[3] = {basis_a, basis_b, basis_c};
  return guarded([&](Ctx& c) -> int { return colsum_impl<FqTag>(c, "gs_r1cs_colsum_g1", r1cs, hb, out); }, true, false, r1cs);
}
int gs_r1cs_colsum_g2(gs_handle r1cs, gs_handle basis_a, gs_handle basis_b, gs_handle basis_c, gs_handle* out) {
  const gs_handle hb[3] = {basis_a, basis_b, basis_c};
  return guarded([&](Ctx& c) -> int { return colsum_impl<Fq2Tag>(c, "gs_r1cs_colsum_g2", r1cs, hb, out); }, true, false, r1cs);
}

int gs_g1_scale(gs_handle bases, const uint64_t k[4], gs_handle* out) {
  return guarded([&](Ctx& c) -> int {
    const char* fn = "gs_g1_scale";
    Bases* b = c.get<Bases>(bases, Kind::G1Bases);
    if (!b || !out) return fail(GS_ERR_ARG, "%s: bad base-array handle", fn);
    if (!k) return fail(GS_ERR_ARG, "%s: null argument", fn);
    Words8 kw;
    for (int i = 0; i < 4; ++i) { kw.w[2 * i] = (uint32_t)k[i]; kw.w[2 * i + 1] = (uint32_t)(k[i] >> 32); }
    cs_canon(kw.w);
    c.drain();
    auto r = std::make_unique<Bases>(Kind::G1Bases);
    r->n = b->n;
    r->buf.alloc(std::max<size_t>(b->n, 1) * 64);
    if (b->n) hipLaunchKernelGGL(k_pt_scale<FqTag>, grid1(b->n, 64), dim3(64), 0, c.stream, b->buf.as<uint32_t>(), (uint32_t)b->n, kw, cs_bitlen(kw.w), r->buf.as<uint32_t>());
    GS_HIP(hipGetLastError());
    GS_HIP(hipStreamSynchronize(c.stream));
    *out = c.put(std::move(r));
    return GS_OK;
  }, true, false, bases);
}

int gs_g1_download_affine_mont(gs_handle bases, void* bytes, size_t n) {
  return guarded([&](Ctx& c) -> int { return download_affine_mont_impl<FqTag>(c, "gs_g1_download_affine_mont", bases, bytes, n); }, true, false, bases);
}
int gs_g2_download_affine_mont(gs_handle bases, void* bytes, size_t n) {
  return guarded([&](Ctx& c) -> int { return download_affine_mont_impl<Fq2Tag>(c, "gs_g2_download_affine_mont", bases, bytes, n); }, true, false, bases);
}

}  // extern "C"
