// Window-table builders for gfx950 (G1 and G2 via the field tag T), launched by tables.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ec.h"
#include "point_io.h"

namespace gs {

// ---- window tables ----------------------------------------------------------------------------------------
// rows[j][i] = 2^(c j) * P_i for j < W, packed affine.  Built once per (base array, c) and kept in HBM: a
// 2^20-point G1 array costs 64 MiB per row, 1 GiB for c = 16 -- the trade the 288 GB of HBM3E is there for.
template <class T>
__global__ void __launch_bounds__(256) k_build_table(const uint32_t* __restrict__ row0, uint32_t n, int c, int W, uint32_t* __restrict__ rows) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  constexpr int aw = PointIO<T>::kAffineWords;
  Affine<T> a = PointIO<T>::load_affine(row0 + (size_t)i * aw);
  if (rows != row0) PointIO<T>::store_affine(rows + (size_t)i * aw, a);
  for (int j = 1; j < W; ++j) {
    if (!is_inf(a)) {
      Xyzz<T> x = xyzz_dbl_affine<T>(a.x, relax<2>(a.y));
      for (int k = 1; k < c; ++k) xyzz_dbl(x);
      a = xyzz_to_affine(x);
    }
    PointIO<T>::store_affine(rows + ((size_t)j * n + i) * aw, a);
  }
}

// The same table with ONE field inversion per point instead of one per row (Montgomery's trick along the rows of a
// point): the forward sweep keeps doubling in XYZZ and parks every row's point and the running product of the ZZZ's in
// a scratch slab, the backward sweep peels the individual inverses off the inverted product and writes the affine rows.
// ~2000 field products per point instead of ~6000 (15 Fermat inversions cost more than the 240 doublings).
// Points that reach infinity while doubling (only possible outside the order-r subgroup) take the per-row path above.
template <class T>
__global__ void __launch_bounds__(256) k_build_table_batched(const uint32_t* __restrict__ row0, uint32_t n, uint32_t first, uint32_t count, int c, int W,
                                                              uint32_t* __restrict__ rows, uint32_t* __restrict__ scratch) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= count) return;
  const uint32_t i = first + t;
  constexpr int aw = PointIO<T>::kAffineWords, pw = PointIO<T>::kXyzzWords, ew = pw / 4, sw = pw + ew;
  using E2 = typename T::template E<2>;
  Affine<T> a = PointIO<T>::load_affine(row0 + (size_t)i * aw);
  if (rows != row0) PointIO<T>::store_affine(rows + (size_t)i * aw, a);
  if (W <= 1) return;
  if (is_inf(a)) {
    for (int j = 1; j < W; ++j) PointIO<T>::store_affine(rows + ((size_t)j * n + i) * aw, a);
    return;
  }
  // Round 6: JACOBIAN doublings (ec.h, jac_dbl: 3M + 4S = 990 multiply-adds against the XYZZ doubling's 1350) -- a table row is 14 x 17
  // doublings of one point and never an addition; per row the point is parked as (X, Y, Z) with the running product of the Z's, one
  // inversion per point turns all rows affine (x = X / Z^2, y = Y / Z^3).
  constexpr int cw = pw / 4;                                     // words per coordinate; a parked row = X | Y | Z | prefix (4 of the sw = 5 cw)
  Jac<T> x = jac_from_affine<T>(a);
  for (int k = 0; k < c; ++k) jac_dbl(x);
  bool degenerate = is_inf(x);
  E2 pref = reduce2(x.z);
  auto park = [&](int j) {
    uint32_t* s = scratch + ((size_t)(j - 1) * count + t) * sw;
    PointIO<T>::store_limbs(s, x.x); PointIO<T>::store_limbs(s + cw, x.y); PointIO<T>::store_limbs(s + 2 * cw, x.z);
    PointIO<T>::store_limbs(s + 3 * cw, pref);
  };
  park(1);
  for (int j = 2; j < W && !degenerate; ++j) {
    for (int k = 0; k < c; ++k) jac_dbl(x);
    degenerate = is_inf(x);
    pref = smul<T>(pref, x.z);
    park(j);
  }
  if (degenerate) {                                             // rare: redo this point row by row
    for (int j = 1; j < W; ++j) {
      if (!is_inf(a)) {
        Xyzz<T> y = xyzz_dbl_affine<T>(a.x, relax<2>(a.y));
        for (int k = 1; k < c; ++k) xyzz_dbl(y);
        a = xyzz_to_affine(y);
      }
      PointIO<T>::store_affine(rows + ((size_t)j * n + i) * aw, a);
    }
    return;
  }
  E2 itot = inv(pref);                                          // 1 / (Z_1 ... Z_{W-1})
  for (int j = W - 1; j >= 1; --j) {
    const uint32_t* s = scratch + ((size_t)(j - 1) * count + t) * sw;
    Jac<T> xj;
    PointIO<T>::load_limbs(s, xj.x); PointIO<T>::load_limbs(s + cw, xj.y); PointIO<T>::load_limbs(s + 2 * cw, xj.z);
    E2 iz = itot;                                               // 1 / Z_j
    if (j > 1) {
      E2 before;
      PointIO<T>::load_limbs(scratch + ((size_t)(j - 2) * count + t) * sw + 3 * cw, before);
      iz = smul<T>(itot, before);
      itot = smul<T>(itot, xj.z);
    }
    PointIO<T>::store_affine(rows + ((size_t)j * n + i) * aw, jac_to_affine_with_inverse<T>(xj, iz));
  }
}

}  // namespace gs
