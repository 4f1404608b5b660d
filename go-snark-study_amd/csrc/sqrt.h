// Square roots in Fq and Fq2 = Fq[u]/(u^2 + 1), and the sign rule of compressed points: the same __host__ __device__ source for the
// kernels of point_codec.hip and for the host test (tests/host/sqrt_host_test.hip).
//
// q = 3 mod 4, so a residue a has the root a^((q+1)/4) and a non-residue has none: no Tonelli-Shanks, no loop whose length depends on a
// value.  Both exponents used here -- (q+1)/4 and (q-3)/4, the inverse of that root -- are constants of 252 bits (bn128_constants.h,
// tools/gen_constants.py) scanned as 84 digits of 3 bits over a table a .. a^7: 249 squarings, 6 products for the table and one product
// per non-zero digit below the top one (68, for either exponent): 323 field products.  The digit is the same in every lane of a wave,
// so the skipped product of a zero digit is a scalar branch and the table is read with selects on a uniform condition: 7 x 9 registers,
// no indexed memory.  (4-bit digits: 318 products and 15 x 9 registers.)
//
// Fq2, the complex method: for a = a0 + a1 u with norm n = a0^2 + a1^2 and s = sqrt(n), a root is x0 + x1 u with x0^2 = (a0 + s)/2 and
// x1 = a1 / (2 x0) -- or with x1^2 = (s - a0)/2: the product of the two candidates t = (a0 + s)/2 and (a0 - s)/2 is -a1^2/4 and -1 is a
// non-residue, so exactly one of them is a residue.  One exponentiation decides which AND inverts: w = t^((q-3)/4), z = w t, chi = w z
// = t^((q-1)/2).  chi = 1: z^2 = t and w = 1/z, the root is (z, a1 w / 2).  chi = -1: z^2 = -t and w = -1/z, the root is
// (-a1 w / 2, z).  With a1 = 0 the candidate is t = a0 itself: (sqrt(a0), 0) for a residue, (0, sqrt(-a0)) else -- the same
// two formulas.  a = 0 gives t = w = z = 0 and the root 0.  Two Fq exponentiations, no inversion, no branch on a value: which of the
// formulas applies is a select.  Whether the result IS a root is decided by squaring it, never by an intermediate.
#pragma once
#include "fq2.h"

namespace gs {

enum : int { kSqrtExpRoot = 0, kSqrtExpInv = 1 };      // (q+1)/4 | (q-3)/4

// 3-bit digit i (0 = least significant) of one of the two exponents
template <int kWhich> GS_HD uint32_t sqrt_exp_digit(int i) {
  const int bit = 3 * i, wi = bit >> 5, sh = bit & 31;
  uint64_t v = kWhich == kSqrtExpRoot ? Gen::sqrt_root32(wi) : Gen::sqrt_inv32(wi);
  if (wi + 1 < 8) v |= (uint64_t)(kWhich == kSqrtExpRoot ? Gen::sqrt_root32(wi + 1) : Gen::sqrt_inv32(wi + 1)) << 32;
  return (uint32_t)(v >> sh) & 7u;
}

// tab[d - 1] for d = 1 .. 7 by selects; d is uniform over a wave
GS_HD Fe<ModQ, 2> sqrt_table_pick(const Fe<ModQ, 2> (&tab)[7], uint32_t d) {
  Fe<ModQ, 2> r = tab[0];
#pragma unroll
  for (int j = 1; j < 7; ++j) r = select(d == (uint32_t)(j + 1), tab[j], r);
  return r;
}

// a^((q+1)/4) or a^((q-3)/4), Montgomery form in and out
template <int kWhich> GS_HD Fe<ModQ, 2> fq_pow_sqrt_exp(const Fe<ModQ, 2>& a) {
  Fe<ModQ, 2> tab[7];
  tab[0] = a;
  tab[1] = sqr(a);
  tab[2] = mul(tab[1], a);
  tab[3] = sqr(tab[1]);
  tab[4] = mul(tab[3], a);
  tab[5] = sqr(tab[2]);
  tab[6] = mul(tab[5], a);
  Fe<ModQ, 2> acc = sqrt_table_pick(tab, sqrt_exp_digit<kWhich>(Gen::kSqrtDigits - 1));      // the top digit is not zero
#pragma unroll 1
  for (int i = Gen::kSqrtDigits - 2; i >= 0; --i) {
    acc = sqr(sqr(sqr(acc)));
    const uint32_t d = sqrt_exp_digit<kWhich>(i);
    if (d) acc = mul(acc, sqrt_table_pick(tab, d));
  }
  return acc;
}

// y = a^((q+1)/4); true when y^2 = a (a is zero or a residue), else y is no root of anything the caller wants
GS_HD bool fq_sqrt(const Fe<ModQ, 2>& a, Fe<ModQ, 2>& y) {
  y = fq_pow_sqrt_exp<kSqrtExpRoot>(a);
  return is_zero(sub(sqr(y), a));
}

GS_HD Fe<ModQ, 1> fq_half() {      // 1/2, Montgomery form
  Fe<ModQ, 1> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = Gen::half(i);
  return r;
}

GS_HD bool fq2_sqrt(const Fq2e<2>& a, Fq2e<2>& y) {
  const Fe<ModQ, 2> n = mul_add(a.c0, a.c0, a.c1, a.c1);
  const Fe<ModQ, 2> s = fq_pow_sqrt_exp<kSqrtExpRoot>(n);
  const Fe<ModQ, 1> half = fq_half();
  const Fe<ModQ, 2> t = select(is_zero(a.c1), a.c0, mul(add(a.c0, s), half));
  const Fe<ModQ, 2> w = fq_pow_sqrt_exp<kSqrtExpInv>(t);
  const Fe<ModQ, 2> z = mul(w, t);
  const bool residue = is_zero(sub(mul(w, z), fe_one<ModQ>()));      // chi = 1; chi = 0 (a = 0) takes the other formula, which gives 0 too
  const Fe<ModQ, 2> v = mul(mul(a.c1, w), half);
  y.c0 = select(residue, z, reduce2(neg(v)));
  y.c1 = select(residue, v, z);
  return is_zero(sub(sqr(y), a));
}

// ---- the sign of a root: y is the LARGER of {y, -y} as canonical integers, i.e. y > (q-1)/2; in Fq2 by c1, by c0 only when c1 = 0 ----
GS_HD bool fq_std_above_half(const Fe<ModQ, 1>& a /* standard form, canonical, fully normalised */) {
  bool gt = false, eq = true;
#pragma unroll
  for (int i = NL - 1; i >= 0; --i) {
    gt = gt || (eq && a.l[i] > Gen::qhalf(i));
    eq = eq && a.l[i] == Gen::qhalf(i);
  }
  return gt;
}
template <int B> GS_HD bool fq_is_largest(const Fe<ModQ, B>& y /* Montgomery form */) { return fq_std_above_half(from_mont(y)); }
template <int B> GS_HD bool fq2_is_largest(const Fq2e<B>& y) {
  const Fe<ModQ, 1> c1 = from_mont(y.c1);
  uint32_t o = 0;
#pragma unroll
  for (int i = 0; i < NL; ++i) o |= c1.l[i];
  return fq_std_above_half(o ? c1 : from_mont(y.c0));
}

}  // namespace gs
