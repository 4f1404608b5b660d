// Raw-limb op table for the limit tests: every field / curve primitive of csrc/fp29.h, fq2.h and ec.h instantiated at the bounds
// of its real call sites and at the largest bounds its static checks admit, fed RAW limbs (no to_mont on the way in, no from_mont /
// canon / carry on the way out), so that operands can sit at the edge of what their types allow: low limbs at kNearlyNormalMax - 1, values at
// B p - 1, un-carried lazy limbs.  ONE table, two builds: tests/host/fp_limits_host_test.hip (CPU, tests/test_limits_host.py) and
// tests/device/prim_test.hip (gs_prim_run_raw, tests/test_gpu_primitives.py); tests/limits_util.py reads the LIMIT_OP(id, name)
// lines below for the op ids, takes the operand bounds from the digits of the name (base__B0_B1_...) and checks them against the
// bounds get<>() echoes back.
//
// Record layout (uint32 words).  Fields (kind 0 = q, 1 = r, 2 = Fq2 over q): in = 8 slots x 9 limbs; out = 4 slots x 9 limbs, then
// 8 words: the compile-time value bound the op read slot s with (0: slot unused).  An Fq2 element takes two adjacent slots (c0, c1).
// Points (kind 3 = G1, 4 = G2): in = accumulator [x | y | zz | zzz] then second operand [x | y | zz | zzz] (an affine operand fills
// x and y), out = [x | y | zz | zzz]; 9 words per coordinate for G1, 18 (c0, c1) for G2.
#pragma once
#include <stdint.h>

#include "../../go-snark-study_amd/csrc/ec.h"

namespace gs {
namespace limits {

constexpr int kInSlots = 8, kOutSlots = 4;
constexpr int kFieldIn = kInSlots * NL, kFieldOut = kOutSlots * NL + kInSlots;
GS_HD constexpr int in_words(int kind) { return kind < 3 ? kFieldIn : kind == 3 ? 8 * NL : 16 * NL; }
GS_HD constexpr int out_words(int kind) { return kind < 3 ? kFieldOut : kind == 3 ? 4 * NL : 8 * NL; }

struct Io {
  const uint32_t* in;
  uint32_t* out;
};
template <class M, int B>
GS_HD Fe<M, B> get(const Io& io, int slot) {
  Fe<M, B> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = io.in[slot * NL + i];
  io.out[kOutSlots * NL + slot] = B;
  return r;
}
template <int B>
GS_HD Fq2e<B> get2(const Io& io, int elem) { return {get<ModQ, B>(io, 2 * elem), get<ModQ, B>(io, 2 * elem + 1)}; }
template <class X>
GS_HD void put(const Io& io, int slot, const X& x) {       // Fe or Lz, as it is
#pragma unroll
  for (int i = 0; i < NL; ++i) io.out[slot * NL + i] = x.l[i];
}
template <int B>
GS_HD void put2(const Io& io, int elem, const Fq2e<B>& x) { put(io, 2 * elem, x.c0); put(io, 2 * elem + 1, x.c1); }
GS_HD void put_flag(const Io& io, int slot, bool f) { io.out[slot * NL] = f ? 1u : 0u; }

// neg_lazy<B> and sub_lazy<2, B> at EVERY B the tables admit (op ids 100 + B and 200 + B): the result's value bound is
// tbias_k(B + 1), which differs from B + 1 wherever (B + 1) p has a low limb below 16
template <class M, int B = 1>
GS_HD void neg_lazy_at(const Io& io, int b) {
  if constexpr (B + 1 <= M::kMaxBiasK) {
    if (b == B) { put(io, 0, neg_lazy(get<M, B>(io, 0))); return; }
    neg_lazy_at<M, B + 1>(io, b);
  }
}
template <class M, int B = 1>
GS_HD void sub_lazy_at(const Io& io, int b) {
  if constexpr (B + 1 <= M::kMaxBiasK) {
    if constexpr (2 + M::tbias_k(B + 1) <= M::kMaxBiasK) {
      if (b == B) { put(io, 0, sub_lazy(get<M, 2>(io, 0), get<M, B>(io, 1))); return; }
    }
    sub_lazy_at<M, B + 1>(io, b);
  }
}

#define LIMIT_OP(id, name) case id:
#define A(B) get<M, B>(io, 0)
#define Bq(B) get<M, B>(io, 1)
#define C(B) get<M, B>(io, 2)
#define D(B) get<M, B>(io, 3)
#define S(s, B) get<M, B>(io, s)

template <class M>
GS_HD void field_op(int op, const Io& io) {
  Fe<M, 2> r0, r1, r2;
  switch (op) {
    LIMIT_OP(0, tables) {                                      // bias / tbias / wbias rows of k = in[0]; tbias_k(k), kTopLimb, kMaxBiasK, kNearlyNormalMax
      const int k = (int)(io.in[0] & 63u);
      for (int i = 0; i < NL; ++i) {
        io.out[i] = M::bias(k, i); io.out[NL + i] = M::tbias(k, i); io.out[2 * NL + i] = M::wbias(k, i);
      }
      io.out[3 * NL] = (uint32_t)M::tbias_k(k); io.out[3 * NL + 1] = M::kTopLimb; io.out[3 * NL + 2] = (uint32_t)M::kMaxBiasK;
      io.out[3 * NL + 3] = (uint32_t)kNearlyNormalMax;
      break;
    }
    // ---- carry / bias ops: call sites, then the table edge (result bound kMaxBiasK = 40)
    LIMIT_OP(1, add__2_2) put(io, 0, add(A(2), Bq(2))); break;
    LIMIT_OP(2, add__20_20) put(io, 0, add(A(20), Bq(20))); break;
    LIMIT_OP(3, dbl__2) put(io, 0, dbl(A(2))); break;
    LIMIT_OP(4, dbl__20) put(io, 0, dbl(A(20))); break;
    LIMIT_OP(5, sub__2_2) put(io, 0, sub(A(2), Bq(2))); break;
    LIMIT_OP(6, sub__2_10) put(io, 0, sub(A(2), Bq(10))); break;
    LIMIT_OP(7, sub__19_20) put(io, 0, sub(A(19), Bq(20))); break;
    LIMIT_OP(8, neg__2) put(io, 0, neg(A(2))); break;
    LIMIT_OP(9, neg__5) put(io, 0, neg(A(5))); break;
    LIMIT_OP(10, neg__39) put(io, 0, neg(A(39))); break;
    LIMIT_OP(11, sub_ripple__2_9) put(io, 0, sub_ripple(A(2), Bq(9))); break;
    LIMIT_OP(12, sub_ripple__2_5) put(io, 0, sub_ripple(A(2), Bq(5))); break;
    LIMIT_OP(13, sub_ripple__2_2) put(io, 0, sub_ripple(A(2), Bq(2))); break;
    LIMIT_OP(14, sub_ripple__19_20) put(io, 0, sub_ripple(A(19), Bq(20))); break;
    LIMIT_OP(15, sub_b_2c__2_2_2) put(io, 0, sub_b_2c(A(2), Bq(2), C(2))); break;
    LIMIT_OP(16, sub_b_2c__9_10_10) put(io, 0, sub_b_2c(A(9), Bq(10), C(10))); break;
    LIMIT_OP(17, add_lazy__2_2) put(io, 0, add_lazy(A(2), Bq(2))); break;
    LIMIT_OP(18, add_lazy__20_20) put(io, 0, add_lazy(A(20), Bq(20))); break;
    LIMIT_OP(19, dbl_lazy__2) put(io, 0, dbl_lazy(A(2))); break;
    LIMIT_OP(20, dbl_lazy__20) put(io, 0, dbl_lazy(A(20))); break;
    LIMIT_OP(21, sub_lazy__19_20) put(io, 0, sub_lazy(A(19), Bq(20))); break;
    LIMIT_OP(22, normalize_sub_lazy__2_9) put(io, 0, normalize(sub_lazy(A(2), Bq(9)))); break;
    LIMIT_OP(23, normalize_add_lazy__20_20) put(io, 0, normalize(add_lazy(A(20), Bq(20)))); break;
    LIMIT_OP(24, normalize_neg_lazy__5) put(io, 0, normalize(neg_lazy(A(5)))); break;
    LIMIT_OP(25, normalize_dbl_lazy__20) put(io, 0, normalize(dbl_lazy(A(20)))); break;
    // ---- reductions / comparisons
    LIMIT_OP(30, reduce2__2) put(io, 0, reduce2(A(2))); break;
    LIMIT_OP(31, reduce2__5) put(io, 0, reduce2(A(5))); break;
    LIMIT_OP(32, reduce2__8) put(io, 0, reduce2(A(8))); break;
    LIMIT_OP(33, reduce2__12) put(io, 0, reduce2(A(12))); break;
    LIMIT_OP(34, reduce2__19) put(io, 0, reduce2(A(19))); break;
    LIMIT_OP(35, reduce2__40) put(io, 0, reduce2(A(40))); break;
    LIMIT_OP(36, reduce2_normal__2) put(io, 0, reduce2_normal(A(2))); break;
    LIMIT_OP(37, reduce2_normal__5) put(io, 0, reduce2_normal(A(5))); break;
    LIMIT_OP(38, reduce2_normal__8) put(io, 0, reduce2_normal(A(8))); break;
    LIMIT_OP(39, reduce2_normal__12) put(io, 0, reduce2_normal(A(12))); break;
    LIMIT_OP(40, reduce2_normal__19) put(io, 0, reduce2_normal(A(19))); break;
    LIMIT_OP(41, reduce2_normal__40) put(io, 0, reduce2_normal(A(40))); break;
    LIMIT_OP(42, canon__2) put(io, 0, canon(A(2))); break;
    LIMIT_OP(43, canon__5) put(io, 0, canon(A(5))); break;
    LIMIT_OP(44, canon__8) put(io, 0, canon(A(8))); break;
    LIMIT_OP(45, canon__12) put(io, 0, canon(A(12))); break;
    LIMIT_OP(46, canon__19) put(io, 0, canon(A(19))); break;
    LIMIT_OP(47, canon__40) put(io, 0, canon(A(40))); break;
    LIMIT_OP(48, is_zero__5) { const auto a = A(5); put_flag(io, 0, is_zero(a)); put_flag(io, 1, maybe_zero(a)); break; }
    LIMIT_OP(49, is_zero__8) { const auto a = A(8); put_flag(io, 0, is_zero(a)); put_flag(io, 1, maybe_zero(a)); break; }
    LIMIT_OP(50, is_zero__12) { const auto a = A(12); put_flag(io, 0, is_zero(a)); put_flag(io, 1, maybe_zero(a)); break; }
    LIMIT_OP(51, equal__2_2) put_flag(io, 0, equal(A(2), Bq(2))); break;
    LIMIT_OP(52, equal__2_5) put_flag(io, 0, equal(A(2), Bq(5))); break;
    LIMIT_OP(53, equal__5_6) put_flag(io, 0, equal(A(5), Bq(6))); break;
    // ---- Montgomery products: call-site bounds, then the value-bound maximum (sum of Ba Bb in 157..160)
    LIMIT_OP(60, mul__2_2) put(io, 0, mul(A(2), Bq(2))); break;
    LIMIT_OP(61, mul__12_13) put(io, 0, mul(A(12), Bq(13))); break;
    LIMIT_OP(62, mul__40_4) put(io, 0, mul(A(40), Bq(4))); break;
    LIMIT_OP(63, mul__4_40) put(io, 0, mul(A(4), Bq(40))); break;
    LIMIT_OP(64, sqr__2) put(io, 0, sqr(A(2))); break;
    LIMIT_OP(65, sqr__12) put(io, 0, sqr(A(12))); break;
    LIMIT_OP(66, mul_add__2_2_2_2) put(io, 0, mul_add(A(2), Bq(2), C(2), D(2))); break;
    LIMIT_OP(67, mul_add__12_12_4_4) put(io, 0, mul_add(A(12), Bq(12), C(4), D(4))); break;
    LIMIT_OP(68, mul_add__8_10_8_10) put(io, 0, mul_add(A(8), Bq(10), C(8), D(10))); break;
    LIMIT_OP(69, dot4__2_2_2_2_2_2_2_2) put(io, 0, dot4(A(2), Bq(2), C(2), D(2), S(4, 2), S(5, 2), S(6, 2), S(7, 2))); break;
    LIMIT_OP(70, dot4__12_13_1_1_1_1_1_1) put(io, 0, dot4(A(12), Bq(13), C(1), D(1), S(4, 1), S(5, 1), S(6, 1), S(7, 1))); break;   // 159
    LIMIT_OP(71, dot4__6_10_5_10_5_5_5_5) put(io, 0, dot4(A(6), Bq(10), C(5), D(10), S(4, 5), S(5, 5), S(6, 5), S(7, 5))); break;   // 160
    LIMIT_OP(72, mul_sub__2_2_2_2) put(io, 0, mul_sub(A(2), Bq(2), C(2), D(2))); break;
    LIMIT_OP(73, mul_sub__12_12_3_4) put(io, 0, mul_sub(A(12), Bq(12), C(3), D(4))); break;                                      // 144 + 4 x 4
    LIMIT_OP(74, inv__2) put(io, 0, inv(A(2))); break;
    LIMIT_OP(75, inv__12) put(io, 0, inv(A(12))); break;
    LIMIT_OP(76, sqr2__2_2) sqr2(A(2), Bq(2), r0, r1); put(io, 0, r0); put(io, 1, r1); break;
    LIMIT_OP(77, sqr2__12_8) sqr2(A(12), Bq(8), r0, r1); put(io, 0, r0); put(io, 1, r1); break;                                  // P | R of the G1 mixed addition
    LIMIT_OP(78, sqr2__12_12) sqr2(A(12), Bq(12), r0, r1); put(io, 0, r0); put(io, 1, r1); break;
    // ---- lazy operands: the limb-weight maximum column_fits admits is 6 (one W3 x W2 term, or 1 + 2 + 2 + 1 over four terms)
    LIMIT_OP(80, mul_lazy_w3w2__2_9_5) put(io, 0, mul_lazy(sub_lazy(A(2), Bq(9)), neg_lazy(C(5)))); break;
    LIMIT_OP(81, mul_lazy_w2w3__2_9_5) put(io, 0, mul_lazy(neg_lazy(C(5)), sub_lazy(A(2), Bq(9)))); break;
    LIMIT_OP(82, mul_lazy_w3fe__2_37_4) put(io, 0, mul_lazy(sub_lazy(A(2), Bq(37)), C(4))); break;                               // 40 x 4
    LIMIT_OP(83, mul_lazy_w2w2__6_6_6) put(io, 0, mul_lazy(add_lazy(A(6), Bq(6)), dbl_lazy(C(6)))); break;                       // 12 x 12
    LIMIT_OP(84, dots2__12_13_2_2_40_4) dots2<M>(dot_of(A(12), Bq(13), C(2), D(2)), dot_of(S(4, 40), S(5, 4)), r0, r1); put(io, 0, r0); put(io, 1, r1); break;
    LIMIT_OP(85, dots3__12_12_4_4_12_13_40_4)
      dots3<M>(dot_of(A(12), Bq(12), C(4), D(4)), dot_of(S(4, 12), S(5, 13)), dot_of(S(6, 40), S(7, 4)), r0, r1, r2);
      put(io, 0, r0); put(io, 1, r1); put(io, 2, r2); break;
    LIMIT_OP(86, chains_fq2_sqr__6_6) {                          // the Fq2 square's two chains: (W2 x W3) | (W2 x Fe), 12 x 13 = 156
      const auto a = A(6), b = Bq(6);
      dots2<M>(dot_of(add_lazy(a, b), sub_lazy(a, b)), dot_of(dbl_lazy(a), b), r0, r1); put(io, 0, r0); put(io, 1, r1); break;
    }
    LIMIT_OP(87, chains_fq2_mul_sub__6_6_12_12_1_1_1_1) {        // the four-term chains of the Fq2 mul_sub at (6, 12, 1, 1): weights 1 + 2 + 2 + 1
      const auto a0 = A(6), a1 = Bq(6); const auto b0 = C(12), b1 = D(12); const auto c0 = S(4, 1), c1 = S(5, 1), d0 = S(6, 1), d1 = S(7, 1);
      const auto na1 = neg_lazy(a1); const auto nc0 = neg_lazy(c0), nc1 = neg_lazy(c1);
      dots2<M>(dot_of(a0, b0, na1, b1, nc0, d0, c1, d1), dot_of(a0, b1, a1, b0, nc0, d1, nc1, d0), r0, r1); put(io, 0, r0); put(io, 1, r1); break;
    }
    LIMIT_OP(88, dots_uniform_4_1__6_6_6_6) {                    // two Fq2 squares side by side (fq2.h sqr2)
      const auto a = A(6), b = Bq(6), c = C(6), d = D(6);
      const auto sa = add_lazy(a, b), sb = add_lazy(c, d); const auto da = sub_lazy(a, b), db = sub_lazy(c, d);
      const auto ta = dbl_lazy(a), tb = dbl_lazy(c);
      const Dot<1> ch[4] = {dot_of(sa, da), dot_of(ta, b), dot_of(sb, db), dot_of(tb, d)};
      Fe<M, 2> r[4];
      dots_uniform<M, 4, 1>(ch, r);
      for (int c4 = 0; c4 < 4; ++c4) put(io, c4, r[c4]);
      break;
    }
    LIMIT_OP(89, dots_uniform_4_2__8_8_9_9_9_9_8_8) {            // two Fq2 products side by side (fq2.h mul2)
      const auto a0 = A(8), a1 = Bq(8), d0 = S(6, 8), d1 = S(7, 8); const auto b0 = C(9), b1 = D(9), c0 = S(4, 9), c1 = S(5, 9);
      const auto nb1 = neg_lazy(b1); const auto nd1 = neg_lazy(d1);
      const Dot<2> ch[4] = {dot_of(a0, b0, a1, nb1), dot_of(a0, b1, a1, b0), dot_of(c0, d0, c1, nd1), dot_of(c0, d1, c1, d0)};
      Fe<M, 2> r[4];
      dots_uniform<M, 4, 2>(ch, r);
      for (int c4 = 0; c4 < 4; ++c4) put(io, c4, r[c4]);
      break;
    }
    // ---- the exact compositions of xyzz_madd_g1 (ec.h), operands at the accumulator's bounds
    LIMIT_OP(90, madd_ppp_q__12_2_9) { const auto PP = Bq(2); dots2<M>(dot_of(A(12), PP), dot_of(C(9), PP), r0, r1); put(io, 0, r0); put(io, 1, r1); break; }
    LIMIT_OP(91, madd_y3__8_2_9_5_2_2_2_2) {                     // slots: R Q X3 y PPP zz PP zzz -> Y3 ZZ3 ZZZ3
      const auto R = A(8); const auto PPP = S(4, 2), PP = S(6, 2);
      const auto Dl = sub_lazy(Bq(2), C(9));
      const auto ny = neg_lazy(D(5));
      dots3<M>(dot_of(R, Dl, ny, PPP), dot_of(S(5, 2), PP), dot_of(S(7, 2), PPP), r0, r1, r2);
      put(io, 0, r0); put(io, 1, r1); put(io, 2, r2); break;
    }
    default:
      if (op > 100 && op < 100 + M::kMaxBiasK) neg_lazy_at<M>(io, op - 100);
      else if (op > 200 && op < 200 + M::kMaxBiasK) sub_lazy_at<M>(io, op - 200);
      break;
  }
}

// U2 | S2 of xyzz_madd_g1 with its own y2 (the select needs tbias_k(2) == 2: q only).  slots: b.x zz b.y zzz
GS_HD void madd_u2s2(const Io& io, bool negate) {
  using M = ModQ;
  const auto by = C(1);
  const auto y2 = select(negate, neg_lazy(by), widen<2>(as_lazy(relax<2>(by))));
  Fe<M, 2> U2, S2;
  dots2<M>(dot_of(A(1), Bq(2)), dot_of(y2, D(2)), U2, S2);
  put(io, 0, U2); put(io, 1, S2);
}
#undef A
#undef Bq
#undef C
#undef D
#undef S

GS_HD void q_only_op(int op, const Io& io) {
  switch (op) {
    LIMIT_OP(92, madd_u2s2__1_2_1_2) madd_u2s2(io, false); break;
    LIMIT_OP(93, madd_u2s2_negate__1_2_1_2) madd_u2s2(io, true); break;
    default: field_op<ModQ>(op, io); break;
  }
}

// Fq2: each at its bound-2 call site and at the largest bounds Fq2Tag::mul_ok / sqr_ok / mul_sub_ok admit.  Bounds in the names are per Fq2
// element (both coordinates).
GS_HD void fq2_op(int op, const Io& io) {
  Fq2e<2> r0, r1;
  switch (op) {
    LIMIT_OP(1, fq2_mul__2_2) put2(io, 0, mul(get2<2>(io, 0), get2<2>(io, 1))); break;
    LIMIT_OP(2, fq2_mul__8_9) put2(io, 0, mul(get2<8>(io, 0), get2<9>(io, 1))); break;
    LIMIT_OP(3, fq2_mul__9_2) put2(io, 0, mul(get2<9>(io, 0), get2<2>(io, 1))); break;
    LIMIT_OP(4, fq2_sqr__2) put2(io, 0, sqr(get2<2>(io, 0))); break;
    LIMIT_OP(5, fq2_sqr__5) put2(io, 0, sqr(get2<5>(io, 0))); break;
    LIMIT_OP(6, fq2_sqr__6) put2(io, 0, sqr(get2<6>(io, 0))); break;
    LIMIT_OP(7, fq2_mul_sub__2_2_2_2) put2(io, 0, mul_sub(get2<2>(io, 0), get2<2>(io, 1), get2<2>(io, 2), get2<2>(io, 3))); break;
    LIMIT_OP(8, fq2_mul_sub__5_12_2_2) put2(io, 0, mul_sub(get2<5>(io, 0), get2<12>(io, 1), get2<2>(io, 2), get2<2>(io, 3))); break;   // Y3 of the tight G2 mixed addition
    LIMIT_OP(9, fq2_mul_sub__2_12_5_2) put2(io, 0, mul_sub(get2<2>(io, 0), get2<12>(io, 1), get2<5>(io, 2), get2<2>(io, 3))); break;   // Y3 of the plain one
    LIMIT_OP(10, fq2_mul_sub__6_12_1_1) put2(io, 0, mul_sub(get2<6>(io, 0), get2<12>(io, 1), get2<1>(io, 2), get2<1>(io, 3))); break;  // 160
    LIMIT_OP(11, fq2_mul2__2_2_2_2) mul2(get2<2>(io, 0), get2<2>(io, 1), get2<2>(io, 2), get2<2>(io, 3), r0, r1); put2(io, 0, r0); put2(io, 1, r1); break;
    LIMIT_OP(12, fq2_mul2__2_2_9_2) mul2(get2<2>(io, 0), get2<2>(io, 1), get2<9>(io, 2), get2<2>(io, 3), r0, r1); put2(io, 0, r0); put2(io, 1, r1); break;   // P^3 | Q
    LIMIT_OP(13, fq2_mul2__8_9_9_8) mul2(get2<8>(io, 0), get2<9>(io, 1), get2<9>(io, 2), get2<8>(io, 3), r0, r1); put2(io, 0, r0); put2(io, 1, r1); break;
    LIMIT_OP(14, fq2_sqr2__2_2) sqr2(get2<2>(io, 0), get2<2>(io, 1), r0, r1); put2(io, 0, r0); put2(io, 1, r1); break;
    LIMIT_OP(15, fq2_sqr2__2_5) sqr2(get2<2>(io, 0), get2<5>(io, 1), r0, r1); put2(io, 0, r0); put2(io, 1, r1); break;                 // P^2 | R^2 of the tight addition
    LIMIT_OP(16, fq2_sqr2__6_6) sqr2(get2<6>(io, 0), get2<6>(io, 1), r0, r1); put2(io, 0, r0); put2(io, 1, r1); break;
    LIMIT_OP(17, fq2_inv__2) put2(io, 0, inv(get2<2>(io, 0))); break;
    LIMIT_OP(18, fq2_inv__8) put2(io, 0, inv(get2<8>(io, 0))); break;                                               // 2 x 8 x 8 <= 160
    default: break;
  }
}
#undef LIMIT_OP

// ---- points: accumulators at the top of their types
template <class T, int B>
GS_HD void store_coord(uint32_t* p, const typename T::template E<B>& e) {
  if constexpr (T::kWords == 8) {
#pragma unroll
    for (int i = 0; i < NL; ++i) p[i] = e.l[i];
  } else {
#pragma unroll
    for (int i = 0; i < NL; ++i) { p[i] = e.c0.l[i]; p[NL + i] = e.c1.l[i]; }
  }
}
// op: 0 xyzz_madd  1 xyzz_madd, negate  2 xyzz_add  3 xyzz_add_mem (second operand read from the record itself)  4 xyzz_dbl
//     5 / 6 the tight accumulator XyzzAcc + its xyzz_madd, plain / negate (G2 only; y < 2p)
template <class T>
GS_HD void point_op(int op, const uint32_t* in, uint32_t* out) {
  constexpr int cw = (T::kWords == 8 ? 1 : 2) * NL;
  Xyzz<T> acc = load_point<T>(in);
  const uint32_t* b = in + 4 * cw;
  Affine<T> q;
  q.x = load_coord<T, 1>(b); q.y = load_coord<T, 1>(b + cw);
  switch (op) {
    case 0: xyzz_madd(acc, q, false); break;
    case 1: xyzz_madd(acc, q, true); break;
    case 2: xyzz_add(acc, load_point<T>(b)); break;
    case 3: xyzz_add_mem<T>(acc, b); break;
    case 4: xyzz_dbl(acc); break;
    case 5: case 6:
      if constexpr (T::kWords != 8) {
        XyzzAcc<T> t;
        t.x = acc.x; t.y = load_coord<T, 2>(in + cw); t.zz = acc.zz; t.zzz = acc.zzz;
        xyzz_madd(t, q, op == 6);
        acc = to_xyzz(t);
      }
      break;
    default: break;
  }
  store_coord<T, 9>(out, acc.x); store_coord<T, 5>(out + cw, acc.y);
  store_coord<T, 2>(out + 2 * cw, acc.zz); store_coord<T, 2>(out + 3 * cw, acc.zzz);
}

// one record; out must be zeroed by the caller
GS_HD void run_case(int kind, int op, const uint32_t* in, uint32_t* out) {
  const Io io{in, out};
  switch (kind) {
    case 0: q_only_op(op, io); break;
    case 1: field_op<ModR>(op, io); break;
    case 2: fq2_op(op, io); break;
    case 3: point_op<FqTag>(op, in, out); break;
    case 4: point_op<Fq2Tag>(op, in, out); break;
    default: break;
  }
}

}  // namespace limits
}  // namespace gs
