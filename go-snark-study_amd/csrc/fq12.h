// Fq6 = Fq2[v]/(v^3 - xi), xi = 9 + u, and Fq12 = Fq6[w]/(w^2 - v) over Fq2e (fq2.h, 29-bit limbs): the tower of pairing.h, as
// __host__ __device__ source for the Miller-loop kernel of pairing_device.hip and for the host test (tests/host/miller_host_test.hip).
//
// An Fq12 is six Fq2 coefficients in the order of pairing.h and of gs_pairing's encoding: (a0.c0, a0.c1, a0.c2, a1.c0, a1.c1, a1.c2),
// that is the coefficients of 1, v, v^2, w, v w, v^2 w.  An accumulator is 108 limbs, more than a lane can keep in registers beside a
// running G2 point and a line, so the three operations below do not take a struct: they take a STORE, anything with
//     Fq2e<2> get(int i) const      and      void set(int i, const Fq2e<2>&)            (i a compile-time constant after inlining)
// and read each coefficient where it is used and write the six results at the end.  Fq12 (an array in registers / on the host stack)
// is one such store, the limb-major slice of LDS a lane owns in pairing_device.hip is another.  Every stored coefficient is < 2p.
//
// Bounds: Fq6 products come back unreduced (Fq6e<10>: a Karatsuba coefficient is three or four products of bound 2 added up), the
// Fq12 level adds at most three of those (bound 32 of the 40 the bias tables reach) and reduces once per stored coefficient.
#pragma once
#include "ec.h"

namespace gs {

using F2 = Fq2Tag;

template <int B> struct Fq6e { Fq2e<B> c0, c1, c2; };

struct Fq12 {
  Fq2e<2> c[6];
  GS_HD Fq2e<2> get(int i) const { return c[i]; }
  GS_HD void set(int i, const Fq2e<2>& v) { c[i] = v; }
};

// xi = 9 + u in Montgomery form: 8 + 1 times the constant one, straight-line code on constants that the compiler folds
GS_HD Fq2e<2> fq2_xi() {
  const auto one = fe_one<ModQ>();
  return {reduce2(add(dbl(dbl(dbl(one))), one)), relax<2>(one)};
}
template <int B> GS_HD Fq2e<2> fq2_mul_xi(const Fq2e<B>& a) { return smul<F2>(a, fq2_xi()); }
// an Fq2 element times one of Fq
template <int B, int Bk> GS_HD Fq2e<2> fq2_mul_fq(const Fq2e<B>& a, const Fe<ModQ, Bk>& k) { return {smul<FqTag>(a.c0, k), smul<FqTag>(a.c1, k)}; }

template <int Ba, int Bb> GS_HD Fq6e<Ba + Bb> f6_add(const Fq6e<Ba>& a, const Fq6e<Bb>& b) { return {add(a.c0, b.c0), add(a.c1, b.c1), add(a.c2, b.c2)}; }
template <int Ba, int Bb> GS_HD Fq6e<Ba + Bb + 1> f6_sub(const Fq6e<Ba>& a, const Fq6e<Bb>& b) { return {sub(a.c0, b.c0), sub(a.c1, b.c1), sub(a.c2, b.c2)}; }
// v (c0 + c1 v + c2 v^2) = xi c2 + c0 v + c1 v^2
template <int B> GS_HD Fq6e<B> f6_mul_v(const Fq6e<B>& a) { return {relax<B>(fq2_mul_xi(a.c2)), a.c0, a.c1}; }

// Karatsuba, the formulas of pairing.h's f6_mul; operands up to bound 4 (sums of two stored coefficients)
template <int Ba, int Bb>
GS_HD Fq6e<10> f6_mul(const Fq6e<Ba>& a, const Fq6e<Bb>& b) {
  static_assert(Ba <= 4 && Bb <= 4, "f6_mul takes stored coefficients or sums of two");
  const auto t0 = smul<F2>(a.c0, b.c0), t1 = smul<F2>(a.c1, b.c1), t2 = smul<F2>(a.c2, b.c2);
  const auto m12 = smul<F2>(add(a.c1, a.c2), add(b.c1, b.c2));
  const auto m01 = smul<F2>(add(a.c0, a.c1), add(b.c0, b.c1));
  const auto m02 = smul<F2>(add(a.c0, a.c2), add(b.c0, b.c2));
  Fq6e<10> r;
  r.c0 = relax<10>(add(t0, fq2_mul_xi(sub(sub(m12, t1), t2))));               // 2 + 2
  r.c1 = add(sub(sub(m01, t0), t1), fq2_mul_xi(t2));                           // 8 + 2
  r.c2 = add(sub(sub(m02, t0), t2), t1);                                       // 8 + 2
  return r;
}
// a (b0 + b1 v): the w-part of a line (pairing.h, f6_mul_01)
template <int Ba, int B0, int B1>
GS_HD Fq6e<8> f6_mul_01(const Fq6e<Ba>& a, const Fq2e<B0>& b0, const Fq2e<B1>& b1) {
  static_assert(Ba <= 4 && B0 <= 4 && B1 <= 2, "f6_mul_01 operand bounds");
  const auto t0 = smul<F2>(a.c0, b0), t1 = smul<F2>(a.c1, b1);
  Fq6e<8> r;
  r.c0 = relax<8>(add(t0, fq2_mul_xi(smul<F2>(a.c2, b1))));
  r.c1 = sub(sub(smul<F2>(add(a.c0, a.c1), add(b0, b1)), t0), t1);             // 2 + 3 + 3 = 8
  r.c2 = relax<8>(add(smul<F2>(a.c2, b0), t1));
  return r;
}

template <class S> GS_HD Fq6e<2> f12_half(const S& f, int h) { return {f.get(3 * h), f.get(3 * h + 1), f.get(3 * h + 2)}; }
template <class S, int B> GS_HD void f12_set_half(S& f, int h, const Fq6e<B>& a) {
  f.set(3 * h, reduce2(a.c0)); f.set(3 * h + 1, reduce2(a.c1)); f.set(3 * h + 2, reduce2(a.c2));
}

template <class S> GS_HD void f12_set_one(S& f) {
  f.set(0, relax<2>(fq2_one()));
#pragma unroll
  for (int i = 1; i < 6; ++i) f.set(i, fq2_zero<2>());
}

// f <- f g  (g may be f: the operands are read before anything is written)
template <class S, class G>
GS_HD void f12_mul(S& f, const G& g) {
  const auto t0 = f6_mul(f12_half(f, 0), f12_half(g, 0));
  const auto t1 = f6_mul(f12_half(f, 1), f12_half(g, 1));
  const auto m = f6_mul(f6_add(f12_half(f, 0), f12_half(f, 1)), f6_add(f12_half(g, 0), f12_half(g, 1)));
  f12_set_half(f, 1, f6_sub(f6_sub(m, t0), t1));                               // 10 + 11 + 11
  f12_set_half(f, 0, f6_add(t0, f6_mul_v(t1)));
}

// f <- f^2, complex squaring over Fq6: c1 = 2 a0 a1, c0 = (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1
template <class S>
GS_HD void f12_sqr(S& f) {
  const auto t = f6_mul(f12_half(f, 0), f12_half(f, 1));
  const auto m = f6_mul(f6_add(f12_half(f, 0), f12_half(f, 1)), f6_add(f12_half(f, 0), f6_mul_v(f12_half(f, 1))));
  f12_set_half(f, 0, f6_sub(f6_sub(m, t), f6_mul_v(t)));
  f12_set_half(f, 1, f6_add(t, t));
}

// f <- f (a + b w + c w^3) = f (a + (b + c v) w): a line of the Miller loop, the shape of pairing.h's f12_mul_line with a in Fq2
template <class S>
GS_HD void f12_mul_line(S& f, const Fq2e<2>& a, const Fq2e<2>& b, const Fq2e<2>& c) {
  const Fq6e<2> f0 = f12_half(f, 0);
  const Fq6e<2> t0 = {smul<F2>(f0.c0, a), smul<F2>(f0.c1, a), smul<F2>(f0.c2, a)};
  const auto t1 = f6_mul_01(f12_half(f, 1), b, c);
  const auto m = f6_mul_01(f6_add(f12_half(f, 0), f12_half(f, 1)), add(a, b), c);
  f12_set_half(f, 1, f6_sub(f6_sub(m, t0), t1));                               // 8 + 3 + 9
  f12_set_half(f, 0, f6_add(t0, f6_mul_v(t1)));
}

// the 48-word standard encoding of gs_pairing (verify.hip, f12_to_std): per coefficient c0 then c1, four 64-bit words each
template <class S>
GS_HD void f12_to_std(const S& f, uint64_t* out) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    const Fq2e<2> v = f.get(i);
    uint32_t w[8];
    pack32<ModQ>(from_mont(v.c0), w);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[8 * i + j] = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
    pack32<ModQ>(from_mont(v.c1), w);
#pragma unroll
    for (int j = 0; j < 4; ++j) out[8 * i + 4 + j] = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
  }
}
// ... and back (any 256-bit words)
template <class S>
GS_HD void f12_from_std(S& f, const uint64_t* in) {
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    Fq2e<2> v;
    uint32_t w[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) { w[2 * j] = (uint32_t)in[8 * i + j]; w[2 * j + 1] = (uint32_t)(in[8 * i + j] >> 32); }
    v.c0 = to_mont(unpack32<ModQ>(w));
#pragma unroll
    for (int j = 0; j < 4; ++j) { w[2 * j] = (uint32_t)in[8 * i + 4 + j]; w[2 * j + 1] = (uint32_t)(in[8 * i + 4 + j] >> 32); }
    v.c1 = to_mont(unpack32<ModQ>(w));
    f.set(i, v);
  }
}

}  // namespace gs
