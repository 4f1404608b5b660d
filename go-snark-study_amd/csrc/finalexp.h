// The rest of the Fq12 tower of fq12.h -- conjugation, inversion, the Frobenius maps, cyclotomic squaring -- and the final
// exponentiation f^((q^12 - 1)/r) of pairing.h, as __host__ __device__ source for the kernel of pairing_device.hip and for the
// host test (tests/host/finalexp_host_test.hip).  Everything is exact arithmetic in Fq and follows pairing.h's formulas and its
// addition chain step for step (products only in another order, which an exact commutative product does not notice), so a
// result is equal to the host's bit for bit on EVERY input, not only up to a power.
//
// Like fq12.h the operations take a STORE (get(i) / set(i, v), every stored coefficient < 2p) and work in place: operands are
// read before anything is written.  Nothing branches on a value: inversion is Fermat's fixed chain (fp29.h, inv: 0 -> 0), and
// the exponent of pow_x is a compile-time constant.
//
// final_exponentiation is written as a PROGRAM for a machine with one working value W and five slots: load, store, multiply
// W by a slot, and the unary operations on W.  A kernel then holds one copy of the code of each operation -- an Fq12 product
// alone is 18 Fq2 products of straight-line code, and the chain has 96 of them and 190 cyclotomic squarings -- and a caller
// chooses where W and the slots live: W in LDS and the slots in global memory on the device, six structs on the host.
#pragma once
#include "fq12.h"
#include "g2_subgroup.h"                                               // fq2_conj

namespace gs {

constexpr unsigned long long kBnX = 0x44e992b44a6909f1ULL;             // the BN parameter x, 63 bits (pairing.h, kX)

// gamma_K^I, gamma_K = w^(q^K - 1), for K = 1 and 3 (bn128_constants.h, Gen::frob; pairing.h computes them at run time: twc())
template <int K, int I> GS_HD Fq2e<1> frob_gamma() {
  static_assert((K == 1 || K == 3) && I >= 1 && I <= 5, "gamma_K^I");
  constexpr int row = (K == 1 ? 0 : 15) + 2 * (I - 1);
  Fq2e<1> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) { r.c0.l[i] = Gen::frob(row, i); r.c1.l[i] = Gen::frob(row + 1, i); }
  return r;
}
// gamma_2^I, an element of Fq
template <int I> GS_HD Fe<ModQ, 1> frob_gamma2() {
  static_assert(I >= 1 && I <= 5, "gamma_2^I");
  Fe<ModQ, 1> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = Gen::frob(10 + (I - 1), i);
  return r;
}

template <int B> GS_HD Fq6e<2> f6_reduce2(const Fq6e<B>& a) { return {reduce2(a.c0), reduce2(a.c1), reduce2(a.c2)}; }

// pairing.h, f6_inv: 1 / (c0 + c1 v + c2 v^2) through the norm to Fq2; 0 -> 0
GS_HD Fq6e<2> f6_inv(const Fq6e<2>& a) {
  const auto A = reduce2(sub(ssqr<F2>(a.c0), fq2_mul_xi(smul<F2>(a.c1, a.c2))));
  const auto B = reduce2(sub(fq2_mul_xi(ssqr<F2>(a.c2)), smul<F2>(a.c0, a.c1)));
  const auto C = reduce2(sub(ssqr<F2>(a.c1), smul<F2>(a.c0, a.c2)));
  const auto F = reduce2(add(smul<F2>(a.c0, A), fq2_mul_xi(add(smul<F2>(a.c2, B), smul<F2>(a.c1, C)))));
  const Fq2e<2> Fi = inv(F);
  return {smul<F2>(A, Fi), smul<F2>(B, Fi), smul<F2>(C, Fi)};
}

template <class D, class S> GS_HD void f12_copy(D& d, const S& s) {
#pragma unroll
  for (int i = 0; i < 6; ++i) d.set(i, s.get(i));
}

// f <- conj(f) = f^(q^6): the w-half changes sign
template <class S> GS_HD void f12_conj(S& f) {
#pragma unroll
  for (int i = 3; i < 6; ++i) f.set(i, reduce2(neg(f.get(i))));
}

// f <- 1/f = conj(f) / (a0^2 - v a1^2); 0 -> 0
template <class S> GS_HD void f12_inv(S& f) {
  const Fq6e<2> d = f6_inv(f6_reduce2(f6_sub(f6_mul(f12_half(f, 0), f12_half(f, 0)), f6_mul_v(f6_mul(f12_half(f, 1), f12_half(f, 1))))));
  const auto r0 = f6_mul(f12_half(f, 0), d);
  const auto r1 = f6_mul(f12_half(f, 1), d);
  f12_set_half(f, 0, r0);
  f.set(3, reduce2(neg(reduce2(r1.c0)))); f.set(4, reduce2(neg(reduce2(r1.c1)))); f.set(5, reduce2(neg(reduce2(r1.c2))));
}

// f <- f^(q^K): stored coefficient j belongs to w^i, i = 2j for the v-half and 2(j - 3) + 1 for the w-half; it is conjugated for
// odd K and multiplied by gamma_K^i (gamma_2 is in Fq)
template <int K, int I, class S> GS_HD void f12_frob_coeff(S& f, int j) {
  const Fq2e<2> c = f.get(j);
  if constexpr (K == 2) f.set(j, fq2_mul_fq(c, frob_gamma2<I>()));
  else f.set(j, smul<F2>(fq2_conj(c), frob_gamma<K, I>()));
}
template <int K, class S> GS_HD void f12_frob(S& f) {
  if constexpr (K != 2) f.set(0, reduce2(fq2_conj(f.get(0))));
  f12_frob_coeff<K, 2>(f, 1);
  f12_frob_coeff<K, 4>(f, 2);
  f12_frob_coeff<K, 1>(f, 3);
  f12_frob_coeff<K, 3>(f, 4);
  f12_frob_coeff<K, 5>(f, 5);
}

// (x0 + x1 s)^2 over Fq4 = Fq2[s]/(s^2 - xi) (pairing.h, f4_sqr), reduced
GS_HD void f4_sqr(const Fq2e<2>& x0, const Fq2e<2>& x1, Fq2e<2>& r0, Fq2e<2>& r1) {
  const auto t0 = ssqr<F2>(x0), t1 = ssqr<F2>(x1);
  r1 = reduce2(sub(sub(ssqr<F2>(add(x0, x1)), t0), t1));
  r0 = reduce2(add(t0, fq2_mul_xi(t1)));
}
GS_HD Fq2e<2> three_minus_two(const Fq2e<2>& t, const Fq2e<2>& c) { return reduce2(add(dbl(sub(t, c)), t)); }     // 3t - 2c
GS_HD Fq2e<2> three_plus_two(const Fq2e<2>& t, const Fq2e<2>& c) { return reduce2(add(dbl(add(t, c)), t)); }      // 3t + 2c

// f <- f^2 for a UNITARY f (after the easy part), Granger-Scott as in pairing.h's f12_cyclotomic_sqr: with c_i the coefficient of
// w^i, (c0, c3), (c1, c4), (c2, c5) are three elements of Fq4.  Stored index of c_i: 0, 3, 1, 4, 2, 5.
template <class S> GS_HD void f12_cyclotomic_sqr(S& f) {
  Fq2e<2> t0, t1, u0, u1, v0, v1;
  const Fq2e<2> c0 = f.get(0), c3 = f.get(4);
  f4_sqr(c0, c3, t0, t1);
  f.set(0, three_minus_two(t0, c0));
  f.set(4, three_plus_two(t1, c3));
  const Fq2e<2> c1 = f.get(3), c4 = f.get(2), c2 = f.get(1), c5 = f.get(5);
  f4_sqr(c2, c5, u0, u1);
  f4_sqr(c1, c4, v0, v1);
  f.set(3, three_plus_two(fq2_mul_xi(u1), c1));
  f.set(2, three_minus_two(u0, c4));
  f.set(1, three_minus_two(v0, c2));
  f.set(5, three_plus_two(v1, c5));
}

// w <- a^x for a unitary a that is not w (pairing.h, f12_pow_x): bit 62 is the top set bit of x
template <class W, class G> GS_HD void f12_pow_x(W& w, const G& a) {
  f12_copy(w, a);
#pragma unroll 1
  for (int i = 61; i >= 0; --i) {
    f12_cyclotomic_sqr(w);
    if ((kBnX >> i) & 1ull) f12_mul(w, a);
  }
}

// ---- the program ---------------------------------------------------------------------------------------------------------------
enum FeOp : unsigned char { FE_LOAD, FE_STORE, FE_MUL, FE_CYC, FE_CONJ, FE_FROB1, FE_FROB2, FE_FROB3, FE_INV, FE_END };
constexpr int kFeSlots = 5;

struct Fq12Bank {                                                      // the slots as structs: the host, and tests
  Fq12 s[kFeSlots];
  GS_HD Fq12& slot(int i) { return s[i]; }
};

struct FeProgram {
  static constexpr int kMax = 512;
  unsigned char code[kMax];                                            // op | slot << 4
  int n;
};
// (an index past kMax is not a constant expression: a program that outgrows the array does not compile)
constexpr void fe_emit(FeProgram& p, FeOp op, int slot = 0) { p.code[p.n++] = (unsigned char)(op | (slot << 4)); }
// W <- W^x for unitary W, which is also in slot s (pairing.h, f12_pow_x)
constexpr void fe_emit_pow_x(FeProgram& p, int s) {
  for (int i = 61; i >= 0; --i) {
    fe_emit(p, FE_CYC);
    if ((kBnX >> i) & 1) fe_emit(p, FE_MUL, s);
  }
}
constexpr FeProgram fe_program(bool easy_part_only) {
  FeProgram p = {};
  // easy part: t = f^((q^6 - 1)(q^2 + 1)), f in W on entry
  fe_emit(p, FE_STORE, 0); fe_emit(p, FE_INV); fe_emit(p, FE_STORE, 1);
  fe_emit(p, FE_LOAD, 0); fe_emit(p, FE_CONJ); fe_emit(p, FE_MUL, 1);
  fe_emit(p, FE_STORE, 0); fe_emit(p, FE_FROB2); fe_emit(p, FE_MUL, 0);
  if (!easy_part_only) {
    fe_emit(p, FE_STORE, 0);                                                                     // slot 0 = t
    fe_emit_pow_x(p, 0); fe_emit(p, FE_STORE, 1);                                                // slot 1 = fx
    fe_emit_pow_x(p, 1); fe_emit(p, FE_STORE, 2);                                                // slot 2 = fx2
    fe_emit_pow_x(p, 2); fe_emit(p, FE_STORE, 3);                                                // slot 3 = fx3
    // y0 .. y6 and the vector addition chain y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 of pairing.h; t0 lives in slot 3, t1 in slot 4
    fe_emit(p, FE_FROB1); fe_emit(p, FE_MUL, 3); fe_emit(p, FE_CONJ); fe_emit(p, FE_CYC); fe_emit(p, FE_STORE, 3);        // t0 = y6^2
    fe_emit(p, FE_LOAD, 2); fe_emit(p, FE_FROB1); fe_emit(p, FE_MUL, 1); fe_emit(p, FE_CONJ);                             // y4
    fe_emit(p, FE_MUL, 3); fe_emit(p, FE_STORE, 3);                                                                       // t0 *= y4
    fe_emit(p, FE_LOAD, 2); fe_emit(p, FE_CONJ); fe_emit(p, FE_STORE, 4);                                                 // slot 4 = y5
    fe_emit(p, FE_MUL, 3); fe_emit(p, FE_STORE, 3);                                                                       // t0 *= y5
    fe_emit(p, FE_LOAD, 1); fe_emit(p, FE_FROB1); fe_emit(p, FE_CONJ);                                                    // y3
    fe_emit(p, FE_MUL, 4); fe_emit(p, FE_MUL, 3); fe_emit(p, FE_STORE, 4);                                                // t1 = y3 y5 t0
    fe_emit(p, FE_LOAD, 2); fe_emit(p, FE_FROB2); fe_emit(p, FE_MUL, 3); fe_emit(p, FE_STORE, 3);                         // t0 *= y2
    fe_emit(p, FE_LOAD, 4); fe_emit(p, FE_CYC); fe_emit(p, FE_MUL, 3); fe_emit(p, FE_CYC); fe_emit(p, FE_STORE, 4);       // t1 = (t1^2 t0)^2
    fe_emit(p, FE_LOAD, 0); fe_emit(p, FE_FROB1); fe_emit(p, FE_STORE, 1);
    fe_emit(p, FE_LOAD, 0); fe_emit(p, FE_FROB2); fe_emit(p, FE_MUL, 1); fe_emit(p, FE_STORE, 1);
    fe_emit(p, FE_LOAD, 0); fe_emit(p, FE_FROB3); fe_emit(p, FE_MUL, 1);                                                  // y0
    fe_emit(p, FE_MUL, 4); fe_emit(p, FE_STORE, 1);                                                                       // slot 1 = t1 y0
    fe_emit(p, FE_LOAD, 0); fe_emit(p, FE_CONJ); fe_emit(p, FE_MUL, 4); fe_emit(p, FE_CYC);                               // (t1 y1)^2
    fe_emit(p, FE_MUL, 1);
  }
  fe_emit(p, FE_END);
  return p;
}

// one step: `code` is uniform over a wave (it comes from the constant program), the switch is a scalar branch
template <class W, class Bank> GS_HD void fe_step(unsigned code, W& w, Bank& bank) {
  decltype(auto) g = bank.slot((int)(code >> 4));
  switch (code & 15) {
    case FE_LOAD: f12_copy(w, g); break;
    case FE_STORE: f12_copy(g, w); break;
    case FE_MUL: f12_mul(w, g); break;
    case FE_CYC: f12_cyclotomic_sqr(w); break;
    case FE_CONJ: f12_conj(w); break;
    case FE_FROB1: f12_frob<1>(w); break;
    case FE_FROB2: f12_frob<2>(w); break;
    case FE_FROB3: f12_frob<3>(w); break;
    case FE_INV: f12_inv(w); break;
    default: break;
  }
}

// w <- w^((q^12 - 1)/r) (pairing.h, final_exponentiation), or its easy part alone: the unitary w^((q^6 - 1)(q^2 + 1)).
// A BANK hands out the kFeSlots scratch stores: slot(i) returns a store or a reference to one.  They may be uninitialised.
template <bool kEasyOnly = false, class W, class Bank> GS_HD void final_exponentiation(W& w, Bank& bank) {
  static constexpr FeProgram prog = fe_program(kEasyOnly);
  static_assert(prog.n > 0 && prog.n <= FeProgram::kMax && prog.code[prog.n - 1] == FE_END, "the program fits FeProgram::kMax and ends");
#pragma unroll 1
  for (int pc = 0; prog.code[pc] != FE_END; ++pc) fe_step((unsigned)prog.code[pc], w, bank);
}

// is the stored value one?  Exact (fp29.h, is_zero), for the verdicts
template <class S> GS_HD bool f12_is_one(const S& f) {
  const Fq2e<2> c = f.get(0);
  int ok = (int)is_zero(sub(c.c0, fe_one<ModQ>())) & (int)is_zero(c.c1);
#pragma unroll
  for (int i = 1; i < 6; ++i) { const Fq2e<2> v = f.get(i); ok &= (int)is_zero(v.c0) & (int)is_zero(v.c1); }
  return ok != 0;
}

}  // namespace gs
