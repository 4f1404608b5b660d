// Is a point of the twist E'(Fq2) in G2, the subgroup of order r?  Exact and per point, the same __host__ __device__ source for the
// kernel of g2_subgroup.hip and for the host test (tests/host/g2_subgroup_host_test.hip).
//
// E'(Fq2) has r (2q - r) points and the cofactor 2q - r = 10069 x (a 246-bit rest) is not prime, so a point that passes the curve equation
// may carry a component of small order.  The untwist-Frobenius-twist endomorphism psi(x, y) = (conj(x) g2, conj(y) g3), g2 = xi^((q-1)/3),
// g3 = xi^((q-1)/2), xi = 9 + u, satisfies psi^2 - [t] psi + [q] = 0 on all of E' and acts on G2 as [q mod r] = [6 x^2].  With the BN
// parameter x the test is
//     [x + 1] Q + psi([x] Q) + psi^2([x] Q) = psi^3([2x] Q)
// (El Housni, Guillevic, Piellard: "Co-factor clearing and subgroup membership testing on pairing-friendly curves", 2022, section 4.3):
// one multiplication by the 63-bit x, non-adjacent weight 24, where the host's psi(Q) = [6 x^2] Q (pairing.h) takes a 127-bit one of
// weight 40.  The scalar is a compile-time constant: every lane of a wave takes the same branch at every digit.
//
// psi is a homomorphism, so the equation is evaluated as a Horner chain in psi that keeps ONE running point beside A = [x] Q:
//     Q + A + psi(A + psi(A - psi(2 A))) = O
// Every addition is the complete one (ec.h): on a point of small order an intermediate multiple does meet +-Q, A or infinity.  No
// inversion: the verdict is "the sum is the point at infinity".
#pragma once
#include "ec.h"

namespace gs {

GS_HD Fq2e<1> g2_psi_gx() {
  Fq2e<1> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) { r.c0.l[i] = Gen::psi2c0(i); r.c1.l[i] = Gen::psi2c1(i); }
  return r;
}
GS_HD Fq2e<1> g2_psi_gy() {
  Fq2e<1> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) { r.c0.l[i] = Gen::psi3c0(i); r.c1.l[i] = Gen::psi3c1(i); }
  return r;
}
template <int B> GS_HD Fq2e<B + 1> fq2_conj(const Fq2e<B>& a) { return {relax<B + 1>(a.c0), neg(a.c1)}; }

// psi of an affine point, canonical; infinity stays infinity
GS_HD Affine<Fq2Tag> g2_psi(const Affine<Fq2Tag>& p) {
  if (is_inf(p)) return p;
  Affine<Fq2Tag> r;
  r.x = canon(smul<Fq2Tag>(fq2_conj(p.x), g2_psi_gx()));
  r.y = canon(smul<Fq2Tag>(fq2_conj(p.y), g2_psi_gy()));
  return r;
}
// psi of (X/ZZ, Y/ZZZ) = (conj(X) g2 / conj(ZZ), conj(Y) g3 / conj(ZZZ)); conj keeps ZZ^3 = ZZZ^2
GS_HD void g2_psi(Xyzz<Fq2Tag>& p) {
  if (is_inf(p)) return;                                // (the conjugate of an all-zero limb vector is p, not all-zero limbs)
  p.x = relax<9>(smul<Fq2Tag>(fq2_conj(p.x), g2_psi_gx()));
  p.y = relax<5>(smul<Fq2Tag>(fq2_conj(p.y), g2_psi_gy()));
  p.zz.c1 = reduce2(neg(p.zz.c1));
  p.zzz.c1 = reduce2(neg(p.zzz.c1));
}

// [x] q for a finite q: the digits of x in non-adjacent form, most significant first (Gen::kXNafPos / kXNafNeg)
GS_HD Xyzz<Fq2Tag> g2_mul_bn_x(const Affine<Fq2Tag>& q) {
  Xyzz<Fq2Tag> acc = xyzz_from_affine(q);               // the leading digit, +1
#pragma unroll 1
  for (int i = Gen::kXNafDigits - 2; i >= 0; --i) {
    xyzz_dbl(acc);
    const bool plus = (Gen::kXNafPos >> i) & 1ull, minus = (Gen::kXNafNeg >> i) & 1ull;
    if (plus || minus) xyzz_madd(acc, q, minus);
  }
  return acc;
}

GS_HD bool g2_in_subgroup(const Affine<Fq2Tag>& q) {
  if (is_inf(q)) return true;
  const Xyzz<Fq2Tag> a = g2_mul_bn_x(q);
  Xyzz<Fq2Tag> t = a;
  xyzz_dbl(t);
  t = xyzz_neg(t);
  // three times t = A + psi(t): A - psi(2A), A + psi(A - psi(2A)), A + psi(A + psi(A - psi(2A))).  A loop, not three copies: one
  // instance of the general addition keeps the register allocation of the tail as small as the chain's.
#pragma unroll 1
  for (int k = 0; k < 3; ++k) {
    g2_psi(t);
    xyzz_add(t, a);
  }
  xyzz_madd(t, q);                                      // Q + A + psi(A + psi(A - psi(2A)))
  return is_inf(t);
}

}  // namespace gs
