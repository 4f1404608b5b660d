// The optimal ate Miller loop of BN254 for ONE pair, as __host__ __device__ source: f_{6x+2, Q}(P) times the two Frobenius lines, the
// function pairing.h's multi_miller_loop computes for every pair -- up to factors in Fq2, which the final exponentiation kills (its
// exponent is a multiple of q^6 - 1).  So a value of this loop is compared with the host's only after final_exponentiation, and
// there it is equal bit for bit.
//
// Why not the host's steps: they are affine, one inversion per step shared by all pairs of a call.  A lane has one pair, so the
// running point T is homogeneous projective (x = X/Z, y = Y/Z) and the lines are the host's scaled by their denominators
// (Costello, Lange, Naehrig: "Faster pairing computations on curves with high-degree twists", 2010, section 5; b' = 3/xi):
//   doubling   2YZ y_P - 3X^2 x_P w + (Y^2 - 3b' Z^2) w^3
//              X3 = 2XY (Y^2 - 9b' Z^2),  Y3 = (Y^2 + 9b' Z^2)^2 - 12 (3b' Z^2)^2,  Z3 = 8 Y^3 Z
//   addition   with theta = Y - y_R Z, lambda = X - x_R Z:     lambda y_P - theta x_P w + (theta x_R - lambda y_R) w^3
//              H = lambda^3 + Z theta^2 - 2 X lambda^2,  X3 = lambda H,  Y3 = theta (X lambda^2 - H) - lambda^3 Y,  Z3 = Z lambda^3
// The doubling uses the curve equation of T (uploads check it for Q).  Nothing here inverts, compares or branches on a value: the
// loop bits are compile-time constants, the two loops are not unrolled, and every lane of a wave runs the same instructions whatever
// its pair holds.  A pair with an infinite member runs on the generators and its result is replaced by one at the end.  A Q on the
// twist but outside the order-r subgroup (the caller's precondition, gs_g2_subgroup_check) gives a value that means nothing, from
// the same instruction sequence.
//
// The accumulator lives in a store (fq12.h): registers on the host, a slice of LDS in the kernel.
#pragma once
#include "fq12.h"
#include "g2_subgroup.h"

namespace gs {

constexpr unsigned long long kAteLoopLow = 0x9d797039be763ba8ULL;      // 6x + 2 = 2^64 + this (pairing.h, kLoop)

struct G2Proj { Fq2e<2> x, y, z; };
struct Line { Fq2e<2> a, b, c; };                                      // a + b w + c w^3

GS_HD Fq2e<3> g2_three_b() {
  const Fq2e<1> b = curve_b<Fq2Tag>();
  return add(dbl(b), b);
}

// T <- 2T and the tangent at T evaluated at P = (xp, yp); nxp = -xp
GS_HD Line miller_double(G2Proj& t, const Fe<ModQ, 2>& nxp, const Fe<ModQ, 1>& yp) {
  const auto A = smul<F2>(t.x, t.y);
  const auto B = ssqr<F2>(t.y);
  const auto C = ssqr<F2>(t.z);
  const auto E = smul<F2>(C, g2_three_b());                            // 3b' Z^2
  const auto F = add(dbl(E), E);                                       // 9b' Z^2, bound 6
  const auto H = dbl(smul<F2>(t.y, t.z));                              // 2YZ, bound 4
  const auto J = ssqr<F2>(t.x);
  const auto E2 = ssqr<F2>(E);
  Line l;
  l.a = fq2_mul_fq(H, yp);
  l.b = fq2_mul_fq(add(dbl(J), J), nxp);
  l.c = reduce2(sub(B, E));
  t.x = smul<F2>(dbl(A), sub(B, F));
  t.y = reduce2(sub(ssqr<F2>(add(B, F)), dbl(dbl(add(dbl(E2), E2)))));  // 2 + 24 + 1
  t.z = smul<F2>(dbl(dbl(B)), H);
  return l;
}

// T <- T + R for an affine R != +-T, and the chord through T and R evaluated at P
GS_HD Line miller_add(G2Proj& t, const Affine<Fq2Tag>& r, const Fe<ModQ, 2>& nxp, const Fe<ModQ, 1>& yp) {
  const auto theta = sub(t.y, smul<F2>(r.y, t.z));                     // bound 5
  const auto lam = sub(t.x, smul<F2>(r.x, t.z));
  const auto C = ssqr<F2>(theta);
  const auto D = ssqr<F2>(lam);
  const auto E = smul<F2>(lam, D);
  const auto F = smul<F2>(t.z, C);
  const auto G = smul<F2>(t.x, D);
  const auto H = sub(add(E, F), dbl(G));                               // bound 9
  Line l;
  l.a = fq2_mul_fq(lam, yp);
  l.b = fq2_mul_fq(theta, nxp);
  l.c = smul_sub<F2>(theta, r.x, lam, r.y);
  const auto y3 = smul_sub<F2>(theta, sub(G, H), E, t.y);
  t.x = smul<F2>(lam, H);
  t.y = y3;
  t.z = smul<F2>(t.z, E);
  return l;
}

// the twisted Frobenius of a finite affine point (g2_subgroup.h: psi), without the test for infinity
GS_HD Affine<Fq2Tag> miller_psi(const Affine<Fq2Tag>& p) {
  Affine<Fq2Tag> r;
  r.x = canon(smul<F2>(fq2_conj(p.x), g2_psi_gx()));
  r.y = canon(smul<F2>(fq2_conj(p.y), g2_psi_gy()));
  return r;
}

template <class S>
GS_HD void miller_loop(S& f, const Affine<FqTag>& p_in, const Affine<Fq2Tag>& q_in) {
  bool skip = is_inf(p_in);
  skip |= is_inf(q_in);
  Affine<FqTag> p;
  Affine<Fq2Tag> q;
#pragma unroll
  for (int i = 0; i < NL; ++i) {                                       // the substitute pair: the generators
    p.x.l[i] = skip ? Gen::g1x(i) : p_in.x.l[i];
    p.y.l[i] = skip ? Gen::g1y(i) : p_in.y.l[i];
    q.x.c0.l[i] = skip ? Gen::g2x0(i) : q_in.x.c0.l[i];
    q.x.c1.l[i] = skip ? Gen::g2x1(i) : q_in.x.c1.l[i];
    q.y.c0.l[i] = skip ? Gen::g2y0(i) : q_in.y.c0.l[i];
    q.y.c1.l[i] = skip ? Gen::g2y1(i) : q_in.y.c1.l[i];
  }
  const Fe<ModQ, 2> nxp = neg(p.x);
  G2Proj t = {relax<2>(q.x), relax<2>(q.y), relax<2>(fq2_one())};
  Affine<Fq2Tag> r = q;
  f12_set_one(f);
  // steps 63 .. 0: the bits of 6x + 2 below the leading one; steps -1 and -2: the chords to pi(Q) and to -pi^2(Q)
#pragma unroll 1
  for (int i = 63; i >= -2; --i) {
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
      Line l;
      if (phase == 0) {
        if (i < 0) continue;
        f12_sqr(f);
        l = miller_double(t, nxp, p.y);
      } else {
        if (i >= 0 && !((kAteLoopLow >> i) & 1ull)) continue;
        if (i < 0) {
          r = miller_psi(r);
          if (i == -2) r.y = canon(neg(r.y));
        }
        l = miller_add(t, r, nxp, p.y);
      }
      f12_mul_line(f, l.a, l.b, l.c);
    }
  }
  f.set(0, select(skip, relax<2>(fq2_one()), f.get(0)));
#pragma unroll
  for (int i = 1; i < 6; ++i) f.set(i, select(skip, fq2_zero<2>(), f.get(i)));
}

// ---- a Groth16 proof: three pairs, ONE accumulator --------------------------------------------------------------------------------
// f <- the Miller value of e(P1, Q1) e(P2, gamma) e(P3, delta): the three pairs share the 64 squarings of f.  gamma and delta are the
// same in every lane, so their lines come PREPARED (pairing.h, prepare_g2_lines: the host's affine steps, (lambda, lambda x_T - y_T)
// per step) and a lane only evaluates them at its P2 and P3: y_P - lambda x_P w + c w^3.  Only the pair with Q1 runs G2 arithmetic,
// the projective steps of miller_loop.  The lines of the three pairs differ from the host's by factors in Fq2, which the final
// exponentiation removes.  A pair whose P (or Q1) is infinite, or whose `skip` flag is set (an infinite gamma or delta), contributes
// one: its line is replaced by the constant 1, a select, not a branch.  L is anything with
//     Fq2e<2> lambda(int k) const   and   Fq2e<2> c(int k) const      (k = the step, the same for every lane of a wave)
constexpr int kPreparedSteps = 64 + 36 + 2;           // tangents + the 36 set bits of kAteLoopLow + the two Frobenius chords
static_assert(__builtin_popcountll(kAteLoopLow) == 36, "kPreparedSteps");

GS_HD Line line_or_one(bool skip, const Line& l) {
  return {select(skip, relax<2>(fq2_one()), l.a), select(skip, fq2_zero<2>(), l.b), select(skip, fq2_zero<2>(), l.c)};
}
template <class L>
GS_HD Line prepared_line_at(const L& lines, int k, const Fe<ModQ, 2>& nxp, const Fe<ModQ, 1>& yp) {
  Line l;
  l.a = {relax<2>(yp), fe_zero<ModQ, 2>()};
  l.b = fq2_mul_fq(lines.lambda(k), nxp);
  l.c = lines.c(k);
  return l;
}

template <class S, class L>
GS_HD void miller_loop_groth16(S& f, const Affine<FqTag>& p1_in, const Affine<Fq2Tag>& q1_in, const Affine<FqTag>& p2, bool skip_gamma,
                               const L& gamma, const Affine<FqTag>& p3, bool skip_delta, const L& delta) {
  bool skip1 = is_inf(p1_in);
  skip1 |= is_inf(q1_in);
  const bool skip2 = skip_gamma | is_inf(p2), skip3 = skip_delta | is_inf(p3);
  Affine<FqTag> p;
  Affine<Fq2Tag> q;
#pragma unroll
  for (int i = 0; i < NL; ++i) {                                       // the substitute pair: the generators
    p.x.l[i] = skip1 ? Gen::g1x(i) : p1_in.x.l[i];
    p.y.l[i] = skip1 ? Gen::g1y(i) : p1_in.y.l[i];
    q.x.c0.l[i] = skip1 ? Gen::g2x0(i) : q1_in.x.c0.l[i];
    q.x.c1.l[i] = skip1 ? Gen::g2x1(i) : q1_in.x.c1.l[i];
    q.y.c0.l[i] = skip1 ? Gen::g2y0(i) : q1_in.y.c0.l[i];
    q.y.c1.l[i] = skip1 ? Gen::g2y1(i) : q1_in.y.c1.l[i];
  }
  const Fe<ModQ, 2> nxp = neg(p.x), nxp2 = neg(p2.x), nxp3 = neg(p3.x);
  G2Proj t = {relax<2>(q.x), relax<2>(q.y), relax<2>(fq2_one())};
  Affine<Fq2Tag> r = q;
  f12_set_one(f);
  int k = 0;
#pragma unroll 1
  for (int i = 63; i >= -2; --i) {
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
      Line l;
      if (phase == 0) {
        if (i < 0) continue;
        f12_sqr(f);
        l = miller_double(t, nxp, p.y);
      } else {
        if (i >= 0 && !((kAteLoopLow >> i) & 1ull)) continue;
        if (i < 0) {
          r = miller_psi(r);
          if (i == -2) r.y = canon(neg(r.y));
        }
        l = miller_add(t, r, nxp, p.y);
      }
      l = line_or_one(skip1, l);
      f12_mul_line(f, l.a, l.b, l.c);
      l = line_or_one(skip2, prepared_line_at(gamma, k, nxp2, p2.y));
      f12_mul_line(f, l.a, l.b, l.c);
      l = line_or_one(skip3, prepared_line_at(delta, k, nxp3, p3.y));
      f12_mul_line(f, l.a, l.b, l.c);
      ++k;
    }
  }
}

// ---- up to three pairs, ALL of their lines prepared -------------------------------------------------------------------------------
// f <- the Miller value of e(P1, Q1) e(P2, Q2) e(P3, Q3) where every Q is the same in every lane (key points and the G2 generator of
// a Pinocchio key): no G2 arithmetic and no running point, a lane only evaluates the three prepared lists at its own P.  The steps are
// taken in the order prepare_g2_lines writes them: per bit of 6x + 2 the tangent, then the chord if the bit is set; then the two
// Frobenius chords.  One squaring of f per bit, shared by the pairs.  A pair whose P is infinite or whose skip flag is set (an
// infinite or absent Q) contributes one by line_or_one.
template <class S, class L>
GS_HD void miller_loop_prepared(S& f, const Affine<FqTag>& p1, bool skip_q1, const L& q1, const Affine<FqTag>& p2, bool skip_q2, const L& q2,
                                const Affine<FqTag>& p3, bool skip_q3, const L& q3) {
  const bool skip1 = skip_q1 | is_inf(p1), skip2 = skip_q2 | is_inf(p2), skip3 = skip_q3 | is_inf(p3);
  const Fe<ModQ, 2> nxp1 = neg(p1.x), nxp2 = neg(p2.x), nxp3 = neg(p3.x);
  f12_set_one(f);
  int k = 0;
#pragma unroll 1
  for (int i = 63; i >= -2; --i) {
#pragma unroll 1
    for (int phase = 0; phase < 2; ++phase) {
      if (phase == 0) {
        if (i < 0) continue;
        f12_sqr(f);
      } else {
        if (i >= 0 && !((kAteLoopLow >> i) & 1ull)) continue;
      }
      Line l = line_or_one(skip1, prepared_line_at(q1, k, nxp1, p1.y));
      f12_mul_line(f, l.a, l.b, l.c);
      l = line_or_one(skip2, prepared_line_at(q2, k, nxp2, p2.y));
      f12_mul_line(f, l.a, l.b, l.c);
      l = line_or_one(skip3, prepared_line_at(q3, k, nxp3, p3.y));
      f12_mul_line(f, l.a, l.b, l.c);
      ++k;
    }
  }
}

// the two sums the Pinocchio equations 4 and 5 share: vkx + A and vkx + A + C, by the complete formulas of ec.h (A may be vkx, -vkx or
// infinite, and so may C against the first sum)
GS_HD void pinocchio_sums(const Affine<FqTag>& vkx, const Affine<FqTag>& a, const Affine<FqTag>& c, Affine<FqTag>& xa, Affine<FqTag>& xac) {
  Xyzz<FqTag> acc = xyzz_inf<FqTag>();
  xyzz_madd(acc, vkx);
  xyzz_madd(acc, a);
  xa = xyzz_to_affine(acc);
  xyzz_madd(acc, c);
  xac = xyzz_to_affine(acc);
}

// vkx = IC_0 + sum_j pub_j IC_{j+1} (verify.hip, accumulate_ic): a joint double-and-add over the npublic points, ONE doubling chain of
// 256 steps and an addition per set bit per signal, complete formulas (ec.h), so any 256-bit scalar is taken as it is -- the group law
// reduces it -- and an addition that meets a doubling or the inverse is right.  ic(j) gives the affine IC_j, bit(j, b) bit b of signal j.
template <class IC, class BITS>
GS_HD Affine<FqTag> groth16_vkx(const IC& ic, const BITS& bit, int npublic) {
  Xyzz<FqTag> acc = xyzz_inf<FqTag>();
#pragma unroll 1
  for (int b = 255; b >= 0; --b) {
    xyzz_dbl(acc);
#pragma unroll 1
    for (int j = 0; j < npublic; ++j)
      if (bit(j, b)) xyzz_madd(acc, ic(j + 1));
  }
  xyzz_madd(acc, ic(0));
  return xyzz_to_affine(acc);
}

}  // namespace gs
