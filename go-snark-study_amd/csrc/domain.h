// The QAP over a power-of-two domain (snarkjs / circom Groth16 keys), next to the reference's QAP over the nodes 1..n.
//
//   m = 2^k, 1 <= k <= 27;   omega = 5^((r-1)/m)  (the polynomial engine's own root: omega28^(2^(28-k)));   row c of the system sits at omega^c
//   g = 5^((r-1)/(2m)):  g^2 = omega, g^m = -1;   the coset  y_j = g omega^j, j < m
//   a, b, c: the interpolants of degree < m of the rows of A w, B w, C w (n <= m constraints, rows n..m-1 are empty)
//   Z = x^m - 1,   H = floor((a b - c) / Z) = coefficients m .. 2m-2 of a b - c  (exact for a satisfying witness; then deg H <= m - 2)
//   Z(y_j) = g^m - 1 = -2 for every j.
// With T = the first m points of the key's h array (hExps) and u_j = (a b - c)(y_j):
//   sum_j u_j E_j = sum_i h_i T_i     for     E_j = -(1 / (2m)) sum_{i<m} y_j^(-i) T_i
// (u_j = -2 H(y_j), and (1/m) sum_j y_j^(l-i) = [l = i] for |l - i| < m).  E is the COSET EVALUATION-BASIS array, kept and exchanged in
// natural order, j <-> y_j.
//
// The coset extension of one value vector v (natural order, v_c at omega^c), with the engine's transforms (ntt_forward: X[f] =
// sum_c v_c omega^(cf), frequency f in slot bitrev(f); ntt_inverse_unscaled: out_t = sum_f X[f] omega^(-ft) from that order):
//   the interpolant's coefficient i is X[(-i) mod m] / m, so its value at y_t is  sum_f X[f] (g^((-f) mod m) / m) omega^(-ft):
//   ntt_forward, slot of frequency f times g^((-f) mod m) / m (while the first inverse pass loads), ntt_inverse_unscaled.
// E itself is one transform of size m in the group over the sequence (-(1/(2m)) g^(-i)) T_i with the root omega^(-1): the terms are
// loaded into the slots bitrev(i) and the decimation-in-time stages leave E in natural order.
// The functions below say which frequency a slot holds and which power of g belongs to it; the table kernel (poly_kernels.h), the
// derivation (ecntt.hip) and a host-compiled test (tests/host/domain_host_test.hip) share them.
#pragma once
#include <stdint.h>

#include "fp29.h"

namespace gs {

constexpr int kDomainMaxLog2 = 27;      // 2m <= 2^28, the 2-adicity of Fr

// the low k bits of p reversed: the frequency (or sequence index) held by slot p of a bit-reversed array of 2^k
GS_HD uint32_t dom_bitrev(int k, uint32_t p) {
  uint32_t r = 0;
  for (int b = 0; b < k; ++b) r |= ((p >> b) & 1u) << (k - 1 - b);
  return r;
}
// slot of coefficient i of the interpolant in the bit-reversed spectrum: the slot of frequency (-i) mod m
GS_HD uint32_t dom_coeff_slot(int k, uint32_t i) { return dom_bitrev(k, (0u - i) & ((1u << k) - 1u)); }
// exponent e of g for slot p of the coset-extension spectrum: the slot is multiplied by g^e / m, e = (-f) mod m, f = bitrev(p)
GS_HD uint32_t dom_coset_exp(int k, uint32_t p) { return (0u - dom_bitrev(k, p)) & ((1u << k) - 1u); }
// exponent e of g for slot p of the derivation's input: the term i = bitrev(p) is multiplied by -(1/(2m)) g^e, e = (-i) mod 2m
GS_HD uint32_t dom_derive_exp(int k, uint32_t p) { return (0u - dom_bitrev(k, p)) & ((2u << k) - 1u); }
// scale * base^e (Montgomery base; the form of the result is the form of `scale`)
GS_HD Fe<ModR, 2> dom_scaled_pow(Fe<ModR, 2> base, uint32_t e, Fe<ModR, 2> scale) {
  for (; e != 0; e >>= 1) {
    if (e & 1u) scale = mul(scale, base);
    base = sqr(base);
  }
  return scale;
}
// g = 5^((r-1)/(2m)) for m = 2^k, Montgomery
GS_HD Fe<ModR, 2> dom_coset_gen(int k) {
  Fe<ModR, 2> w;
  for (int i = 0; i < NL; ++i) w.l[i] = ModR::omega28_mont(i);
  for (int i = 0; i < ModR::kTwoAdicity - (k + 1); ++i) w = sqr(w);
  return w;
}

}  // namespace gs
