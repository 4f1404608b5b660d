// Host-compiled view of the index and exponent functions of the power-of-two domain QAP (go-snark-study_amd/csrc/domain.h): what the
// table kernel (k_domain_table), the coefficient gather (k_domain_coeffs) and the evaluation-basis derivation (ecntt.hip) compute per
// slot.  Driven from tests/test_domain_host.py, which checks every line against Python's pow.
// Protocol: one request per line on stdin:  <k>   ->   one line of 2^k records  slot:frequency:coset_exp:derive_exp:coeff_slot:hex(g^coset_exp / m)
#include <cstdio>
#include <iostream>
#include <string>
#include "../../go-snark-study_amd/csrc/domain.h"

using namespace gs;
using F = Fe<ModR, 2>;

static F f_small(uint64_t v) {
  uint32_t w[8] = {(uint32_t)v, (uint32_t)(v >> 32), 0, 0, 0, 0, 0, 0};
  return to_mont(unpack32<ModR>(w));
}
static std::string hex_of(const F& a) {
  uint32_t w[8];
  pack32<ModR>(from_mont(a), w);
  char buf[80];
  snprintf(buf, sizeof buf, "%08x%08x%08x%08x%08x%08x%08x%08x", w[7], w[6], w[5], w[4], w[3], w[2], w[1], w[0]);
  return buf;
}

int main() {
  int k;
  while (std::cin >> k) {
    if (k < 1 || k > kDomainMaxLog2) { std::cout << "bad\n"; continue; }
    const F g = dom_coset_gen(k), inv_m = inv(f_small(1ull << k));
    for (uint32_t p = 0; p < (1u << k); ++p) {
      const uint32_t e = dom_coset_exp(k, p);
      std::cout << (p ? " " : "") << p << ":" << dom_bitrev(k, p) << ":" << e << ":" << dom_derive_exp(k, p) << ":" << dom_coeff_slot(k, p) << ":"
                << hex_of(dom_scaled_pow(g, e, inv_m));
    }
    std::cout << "\n";
  }
  return 0;
}
