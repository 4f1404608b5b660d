// The two number conversions of a snarkjs .zkey file (capi_zkey.hip), host and device: the file keeps every number in Montgomery
// form to the base 2^256, the engine to the base 2^261 (fp29.h), so each conversion is ONE Montgomery product by a constant.
//   coordinate   c = x 2^256 mod q  ->  x 2^261:   mont_mul(c, 2^266) = c 2^266 2^-261 = 32 c
//   coefficient  c = v 2^512 mod r  ->  v (standard form, what the CSR value arrays hold):   mont_mul(c, 2^-251) = c 2^-512
// tests/host/zkey_host_test.hip checks both against integer arithmetic.
#pragma once
#include <stdint.h>

#include "fp29.h"

namespace gs {

GS_HD Fe<ModQ, 1> zkey_coord_const() {       // 2^266 mod q
  const uint32_t k[NL] = {0x13349ca1u, 0x1a5d84a8u, 0x0a3e5cacu, 0x100249e0u, 0x12b951e8u, 0x0e92d304u, 0x14cb95b3u, 0x041b9d3du, 0x00058003u};
  Fe<ModQ, 1> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = k[i];
  return r;
}
GS_HD Fe<ModR, 1> zkey_coef_const() {        // 2^-251 mod r
  const uint32_t k[NL] = {0x162329b2u, 0x08c494b4u, 0x065a4275u, 0x10028af4u, 0x0d688ef0u, 0x164d60fcu, 0x0543c177u, 0x1d00fe7cu, 0x001802dfu};
  Fe<ModR, 1> r;
#pragma unroll
  for (int i = 0; i < NL; ++i) r.l[i] = k[i];
  return r;
}

// w < p as 256-bit numbers (8 little-endian words)
template <class M>
GS_HD bool zkey_words_below(const uint32_t (&w)[8]) {
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) borrow = (((uint64_t)w[i] - M::p32(i) - borrow) >> 32) & 1u;
  return borrow != 0;
}

// a coordinate of the file (any 256-bit word; the caller refuses words >= q) -> the engine's canonical Montgomery element
GS_HD Fe<ModQ, 1> zkey_coord_to_engine(const uint32_t (&w)[8]) { return canon(mul(unpack32<ModQ>(w), zkey_coord_const())); }
// a coefficient of the file (any 256-bit word) -> its value, canonical standard form
GS_HD Fe<ModR, 1> zkey_coef_to_std(const uint32_t (&w)[8]) { return canon(mul(unpack32<ModR>(w), zkey_coef_const())); }

}  // namespace gs
