// Host-compiled view of the two number conversions of a .zkey (go-snark-study_amd/csrc/zkey_convert.h): a coordinate in Montgomery form to
// the base 2^256 -> the engine's form (base 2^261), a coefficient times 2^512 -> its value.  Driven from tests/test_zkey_host.py, which
// checks every line against Python integers.
// Protocol: one request per line on stdin:  <q|r> <64 hex digits, big-endian>   ->   <below modulus 0|1> <hex of the result's STANDARD value>
// (q: the engine element taken out of Montgomery form, i.e. input * 2^-256 mod q;  r: input * 2^-512 mod r)
#include <cstdio>
#include <iostream>
#include <string>
#include "../../go-snark-study_amd/csrc/zkey_convert.h"

using namespace gs;

static bool parse(const std::string& hex, uint32_t (&w)[8]) {
  if (hex.size() != 64) return false;
  for (int i = 0; i < 8; ++i) w[i] = (uint32_t)std::stoul(hex.substr(64 - 8 * (i + 1), 8), nullptr, 16);
  return true;
}
static std::string hex_of(const uint32_t (&w)[8]) {
  char buf[80];
  snprintf(buf, sizeof buf, "%08x%08x%08x%08x%08x%08x%08x%08x", w[7], w[6], w[5], w[4], w[3], w[2], w[1], w[0]);
  return buf;
}

int main() {
  std::string which, hex;
  while (std::cin >> which >> hex) {
    uint32_t w[8], o[8];
    if (!parse(hex, w) || (which != "q" && which != "r")) { std::cout << "bad\n"; continue; }
    if (which == "q") {
      pack32<ModQ>(from_mont(zkey_coord_to_engine(w)), o);
      std::cout << (zkey_words_below<ModQ>(w) ? 1 : 0) << " " << hex_of(o) << "\n";
    } else {
      pack32<ModR>(zkey_coef_to_std(w), o);
      std::cout << (zkey_words_below<ModR>(w) ? 1 : 0) << " " << hex_of(o) << "\n";
    }
  }
  return 0;
}
