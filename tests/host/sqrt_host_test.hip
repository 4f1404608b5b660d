// Host-side unit-test driver for go-snark-study_amd/csrc/sqrt.h (the same __host__ __device__ source the kernels of point_codec.hip
// run), driven by tests/test_sqrt_host.py against Python integers.
// Input, one request per line, values in hex, standard form:
//   fq a        ->  "<ok> <y> <largest>": ok = fq_sqrt's verdict, y the value it returned, largest = fq_is_largest(y) (0 / 1)
//   fq2 a0 a1   ->  "<ok> <y0> <y1> <largest>": the same for fq2_sqrt and fq2_is_largest
//   big a       ->  "<largest>": fq_is_largest(a) alone
//   big2 a0 a1  ->  "<largest>": fq2_is_largest(a) alone
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "../../go-snark-study_amd/csrc/sqrt.h"

using namespace gs;

static Fe<ModQ, 2> rd(std::istringstream& ss) {
  std::string s;
  ss >> s;
  uint32_t w[8];
  memset(w, 0, sizeof(w));
  const int n = (int)s.size();
  for (int i = 0; i < n; ++i) {
    const char c = s[n - 1 - i];
    const uint32_t v = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : c - 'A' + 10;
    if (i / 8 < 8) w[i / 8] |= v << (4 * (i % 8));
  }
  return to_mont(unpack32<ModQ>(w));
}
static std::string hex_of(const Fe<ModQ, 2>& mont) {
  uint32_t w[8];
  pack32<ModQ>(from_mont(mont), w);
  char buf[80];
  snprintf(buf, sizeof buf, "%08x%08x%08x%08x%08x%08x%08x%08x", w[7], w[6], w[5], w[4], w[3], w[2], w[1], w[0]);
  return buf;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    std::string op;
    ss >> op;
    if (op == "fq") {
      Fe<ModQ, 2> y;
      const bool ok = fq_sqrt(rd(ss), y);
      std::cout << (ok ? 1 : 0) << " " << hex_of(y) << " " << (fq_is_largest(y) ? 1 : 0) << "\n";
    } else if (op == "fq2") {
      Fq2e<2> a, y;
      a.c0 = rd(ss); a.c1 = rd(ss);
      const bool ok = fq2_sqrt(a, y);
      std::cout << (ok ? 1 : 0) << " " << hex_of(y.c0) << " " << hex_of(y.c1) << " " << (fq2_is_largest(y) ? 1 : 0) << "\n";
    } else if (op == "big") {
      std::cout << (fq_is_largest(rd(ss)) ? 1 : 0) << "\n";
    } else if (op == "big2") {
      Fq2e<2> a;
      a.c0 = rd(ss); a.c1 = rd(ss);
      std::cout << (fq2_is_largest(a) ? 1 : 0) << "\n";
    } else {
      std::cout << "?\n";
    }
  }
  return 0;
}
