// Host-side unit-test driver for go-snark-study_amd/csrc/g2_subgroup.h (the same __host__ __device__ source the kernel of
// g2_subgroup.hip runs), driven by tests/test_g2_subgroup_host.py against oracle/ref_py.py.
// Input, one request per line, coordinates in hex, standard form, "inf" for the point at infinity:
//   member x0 x1 y0 y1   ->  "<a> <b>": a = g2_in_subgroup of g2_subgroup.h, b = the independent 4 x 64-bit one of pairing.h (0 / 1)
//   psi x0 x1 y0 y1      ->  the affine coordinates of g2_psi(point), or "inf"
//   psixyzz x0 x1 y0 y1  ->  psi(2 * point) through the XYZZ overload (the doubling gives it denominators), in affine form
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "../../go-snark-study_amd/csrc/g2_subgroup.h"
#include "../../go-snark-study_amd/csrc/pairing.h"

using namespace gs;

static void parse_hex(const std::string& s, uint32_t (&w)[8]) {
  memset(w, 0, sizeof(w));
  int n = (int)s.size();
  for (int i = 0; i < n; ++i) {
    char c = s[n - 1 - i];
    uint32_t v = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : c - 'A' + 10;
    if (i / 8 < 8) w[i / 8] |= v << (4 * (i % 8));
  }
}
static std::string hex_of(const Fe<ModQ, 1>& mont) {
  uint32_t w[8];
  pack32<ModQ>(from_mont(mont), w);
  char buf[80];
  snprintf(buf, sizeof buf, "%08x%08x%08x%08x%08x%08x%08x%08x", w[7], w[6], w[5], w[4], w[3], w[2], w[1], w[0]);
  return buf;
}
static std::string show(const Affine<Fq2Tag>& a) {
  if (is_inf(a)) return "inf";
  return hex_of(a.x.c0) + " " + hex_of(a.x.c1) + " " + hex_of(a.y.c0) + " " + hex_of(a.y.c1);
}

// one point in both representations
struct Both {
  Affine<Fq2Tag> eng;
  pairing::G2Aff host;
};
static Both rd_point(std::istringstream& ss) {
  Both b;
  b.eng.x = fq2_zero<1>(); b.eng.y = fq2_zero<1>();
  b.host = pairing::G2Aff{};
  b.host.inf = true;
  std::string h[4];
  ss >> h[0];
  if (h[0] == "inf") return b;
  ss >> h[1] >> h[2] >> h[3];
  Fe<ModQ, 1> e[4];
  pairing::Fp f[4];
  for (int k = 0; k < 4; ++k) {
    uint32_t w[8];
    parse_hex(h[k], w);
    e[k] = canon(to_mont(unpack32<ModQ>(w)));
    uint64_t w64[4];
    for (int i = 0; i < 4; ++i) w64[i] = (uint64_t)w[2 * i] | ((uint64_t)w[2 * i + 1] << 32);
    f[k] = pairing::fp_from_std(w64);
  }
  b.eng.x.c0 = e[0]; b.eng.x.c1 = e[1]; b.eng.y.c0 = e[2]; b.eng.y.c1 = e[3];
  b.host = pairing::G2Aff{{f[0], f[1]}, {f[2], f[3]}, false};
  return b;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    std::string op;
    ss >> op;
    const Both p = rd_point(ss);
    if (op == "member") {
      std::cout << (g2_in_subgroup(p.eng) ? 1 : 0) << " " << (pairing::g2_in_subgroup(p.host) ? 1 : 0) << "\n";
    } else if (op == "psi") {
      std::cout << show(g2_psi(p.eng)) << "\n";
    } else if (op == "psixyzz") {
      Xyzz<Fq2Tag> t = xyzz_from_affine(p.eng);
      xyzz_dbl(t);                                       // ZZ, ZZZ != 1: the overload has denominators to conjugate
      g2_psi(t);
      std::cout << show(xyzz_to_affine(t)) << "\n";
    } else {
      std::cout << "?\n";
    }
  }
  return 0;
}
