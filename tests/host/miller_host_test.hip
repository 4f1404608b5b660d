// Host-side unit-test driver for go-snark-study_amd/csrc/fq12.h and miller.h (the same __host__ __device__ source the kernels of
// pairing_device.hip run), driven by tests/test_miller_host.py against the 4 x 64-bit tower and pairing of pairing.h.
// Input, one request per line, every field element in hex, standard form; an Fq12 is its 12 coordinates in gs_pairing's order:
//   mul a[12] b[12]          ->  fq12.h's a b, then pairing.h's f12_mul                                   (12 + 12 words)
//   sqr a[12]                ->  fq12.h's a^2, then pairing.h's f12_sqr
//   line a[12] l[6]          ->  fq12.h's a (l0 + l1 w + l2 w^3), then pairing.h's f12_mul by that element written out, then
//                                pairing.h's f12_mul_line with y = the real part of l0 (the caller compares it when l0 is in Fq)
//   pair P Q                 ->  final_exponentiation(miller_loop(P, Q)) through miller.h, then pairing.h's pairing (one for an
//                                infinite member).  P is "x y" or "inf", Q is "x0 x1 y0 y1" or "inf".
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include "../../go-snark-study_amd/csrc/miller.h"
#include "../../go-snark-study_amd/csrc/pairing.h"

using namespace gs;
namespace H = gs::pairing;

static void parse_hex(const std::string& s, uint64_t (&w)[4]) {
  memset(w, 0, sizeof(w));
  int n = (int)s.size();
  for (int i = 0; i < n; ++i) {
    char c = s[n - 1 - i];
    uint64_t v = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : c - 'A' + 10;
    if (i / 16 < 4) w[i / 16] |= v << (4 * (i % 16));
  }
}
static std::string hex_words(const uint64_t* w, int count) {
  std::string out;
  char buf[80];
  for (int i = 0; i < count; ++i) {
    snprintf(buf, sizeof buf, "%016llx%016llx%016llx%016llx", (unsigned long long)w[4 * i + 3], (unsigned long long)w[4 * i + 2],
             (unsigned long long)w[4 * i + 1], (unsigned long long)w[4 * i]);
    if (i) out += " ";
    out += buf;
  }
  return out;
}
static void rd_words(std::istringstream& ss, uint64_t* w, int count) {
  for (int i = 0; i < count; ++i) {
    std::string h;
    ss >> h;
    uint64_t t[4];
    parse_hex(h, t);
    memcpy(w + 4 * i, t, 32);
  }
}
static H::Fp2 host_f2(const uint64_t* w) { return H::Fp2{H::fp_from_std(w), H::fp_from_std(w + 4)}; }
static std::string show(const H::Fp12& f) {
  uint64_t w[48];
  H::f12_to_std(f, w);
  return hex_words(w, 12);
}
static std::string show(const Fq12& f) {
  uint64_t w[48];
  f12_to_std(f, w);
  return hex_words(w, 12);
}
static Fe<ModQ, 1> eng_fq(const uint64_t* w) {
  uint32_t w32[8];
  for (int i = 0; i < 4; ++i) { w32[2 * i] = (uint32_t)w[i]; w32[2 * i + 1] = (uint32_t)(w[i] >> 32); }
  return canon(to_mont(unpack32<ModQ>(w32)));
}
static Fq2e<2> eng_f2(const uint64_t* w) { return {relax<2>(eng_fq(w)), relax<2>(eng_fq(w + 4))}; }

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    std::string op;
    ss >> op;
    if (op == "mul" || op == "sqr") {
      uint64_t a[48], b[48];
      rd_words(ss, a, 12);
      Fq12 fa, fb;
      f12_from_std(fa, a);
      if (op == "mul") {
        rd_words(ss, b, 12);
        f12_from_std(fb, b);
        f12_mul(fa, fb);
        std::cout << show(fa) << " " << show(H::f12_mul(H::f12_from_std(a), H::f12_from_std(b))) << "\n";
      } else {
        f12_sqr(fa);
        std::cout << show(fa) << " " << show(H::f12_sqr(H::f12_from_std(a))) << "\n";
      }
    } else if (op == "line") {
      uint64_t a[48], l[24];
      rd_words(ss, a, 12);
      rd_words(ss, l, 6);
      Fq12 fa;
      f12_from_std(fa, a);
      f12_mul_line(fa, eng_f2(l), eng_f2(l + 8), eng_f2(l + 16));
      H::Fp12 g{H::Fp6{host_f2(l), H::f2_zero(), H::f2_zero()}, H::Fp6{host_f2(l + 8), host_f2(l + 16), H::f2_zero()}};
      std::cout << show(fa) << " " << show(H::f12_mul(H::f12_from_std(a), g)) << " "
                << show(H::f12_mul_line(H::f12_from_std(a), H::fp_from_std(l), host_f2(l + 8), host_f2(l + 16))) << "\n";
    } else if (op == "pair") {
      Affine<FqTag> p;
      Affine<Fq2Tag> q;
      p.x = fe_zero<ModQ, 1>(); p.y = fe_zero<ModQ, 1>();
      q.x = fq2_zero<1>(); q.y = fq2_zero<1>();
      H::G1Aff hp{};
      H::G2Aff hq{};
      hp.inf = hq.inf = true;
      std::string tok;
      std::streampos at = ss.tellg();
      ss >> tok;
      if (tok != "inf") {
        ss.seekg(at);
        uint64_t w[8];
        rd_words(ss, w, 2);
        p.x = eng_fq(w); p.y = eng_fq(w + 4);
        hp = H::G1Aff{H::fp_from_std(w), H::fp_from_std(w + 4), false};
      }
      at = ss.tellg();
      ss >> tok;
      if (tok != "inf") {
        ss.seekg(at);
        uint64_t w[16];
        rd_words(ss, w, 4);
        q.x = {eng_fq(w), eng_fq(w + 4)}; q.y = {eng_fq(w + 8), eng_fq(w + 12)};
        hq = H::G2Aff{host_f2(w), host_f2(w + 8), false};
      }
      Fq12 f;
      miller_loop(f, p, q);
      uint64_t fw[48];
      f12_to_std(f, fw);
      H::Fp12 want;
      if (!H::multi_miller_loop({hp}, {hq}, want)) { std::cout << "degenerate\n"; continue; }
      std::cout << show(H::final_exponentiation(H::f12_from_std(fw))) << " " << show(H::final_exponentiation(want)) << "\n";
    } else {
      std::cout << "?\n";
    }
  }
  return 0;
}
