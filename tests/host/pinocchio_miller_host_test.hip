// Host-side unit-test driver for the device code under gs_pinocchio_verify_each (go-snark-study_amd/csrc/miller.h: miller_loop_prepared,
// miller_loop_groth16, pinocchio_sums; finalexp.h), the same __host__ __device__ source the kernels of pairing_device.hip run, driven by
// tests/test_pinocchio_miller_host.py against pairing.h.  One request per line, every field element in hex, standard form; a G1 point is
// "x y" or "inf", a G2 point "x0 x1 y0 y1" or "inf".
//   prep3 P1 Q1 P2 Q2 P3 Q3  ->  final_exponentiation(miller_loop_prepared(...)): the lines of all three Q prepared (pairing.h,
//                                prepare_g2_lines), an infinite Q sets the pair's skip flag; then pairing.h's
//                                final_exponentiation(multi_miller_loop(...)) over the same pairs                        (12 + 12 words)
//   live3 P1 Q1 P2 Q2 P3 Q3  ->  the same with miller_loop_groth16: Q1 runs the projective steps, Q2 and Q3 are prepared
//   sums V A C               ->  pinocchio_sums: V + A, " | ", V + A + C, each "x y" or "inf"
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../go-snark-study_amd/csrc/finalexp.h"
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
// `count` field elements, or nothing when the next token is "inf"
static bool rd_point(std::istringstream& ss, uint64_t* w, int count) {
  for (int i = 0; i < count; ++i) {
    std::string h;
    ss >> h;
    if (i == 0 && h == "inf") return false;
    uint64_t t[4];
    parse_hex(h, t);
    memcpy(w + 4 * i, t, 32);
  }
  return true;
}
static H::Fp2 host_f2(const uint64_t* w) { return H::Fp2{H::fp_from_std(w), H::fp_from_std(w + 4)}; }
static std::string show(const H::Fp12& f) {
  const H::Fp2* c[6] = {&f.a0.c0, &f.a0.c1, &f.a0.c2, &f.a1.c0, &f.a1.c1, &f.a1.c2};
  uint64_t w[48];
  for (int i = 0; i < 6; ++i) { H::fp_to_std(c[i]->c0, w + 8 * i); H::fp_to_std(c[i]->c1, w + 8 * i + 4); }
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
static std::string show(const Affine<FqTag>& p) {
  if (is_inf(p)) return "inf";
  uint64_t w[8];
  uint32_t w32[8];
  pack32<ModQ>(from_mont(p.x), w32);
  for (int j = 0; j < 4; ++j) w[j] = (uint64_t)w32[2 * j] | ((uint64_t)w32[2 * j + 1] << 32);
  pack32<ModQ>(from_mont(p.y), w32);
  for (int j = 0; j < 4; ++j) w[4 + j] = (uint64_t)w32[2 * j] | ((uint64_t)w32[2 * j + 1] << 32);
  return hex_words(w, 2);
}
static Affine<FqTag> rd_g1(std::istringstream& ss, H::G1Aff* host = nullptr) {
  Affine<FqTag> p;
  p.x = fe_zero<ModQ, 1>(); p.y = fe_zero<ModQ, 1>();
  H::G1Aff hp{};
  hp.inf = true;
  uint64_t w[8];
  if (rd_point(ss, w, 2)) {
    p.x = eng_fq(w); p.y = eng_fq(w + 4);
    hp = H::G1Aff{H::fp_from_std(w), H::fp_from_std(w + 4), false};
  }
  if (host) *host = hp;
  return p;
}
static Affine<Fq2Tag> rd_g2(std::istringstream& ss, H::G2Aff* host) {
  Affine<Fq2Tag> q;
  q.x = fq2_zero<1>(); q.y = fq2_zero<1>();
  *host = H::G2Aff{};
  host->inf = true;
  uint64_t w[16];
  if (rd_point(ss, w, 4)) {
    q.x = {eng_fq(w), eng_fq(w + 4)}; q.y = {eng_fq(w + 8), eng_fq(w + 12)};
    *host = H::G2Aff{host_f2(w), host_f2(w + 8), false};
  }
  return q;
}
// prepared lines in standard form (pairing.h, prepare_g2_lines) as miller.h's loops read them
struct HostLines {
  std::vector<uint64_t> w;
  Fq2e<2> at(size_t off) const { return {relax<2>(eng_fq(w.data() + off)), relax<2>(eng_fq(w.data() + off + 4))}; }
  Fq2e<2> lambda(int k) const { return at(16 * (size_t)k); }
  Fq2e<2> c(int k) const { return at(16 * (size_t)k + 8); }
};

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    std::string op;
    ss >> op;
    if (op == "prep3" || op == "live3") {
      Affine<FqTag> p[3];
      Affine<Fq2Tag> q[3];
      H::G1Aff hp[3];
      H::G2Aff hq[3];
      HostLines lines[3];
      bool degenerate = false;
      for (int k = 0; k < 3; ++k) {
        p[k] = rd_g1(ss, &hp[k]);
        q[k] = rd_g2(ss, &hq[k]);
        lines[k].w.assign((size_t)H::kPreparedSteps * 16, 0);              // an infinite Q: the lines are read and not used
        if ((k > 0 || op == "prep3") && !hq[k].inf && !H::prepare_g2_lines(hq[k], lines[k].w)) degenerate = true;
      }
      H::Fp12 want;
      if (degenerate || !H::multi_miller_loop({hp[0], hp[1], hp[2]}, {hq[0], hq[1], hq[2]}, want)) { std::cout << "degenerate\n"; continue; }
      Fq12 f;
      Fq12Bank bank;
      if (op == "prep3") miller_loop_prepared(f, p[0], hq[0].inf, lines[0], p[1], hq[1].inf, lines[1], p[2], hq[2].inf, lines[2]);
      else miller_loop_groth16(f, p[0], q[0], p[1], hq[1].inf, lines[1], p[2], hq[2].inf, lines[2]);
      final_exponentiation(f, bank);
      std::cout << show(f) << " " << show(H::final_exponentiation(want)) << "\n";
    } else if (op == "sums") {
      const Affine<FqTag> v = rd_g1(ss), a = rd_g1(ss), c = rd_g1(ss);
      Affine<FqTag> xa, xac;
      pinocchio_sums(v, a, c, xa, xac);
      std::cout << show(xa) << " | " << show(xac) << "\n";
    } else {
      std::cout << "?\n";
    }
  }
  return 0;
}
