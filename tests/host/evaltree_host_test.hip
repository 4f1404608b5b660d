// Host-side replay of the evaluation-basis derivation (go-snark-study_amd/csrc/ecntt.hip, pk_derive_eval_impl) over Fr SCALARS in
// place of points, with the index arithmetic the kernels use (csrc/evaltree.h): the same buffers (sequences in slots of 2^level, the
// two products of a parent in slots of the parent's size, the children's spectra in the same layout), the same per-level steps
// (transform every slot, fork every spectrum element to both children, transform back, cut the windows), the transforms done as
// plain O(N^2) sums.  The map is linear, so what holds for scalars holds for points.  Driven from tests/test_evaltree_host.py, which
// computes the rows of the definition with Python integers.
// Protocol: one request per line on stdin:  <n> <hex h[0]> .. <hex h[n-1]>   ->   one line:  <hex E[0]> .. <hex E[n-1]>
#include <cstdio>
#include <cstring>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>
#include "../../go-snark-study_amd/csrc/evaltree.h"

using namespace gs;
using F = Fe<ModR, 2>;          // Montgomery form

static F f_small(uint64_t v) {
  uint32_t w[8] = {(uint32_t)v, (uint32_t)(v >> 32), 0, 0, 0, 0, 0, 0};
  return to_mont(unpack32<ModR>(w));
}
static F f_add(const F& a, const F& b) { return reduce2(add(a, b)); }
static F f_sub(const F& a, const F& b) { return reduce2(sub(a, b)); }
static F f_hex(const std::string& s) {
  uint32_t w[8];
  memset(w, 0, sizeof(w));
  const int n = (int)s.size();
  for (int i = 0; i < n && i < 64; ++i) {
    const char c = s[n - 1 - i];
    const uint32_t v = (c >= '0' && c <= '9') ? c - '0' : (c >= 'a' && c <= 'f') ? c - 'a' + 10 : c - 'A' + 10;
    w[i / 8] |= v << (4 * (i % 8));
  }
  return to_mont(unpack32<ModR>(w));
}
static std::string hex_of(const F& a) {
  uint32_t w[8];
  pack32<ModR>(from_mont(a), w);
  char buf[80];
  snprintf(buf, sizeof buf, "%08x%08x%08x%08x%08x%08x%08x%08x", w[7], w[6], w[5], w[4], w[3], w[2], w[1], w[0]);
  return buf;
}
// omega_N^(+-1), N = 2^logn
static F root(int logn, bool inverse) {
  F w;
  for (int i = 0; i < NL; ++i) w.l[i] = inverse ? ModR::omega28_inv_mont(i) : ModR::omega28_mont(i);
  for (int i = 0; i < ModR::kTwoAdicity - logn; ++i) w = sqr(w);
  return w;
}
// every slot of 2^level elements of x -> its transform (natural order in and out; both sides of a product use the same order)
static void transform_slots(std::vector<F>& x, int level, bool inverse) {
  const size_t N = (size_t)1 << level;
  const F w = root(level, inverse);
  std::vector<F> pw(N), out(N);
  pw[0] = f_small(1);
  for (size_t i = 1; i < N; ++i) pw[i] = mul(pw[i - 1], w);
  for (size_t s = 0; s < x.size(); s += N) {
    for (size_t k = 0; k < N; ++k) {
      F acc = f_small(0);
      for (size_t i = 0; i < N; ++i) acc = f_add(acc, mul(x[s + i], pw[(i * k) & (N - 1)]));
      out[k] = acc;
    }
    for (size_t k = 0; k < N; ++k) x[s + k] = out[k];
  }
}

static std::vector<F> derive(uint32_t n, const std::vector<F>& h) {
  int L = 0;
  while (((size_t)1 << L) < n) ++L;
  const size_t total = (size_t)1 << L;
  // reversed node polynomials rev(M) = prod (1 - x_j x), level by level; a padding leaf is the polynomial 1
  std::vector<std::vector<std::vector<F>>> rev(L + 1);
  rev[0].resize(total);
  for (uint32_t j = 0; j < total; ++j) {
    rev[0][j] = {f_small(1)};
    if (et_real(n, 0, j)) rev[0][j].push_back(f_sub(f_small(0), f_small((uint64_t)n + 1 + j)));
  }
  for (int l = 1; l <= L; ++l) {
    rev[l].resize(total >> l);
    for (uint32_t b = 0; b < (total >> l); ++b) {
      const auto &a = rev[l - 1][et_child(b, 0)], &c = rev[l - 1][et_child(b, 1)];
      std::vector<F> o(a.size() + c.size() - 1, f_small(0));
      for (size_t i = 0; i < a.size(); ++i)
        for (size_t j = 0; j < c.size(); ++j) o[i + j] = f_add(o[i + j], mul(a[i], c[j]));
      if (o.size() != (size_t)et_real(n, l, b) + 1) { fprintf(stderr, "degree of node (%d, %u) is not its number of real leaves\n", l, b); exit(2); }
      rev[l][b] = o;
    }
  }
  std::vector<F> cur(total, f_small(0)), prod(2 * total), spec(2 * total);
  for (uint32_t i = 0; i < n; ++i) cur[i] = h[i];
  for (int level = L; level >= 1; --level) {
    const size_t N = (size_t)1 << level;
    // the level's spectra: child b's reversed polynomial in slot b of the parent's size, / N
    const F inv_n = inv(f_small(N));
    for (size_t i = 0; i < 2 * total; ++i) spec[i] = f_small(0);
    for (uint32_t b = 0; b < (2 * total) >> level; ++b)
      for (size_t t = 0; t < rev[level - 1][b].size(); ++t) spec[et_slot(level, b) + t] = mul(rev[level - 1][b][t], inv_n);
    transform_slots(spec, level, false);
    transform_slots(cur, level, false);
    for (uint32_t e = 0; e < total; ++e) {                       // k_ec_fork
      const uint32_t p = e >> level, in = e & ((1u << level) - 1u);
      const size_t o0 = et_slot(level, et_child(p, 0)) + in, o1 = et_slot(level, et_child(p, 1)) + in;
      prod[o0] = et_real(n, level - 1, et_child(p, 0)) ? mul(spec[et_sibling_elem(level, o0)], cur[e]) : f_small(0);
      prod[o1] = et_real(n, level - 1, et_child(p, 1)) ? mul(spec[et_sibling_elem(level, o1)], cur[e]) : f_small(0);
    }
    transform_slots(prod, level, true);
    for (uint32_t i = 0; i < total; ++i) {                       // k_ec_window
      const uint32_t child = i >> (level - 1), k = i & ((1u << (level - 1)) - 1u);
      cur[i] = k < et_real(n, level - 1, child) ? prod[et_slot(level, child) + et_window(n, level, child >> 1, (int)(child & 1u)) + k] : f_small(0);
    }
  }
  // leaves: E_j = c[0] / M'(x_j),  M'(n + j) = (-1)^(n-j) (j-1)! (n-j)!
  std::vector<F> fact(n + 1);
  fact[0] = f_small(1);
  for (uint32_t i = 1; i <= n; ++i) fact[i] = mul(fact[i - 1], f_small(i));
  std::vector<F> e(n);
  for (uint32_t j = 1; j <= n; ++j) {
    F d = mul(fact[j - 1], fact[n - j]);
    if ((n - j) & 1u) d = f_sub(f_small(0), d);
    e[j - 1] = mul(cur[j - 1], inv(d));
  }
  return e;
}

int main() {
  std::string line;
  while (std::getline(std::cin, line)) {
    std::istringstream ss(line);
    uint32_t n = 0;
    ss >> n;
    std::vector<F> h(n);
    std::string tok;
    for (uint32_t i = 0; i < n; ++i) { ss >> tok; h[i] = f_hex(tok); }
    const std::vector<F> e = derive(n, h);
    for (uint32_t i = 0; i < n; ++i) std::cout << (i ? " " : "") << hex_of(e[i]);
    std::cout << "\n";
  }
  return 0;
}
