// Host check of the index arithmetic of the all-levels transform (levels_plan.h), compiled for the CPU.  For every 0 <= lo <= hi <= 10:
//   the points of the workspace are the levels lo .. hi, each index of each level once (lv_point_level / lv_point_within);
//   for every span 2^s the launch visits each (level, butterfly) with 2^p >= 2 * 2^s exactly once and nothing else, both operands lie
//   inside their level's slot and are the pair k_ec_stage takes at that level, the twiddle index is below 2^(hi-1) and names the
//   level's own twiddle;
//   and the whole schedule -- bit-reversed load, 2^(-p), the stages in launch order -- run on integers mod 12289 gives every level's
//   inverse transform by its O(n^2) definition.
#include <cstdint>
#include <cstdio>
#include <vector>
#include "../../go-snark-study_amd/csrc/domain.h"
#include "../../go-snark-study_amd/csrc/levels_plan.h"
using namespace gs;

static const uint32_t Q = 12289;      // 2^12 * 3 + 1, 11 generates the units
static uint32_t mpow(uint32_t b, uint32_t e) {
  uint64_t r = 1, x = b % Q;
  for (; e; e >>= 1) { if (e & 1) r = r * x % Q; x = x * x % Q; }
  return (uint32_t)r;
}

static int check(int lo, int hi, long& visited) {
  const uint32_t total = lv_total(lo, hi), top = 1u << hi;
  // the points
  std::vector<int> seen(total, 0);
  for (int p = lo; p <= hi; ++p)
    for (uint32_t i = 0; i < (1u << p); ++i) {
      const uint32_t q = lv_level_start(lo, p) + i;
      if (q >= total || lv_point_level(lo, q) != p || lv_point_within(lo, q) != i) return 1;
      seen[q] += 1;
    }
  for (uint32_t q = 0; q < total; ++q)
    if (seen[q] != 1) return 2;
  // the transform on integers: P[i] = 3 i^2 + 7 i + 1, the last point of the top level missing (the short-array rule) when hi is odd
  const uint32_t n = (hi & 1) ? top - 1 : top;
  std::vector<uint32_t> P(top), ws(total), tw(top / 2 ? top / 2 : 1);
  for (uint32_t i = 0; i < top; ++i) P[i] = i < n ? (3 * i * i + 7 * i + 1) % Q : 0;
  const uint32_t wi = mpow(mpow(11, (Q - 1) / top), Q - 2), half = mpow(2, Q - 2);
  for (uint32_t e = 0; e < top / 2; ++e) tw[e] = mpow(wi, e);
  for (uint32_t q = 0; q < total; ++q) {
    const int p = lv_point_level(lo, q);
    const uint32_t i = dom_bitrev(p, lv_point_within(lo, q));
    ws[q] = (uint32_t)((uint64_t)(i < n ? P[i] : 0) * mpow(half, (uint32_t)p) % Q);
  }
  for (int s = 0; s < hi; ++s) {
    const uint32_t nbf = lv_stage_count(lo, hi, s), h = 1u << s;
    std::vector<int> hit(total, 0);
    for (uint32_t t = 0; t < nbf; ++t) {
      const LvButterfly f = lv_butterfly(lo, hi, s, t);
      const int p = f.level;
      if (p < lo || p > hi || (1u << p) < 2 * h) return 3;
      const uint32_t start = lv_level_start(lo, p), m = 1u << p;
      if (f.i0 < start || f.i1 >= start + m || f.i1 != f.i0 + h) return 4;
      const uint32_t x = f.i0 - start, j = x & (h - 1);
      if (x & h) return 5;                                                // i0 is the lower operand of its pair
      if (top >= 2 && f.twiddle >= top / 2) return 6;
      if (f.twiddle != j * (top / (2 * h))) return 7;                      // = j * m / 2h of the level's table, times 2^hi / m
      hit[f.i0] += 1;
      hit[f.i1] += 1;
      const uint32_t a = ws[f.i0], b = (uint32_t)((uint64_t)ws[f.i1] * tw[f.twiddle] % Q);
      ws[f.i0] = (a + b) % Q;
      ws[f.i1] = (a + Q - b) % Q;
      ++visited;
    }
    for (int p = lo; p <= hi; ++p)
      for (uint32_t i = 0; i < (1u << p); ++i)
        if (hit[lv_level_start(lo, p) + i] != ((1u << p) >= 2 * h ? 1 : 0)) return 8;
  }
  for (int p = lo; p <= hi; ++p) {
    const uint32_t m = 1u << p, wp = mpow(wi, top / m), inv_m = mpow(m % Q, Q - 2);
    for (uint32_t j = 0; j < m; ++j) {
      uint64_t acc = 0;
      for (uint32_t i = 0; i < m; ++i) acc = (acc + (uint64_t)P[i] * mpow(wp, (uint32_t)((uint64_t)i * j % m))) % Q;
      if (ws[lv_level_start(lo, p) + j] != acc * inv_m % Q) return 9;
    }
  }
  return 0;
}

int main() {
  long visited = 0;
  int pairs = 0;
  for (int hi = 0; hi <= 10; ++hi)
    for (int lo = 0; lo <= hi; ++lo) {
      const int rc = check(lo, hi, visited);
      if (rc) { printf("FAIL lo %d hi %d: rule %d\n", lo, hi, rc); return 1; }
      ++pairs;
    }
  printf("OK %d pairs %ld butterflies\n", pairs, visited);
  return 0;
}
