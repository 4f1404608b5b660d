// The index arithmetic of a transform in the group over EVERY power-of-two domain at once (ptau_levels.hip: the prepared sections of a
// powers-of-tau transcript).  The levels lo .. hi of one section share one workspace: level p, the transform of the first 2^p points,
// sits at point index 2^p - 2^lo, so the workspace holds 2^(hi+1) - 2^lo points.  A decimation-in-time stage of span h = 2^s has the
// same twiddles at every level (the butterfly j of a block takes omega_(2^p)^(-j 2^p / 2h) = omega_(2^hi)^(-j 2^hi / 2h)), so ONE launch
// carries the stage of that span for all levels with 2^p >= 2h.  Level p has 2^(p-1) butterflies per stage: numbered from the lowest
// level that takes part, butterfly t of the launch is number t' = t + base, base = max(2^s, 2^(lo-1)), of the sequence in which level p
// owns [2^(p-1), 2^p) -- the top bit of t' gives the level, the rest the butterfly within it.
// The kernels and a host-compiled test (tests/host/levels_plan_host_test.hip) share the functions below.
#pragma once
#include <stdint.h>

#include "fp29.h"

namespace gs {

constexpr int kLevelsMaxLog2 = 27;      // the top level: 2^27 points, as one transform (domain.h)

GS_HD int lv_floor_log2(uint32_t x) {      // x >= 1
  int b = 0;
  while (x >>= 1) ++b;
  return b;
}
// points of the workspace, and where level p starts in it
GS_HD uint32_t lv_total(int lo, int hi) { return (2u << hi) - (1u << lo); }
GS_HD uint32_t lv_level_start(int lo, int p) { return (1u << p) - (1u << lo); }
// workspace index q -> its level, and the index within the level
GS_HD int lv_point_level(int lo, uint32_t q) { return lv_floor_log2(q + (1u << lo)); }
GS_HD uint32_t lv_point_within(int lo, uint32_t q) {
  const uint32_t v = q + (1u << lo);
  return v - (1u << lv_floor_log2(v));
}
// the stage of span 2^s (s < hi): number of the first butterfly, and how many there are over the levels max(lo, s + 1) .. hi
GS_HD uint32_t lv_stage_base(int lo, int s) {
  const uint32_t a = 1u << s, b = lo > 0 ? 1u << (lo - 1) : 0u;
  return a > b ? a : b;
}
GS_HD uint32_t lv_stage_count(int lo, int hi, int s) { return (1u << hi) - lv_stage_base(lo, s); }

struct LvButterfly {
  int level;             // p
  uint32_t i0, i1;       // workspace indices of the two operands
  uint32_t twiddle;      // index into the 2^(hi-1) powers of omega_(2^hi)^(-1); 0 = no multiplication
};
// butterfly t < lv_stage_count(lo, hi, s) of the stage of span 2^s
GS_HD LvButterfly lv_butterfly(int lo, int hi, int s, uint32_t t) {
  const uint32_t tp = t + lv_stage_base(lo, s), h = 1u << s;
  LvButterfly b;
  b.level = lv_floor_log2(tp) + 1;
  const uint32_t u = tp - (1u << (b.level - 1)), j = u & (h - 1);
  b.i0 = lv_level_start(lo, b.level) + (u - j) * 2 + j;
  b.i1 = b.i0 + h;
  b.twiddle = j << (hi - 1 - s);
  return b;
}

}  // namespace gs
