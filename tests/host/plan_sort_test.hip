// Host check of the sort plan's index arithmetic in msm_kernels.h, compiled for the CPU:
//   sort_block_of / sort_grid   every (window, slice, range) gets exactly one workgroup id, that id has id % 8 == window % 8 (one XCD
//                               per window), and the ids that pad W to a multiple of 8 are rejected;
//   sort_slice_terms / _groups  the slices of a padded digit row are consecutive, disjoint and cover every 8-term group of the row;
//   digit_encode / _decode      every digit of every window width survives the stored form (16-bit magnitude up to c = 17, 32-bit
//                               above, one skip and one sign bit).
#include <cstdio>
#include <vector>
#include "../../go-snark-study_amd/csrc/msm_kernels.h"
using namespace gs;
int main() {
  long maps = 0, rows = 0, digits = 0;
  for (int W : {8, 13, 15, 16, 17, 26})
    for (uint32_t S : {1u, 2u, 3u, 8u, 16u})
      for (uint32_t R : {1u, 2u, 3u, 8u, 16u}) {
        PlanParams pp{};
        pp.W = W; pp.S = S; pp.R = R;
        const uint32_t grid = sort_grid(pp);
        if (grid % 8u != 0 || grid < (uint32_t)W * S * R || grid >= ((uint32_t)W + 8u) * S * R) { printf("FAIL grid %u for W=%d S=%u R=%u\n", grid, W, S, R); return 1; }
        std::vector<int> seen((size_t)W * S * R, 0);
        uint32_t live = 0;
        for (uint32_t id = 0; id < grid; ++id) {
          uint32_t w, s, r;
          const bool ok = sort_block_of(id, pp, w, s, r);
          if (ok != (w < (uint32_t)W)) { printf("FAIL id %u: ok=%d but w=%u (W=%d)\n", id, (int)ok, w, W); return 1; }
          if (w % 8u != id % 8u || s >= S || r >= R) { printf("FAIL id %u -> (%u, %u, %u) for W=%d S=%u R=%u\n", id, w, s, r, W, S, R); return 1; }
          if (!ok) continue;
          ++live;
          if (seen[((size_t)w * S + s) * R + r]++) { printf("FAIL (%u, %u, %u) twice, W=%d S=%u R=%u\n", w, s, r, W, S, R); return 1; }
        }
        if (live != (uint32_t)W * S * R) { printf("FAIL %u live ids for W=%d S=%u R=%u\n", live, W, S, R); return 1; }
        ++maps;
      }
  for (uint32_t n : {1u, 7u, 8u, 63u, 64u, 65u, 1000u, 16385u, 40000u, (1u << 17) + 3u, (1u << 20), (1u << 20) + 1u})
    for (uint32_t S : {1u, 2u, 3u, 8u, 16u}) {
      PlanParams pp{};
      pp.n = n; pp.S = S; pp.slice = sort_slice_terms(n, S); pp.stride = (n + 63u) & ~63u;
      if (pp.slice % 64u != 0 || (uint64_t)pp.slice * S < n) { printf("FAIL slice %u for n=%u S=%u\n", pp.slice, n, S); return 1; }
      uint32_t next = 0;
      for (uint32_t s = 0; s < S; ++s) {
        uint32_t lo, hi;
        sort_slice_groups(pp, s, lo, hi);
        if (lo != next || hi < lo || hi > pp.stride / 8u) { printf("FAIL n=%u S=%u slice %u: [%u, %u) after %u\n", n, S, s, lo, hi, next); return 1; }
        next = hi;
      }
      if (next != pp.stride / 8u) { printf("FAIL n=%u S=%u: slices end at group %u of %u\n", n, S, next, pp.stride / 8u); return 1; }
      ++rows;
    }
  for (int c = 8; c <= 20; ++c) {
    const int32_t B = 1 << (c - 1);
    PlanParams pp{};
    pp.c = c; pp.W = 254 / c + 1; pp.stride = 64;
    const bool narrow = c <= kNarrowDigitBits;
    if (digit_mag_bytes(pp) != (size_t)64 * pp.W * (narrow ? 2 : 4) || digit_plane_words(pp) != (size_t)pp.W * 2) { printf("FAIL sizes at c=%d\n", c); return 1; }
    for (int32_t d = -B + 1; d <= B; ++d) {
      const DigitCode e = digit_encode(d);
      const uint32_t stored = narrow ? (uint32_t)(uint16_t)e.mag : e.mag;
      if (e.skip != (d == 0) || e.neg != (d < 0) || (!e.skip && e.mag >= (uint32_t)B) || stored != e.mag || digit_decode(stored, e.neg, e.skip) != d) {
        printf("FAIL c=%d d=%d -> mag %u neg %d skip %d\n", c, d, e.mag, (int)e.neg, (int)e.skip);
        return 1;
      }
      ++digits;
    }
  }
  printf("OK %ld maps, %ld rows, %ld digits\n", maps, rows, digits);
  return 0;
}
