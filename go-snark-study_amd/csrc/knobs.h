// Environment switches of the library, in ONE place (round 3 shipped ~15 raw getenv/atoi calls, one of
// which -- GS_REDUCE_L=3 -- silently produced a wrong MSM).
//
//  * run_flag / run_knob: available in every build.  They select between code paths that give the SAME results (stream layout,
//    tracing, copy threads); numeric ones are parsed strictly and a value outside their range is ignored (the default stands).
//  * dev_knob / dev_knob_f / dev_flag: tuning of the algorithms themselves (window model, chunk sizes, reduce shape, ...).
//    Compiled OUT of the product library: they read the environment only in a development build (`make EXTRA=-DGS_DEV_KNOBS ...`,
//    how tools/gpu_run.sh's A/B variants are made), and even there a value the algorithm cannot take -- out of range, not a
//    multiple of `multiple_of`, not a power of two where one is needed -- falls back to the default instead of being used.
#pragma once
#include <cerrno>
#include <cstdint>
#include <cstdlib>

namespace gs {

inline bool knob_parse(const char* name, long lo, long hi, long multiple_of, bool pow2, long& out) {
  const char* s = getenv(name);
  if (!s || !*s) return false;
  char* end = nullptr;
  errno = 0;
  const long v = strtol(s, &end, 10);
  if (errno != 0 || end == s || *end != '\0') return false;
  if (v < lo || v > hi) return false;
  if (multiple_of > 1 && v % multiple_of != 0) return false;
  if (pow2 && (v <= 0 || (v & (v - 1)) != 0)) return false;
  out = v;
  return true;
}

inline bool run_flag(const char* name) { return getenv(name) != nullptr; }
inline long run_knob(const char* name, long dflt, long lo, long hi) {
  long v = dflt;
  return knob_parse(name, lo, hi, 1, false, v) ? v : dflt;
}

// GS_ACC_GROUP_G1 / GS_ACC_GROUP_G2: threads per workgroup of k_bucket_accumulate<G1> / <G2>, 64, 128 or 256 (scheduling only: the
// same additions in the same order whatever the size).  A set switch goes before acc_shape.h's policy for that curve in EVERY launch;
// any other value is ignored.  The instrument of profiles/acc_group_ab.txt and tests/test_gpu_acc_group.py.
inline long acc_group_env(const char* name) {           // the switch's value, or 0 = unset
  const long v = run_knob(name, 0, 64, 256);
  return (v == 64 || v == 128 || v == 256) ? v : 0;
}
inline long acc_group_forced(bool g2) {                 // read once per process
  static const long g1_v = acc_group_env("GS_ACC_GROUP_G1"), g2_v = acc_group_env("GS_ACC_GROUP_G2");
  return g2 ? g2_v : g1_v;
}

// The schedule of gs_r1cs_solve (solve_plan.h), when gs_solve_opts leaves a field 0.  Levels narrower than kSolveNarrow rows merge into
// sequential runs (k_solve_run: one thread per witness walks them in order), cut every kSolveRunMaxRows rows.
// Measured on one MI355X (profiles/r1cs_solve_timing.txt, tools/time_r1cs_solve.py), one witness: one dependent row in k_solve_run
// takes 6.78 us on sqchain 2^16 and 6.51 us on sqchain 2^12 (a chain of dependent loads -- plan entry, row pointers, entries, the
// element the row before stored -- and some ten field multiplications, in ONE wave with nothing to hide them behind); the same 2^12
// chain with every row a launch of its own takes 8.33 us per launch, so a launch boundary costs 1.82 us (the ABI cannot enqueue an
// empty level; the difference on one chain stands for the gap between two launches).  The ratio gap / row is 0.28: rounded to a power
// of two it is below one row, i.e. a launch of its own is cheaper than a run for every level of two rows or more (8.3 us against
// 13 us and up), and only a level of ONE row is cheaper inside a run (6.5 us against 8.3 us).  Hence kSolveNarrow = 2: the smallest
// value that still merges anything.  kSolveRunMaxRows keeps one launch under 50 ms: 50 ms / 6.78 us = 7379 rows, as a power of two
// 4096 (28 ms).
constexpr uint32_t kSolveNarrow = 2;
constexpr uint32_t kSolveRunMaxRows = 1u << 12;

#ifdef GS_DEV_KNOBS
inline bool dev_flag(const char* name) { return getenv(name) != nullptr; }
inline long dev_knob(const char* name, long dflt, long lo, long hi, long multiple_of = 1, bool pow2 = false) {
  long v = dflt;
  return knob_parse(name, lo, hi, multiple_of, pow2, v) ? v : dflt;
}
inline double dev_knob_f(const char* name, double dflt, double lo, double hi) {
  const char* s = getenv(name);
  if (!s || !*s) return dflt;
  char* end = nullptr;
  const double v = strtod(s, &end);
  return (end == s || *end != '\0' || !(v >= lo && v <= hi)) ? dflt : v;
}
#else
inline bool dev_flag(const char*) { return false; }
inline long dev_knob(const char*, long dflt, long, long, long = 1, bool = false) { return dflt; }
inline double dev_knob_f(const char*, double dflt, double, double) { return dflt; }
#endif

}  // namespace gs
