// The level plan and the launch schedule of gs_r1cs_solve (r1cs_solve.hip): a witness solved FROM the system.
//
// For the systems the reference's compiler emits (circuitcompiler/circuit.go: GenerateR1CS writes one flattened gate per row) `out`
// sits alone in C, or alone in A / B for a division, so every row defines one new signal from earlier ones: a sparse triangular solve.
//
// The plan is level-synchronous and deterministic (tests/solve_util.py restates it the slow way):
//   known_0 = {0} + inputs (variable 0 is the constant one);
//   level l >= 1 takes every row not yet used whose set of DISTINCT variables -- every column that occurs in the row of A, B or C,
//     whatever its coefficient -- has exactly one member x outside known_(l-1), provided the coefficient of x, summed mod r over the
//     duplicate columns of each matrix row, is nonzero in exactly ONE of A, B, C;
//   such a row defines x.  With w[x] = 0 the three dot products SA, SB, SC run over the whole row:
//     form C:  x = (SA SB - SC) / c_x        form A:  x = (SC - SA SB) / (a_x SB)        form B:  x = (SC - SA SB) / (b_x SA)
//   if several rows of one level define the same x the lowest row wins, the others become checks;
//   known_l = known_(l-1) + the targets of level l; planning stops at the first empty level.
// A row whose unknown sits in two matrices (v v = k) or that has two unknowns never defines anything: its variables stay unsolved
// unless another row defines them.  Rows that define nothing and whose variables all became known are CHECKS (the solve does not
// examine them, gs_r1cs_check does); rows with a variable that stays unsolved are STUCK.
// Inside a level the entries are ordered by (form, row), which keeps the lanes that invert together.
// Counters per row and a variable -> rows adjacency, never a rescan per level: O(nnz) for the levels (a row is looked at once, when
// its count reaches one), after one sort of every row's columns to find its distinct
// variables, O(nnz log(row length)), and with one sort of each level's candidate rows, O(n log n) over all levels.
//
// The schedule: consecutive levels narrower than `narrow` rows merge into a RUN, executed by one launch in plan order (which respects
// the levels) and cut every `run_max_rows` rows, so that no launch is unbounded; every other level is one WIDE launch.
//
// Pure host code, no HIP calls: capi_r1cs.hip and tests/host/solve_plan_host_test.hip include it (fp29.h compiles for the host).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "fp29.h"
#include "knobs.h"

namespace gs {

enum SolveForm : uint32_t { kSolveFormC = 0, kSolveFormA = 1, kSolveFormB = 2 };

struct SolveCsr {                     // one matrix: n + 1 | nnz | nnz x 4 words (standard form, any 256-bit value)
  const uint32_t* rowptr;
  const uint32_t* col;
  const uint64_t* val;
};
struct SolveOptions { uint32_t narrow = 0, run_max_rows = 0; };     // 0 = knobs.h's default
struct SolveEntry {
  uint32_t row, target, form;
  uint32_t elem[8];                   // Montgomery form, canonical: 1 / c_x (form C), a_x (form A), b_x (form B)
};
struct SolveLaunch { uint32_t lo, hi; bool run; };                  // plan positions [lo, hi)
struct SolvePlan {
  std::vector<SolveEntry> entries;    // solve order
  std::vector<uint32_t> level_off;    // levels + 1 offsets into entries
  std::vector<uint32_t> unsolved;     // ascending
  uint64_t checks = 0, stuck = 0;
};

enum SolvePlanStatus { kSpOk = 0, kSpInputRange = 1, kSpInputZero = 2, kSpInputTwice = 3 };

using SpFr = Fe<ModR, 2>;
inline SpFr sp_load_mont(const uint64_t* w) {
  uint32_t u[8];
  for (int i = 0; i < 4; ++i) { u[2 * i] = (uint32_t)w[i]; u[2 * i + 1] = (uint32_t)(w[i] >> 32); }
  return to_mont(unpack32<ModR>(u));
}
inline void sp_store(const SpFr& a, uint32_t (&out)[8]) { pack32<ModR>(canon(a), out); }
// the coefficient of column x in one matrix row, duplicates summed (Montgomery)
inline SpFr sp_coeff(const SolveCsr& M, uint32_t row, uint32_t x) {
  SpFr acc = fe_zero<ModR, 2>();
  for (uint32_t e = M.rowptr[row]; e < M.rowptr[row + 1]; ++e)
    if (M.col[e] == x) acc = reduce2(add(acc, sp_load_mont(M.val + (size_t)e * 4)));
  return acc;
}

// On an error *bad_input is the index of the first offending entry of `inputs` and the plan's contents are unspecified.
inline SolvePlanStatus plan_solve_levels(const SolveCsr mat[3], size_t n, size_t m, const uint32_t* inputs, size_t ninputs, SolvePlan& plan,
                                         size_t* bad_input = nullptr) {
  plan = SolvePlan{};
  std::vector<uint8_t> known(m, 0);
  if (m) known[0] = 1;
  for (size_t i = 0; i < ninputs; ++i) {
    const uint32_t v = inputs[i];
    const SolvePlanStatus st = v >= m ? kSpInputRange : v == 0 ? kSpInputZero : known[v] ? kSpInputTwice : kSpOk;
    if (st != kSpOk) {
      if (bad_input) *bad_input = i;
      return st;
    }
    known[v] = 1;
  }
  // the distinct variables of every row
  std::vector<size_t> rv_ptr(n + 1, 0);
  std::vector<uint32_t> rv;
  rv.reserve((size_t)mat[0].rowptr[n] + mat[1].rowptr[n] + mat[2].rowptr[n]);
  for (size_t r = 0; r < n; ++r) {
    const size_t start = rv.size();
    for (int k = 0; k < 3; ++k) rv.insert(rv.end(), mat[k].col + mat[k].rowptr[r], mat[k].col + mat[k].rowptr[r + 1]);
    std::sort(rv.begin() + start, rv.end());
    rv.erase(std::unique(rv.begin() + start, rv.end()), rv.end());
    rv_ptr[r + 1] = rv.size();
  }
  // variable -> rows (ascending), and the number of unknown variables per row
  std::vector<size_t> adj_ptr(m + 1, 0);
  for (uint32_t v : rv) adj_ptr[v + 1] += 1;
  for (size_t v = 0; v < m; ++v) adj_ptr[v + 1] += adj_ptr[v];
  std::vector<uint32_t> adj(rv.size());
  {
    std::vector<size_t> fill(adj_ptr.begin(), adj_ptr.end() - 1);
    for (size_t r = 0; r < n; ++r)
      for (size_t e = rv_ptr[r]; e < rv_ptr[r + 1]; ++e) adj[fill[rv[e]]++] = (uint32_t)r;
  }
  std::vector<uint32_t> unk(n, 0);
  std::vector<uint8_t> used(n, 0);
  std::vector<uint32_t> cand, next;
  for (size_t r = 0; r < n; ++r) {
    for (size_t e = rv_ptr[r]; e < rv_ptr[r + 1]; ++e) unk[r] += !known[rv[e]];
    if (unk[r] == 1) cand.push_back((uint32_t)r);
  }
  // A row is a candidate once, at the level at which its count reaches one: the loser of a tie has none left at the next level, and
  // a row whose unknown sits in two matrices (or in none: coefficients that cancel) is the same row at every later level.
  std::vector<uint32_t> claimed(m, 0);             // the level that claimed the variable, 0 = none
  std::vector<SpFr> cinv;                          // form C: c_x per entry, inverted together at the end
  std::vector<size_t> cinv_at;
  plan.level_off.push_back(0);
  for (uint32_t level = 1; !cand.empty(); ++level) {
    std::sort(cand.begin(), cand.end());
    const size_t first = plan.entries.size();
    struct Pending { SolveEntry e; SpFr k; };
    std::vector<Pending> lvl;
    for (uint32_t r : cand) {
      if (unk[r] != 1) continue;                   // two of its variables were solved by the level before: nothing left to define
      uint32_t x = 0;
      for (size_t e = rv_ptr[r]; e < rv_ptr[r + 1]; ++e) if (!known[rv[e]]) x = rv[e];
      SpFr k[3];
      int nonzero = 0, which = 0;
      for (int j = 0; j < 3; ++j) {
        k[j] = sp_coeff(mat[j], r, x);
        if (!is_zero(k[j])) { nonzero += 1; which = j; }
      }
      if (nonzero != 1 || claimed[x] == level) continue;
      claimed[x] = level;
      Pending p;
      p.e.row = r; p.e.target = x;
      p.e.form = which == 2 ? kSolveFormC : which == 0 ? kSolveFormA : kSolveFormB;
      p.k = k[which];
      lvl.push_back(p);
    }
    if (lvl.empty()) break;
    std::stable_sort(lvl.begin(), lvl.end(), [](const Pending& a, const Pending& b) { return a.e.form < b.e.form; });   // rows ascend already
    next.clear();
    for (const Pending& p : lvl) {
      if (p.e.form == kSolveFormC) { cinv.push_back(p.k); cinv_at.push_back(plan.entries.size()); }
      plan.entries.push_back(p.e);
      sp_store(p.k, plan.entries.back().elem);
      used[p.e.row] = 1;
    }
    for (size_t i = first; i < plan.entries.size(); ++i) {
      const uint32_t x = plan.entries[i].target;
      known[x] = 1;
      for (size_t e = adj_ptr[x]; e < adj_ptr[x + 1]; ++e) {
        const uint32_t r = adj[e];
        if (--unk[r] == 1 && !used[r]) next.push_back(r);
      }
    }
    plan.level_off.push_back((uint32_t)plan.entries.size());
    cand.swap(next);
  }
  // 1 / c_x for every form-C entry: one inversion (prefix products), three multiplications per entry
  if (!cinv.empty()) {
    std::vector<SpFr> pre(cinv.size());
    SpFr acc = relax<2>(fe_one<ModR>());
    for (size_t i = 0; i < cinv.size(); ++i) { pre[i] = acc; acc = mul(acc, cinv[i]); }
    SpFr back = inv(acc);
    for (size_t i = cinv.size(); i-- > 0;) {
      sp_store(mul(back, pre[i]), plan.entries[cinv_at[i]].elem);
      back = mul(back, cinv[i]);
    }
  }
  for (size_t v = 0; v < m; ++v) if (!known[v]) plan.unsolved.push_back((uint32_t)v);
  for (size_t r = 0; r < n; ++r) if (!used[r]) (unk[r] ? plan.stuck : plan.checks) += 1;
  return kSpOk;
}

// level offsets -> launches
inline void plan_solve_launches(const std::vector<uint32_t>& level_off, const SolveOptions& opts, std::vector<SolveLaunch>& out) {
  const uint32_t narrow = opts.narrow ? opts.narrow : kSolveNarrow;
  const uint32_t run_max = opts.run_max_rows ? opts.run_max_rows : kSolveRunMaxRows;
  out.clear();
  auto flush_run = [&](uint32_t lo, uint32_t hi) {
    for (; lo < hi; lo += std::min(run_max, hi - lo)) out.push_back(SolveLaunch{lo, lo + std::min(run_max, hi - lo), true});
  };
  uint32_t run_lo = 0, run_hi = 0;                   // the open run, empty when run_lo == run_hi
  for (size_t l = 0; l + 1 < level_off.size(); ++l) {
    const uint32_t lo = level_off[l], hi = level_off[l + 1];
    if (hi - lo < narrow) {
      if (run_lo == run_hi) run_lo = lo;
      run_hi = hi;
      continue;
    }
    flush_run(run_lo, run_hi);
    run_lo = run_hi = 0;
    out.push_back(SolveLaunch{lo, hi, false});
  }
  flush_run(run_lo, run_hi);
}

}  // namespace gs
