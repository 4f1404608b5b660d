// Host driver of csrc/solve_plan.h (no GPU): reads one system from stdin, prints its level plan and launch schedule;
// tests/test_solve_plan_host.py compares them with the plan restated in Python (tests/solve_util.py).
// Input:  n m ninputs narrow run_max_rows / the inputs / then for A, B, C every row as: count (col hexvalue)*
// Output: STATUS s bad / ENTRIES k + k lines "row target form element" (element in standard form, hex) / LEVELS .. / UNSOLVED .. /
//         COUNTS checks stuck / LAUNCHES k + k lines "lo hi run"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../go-snark-study_amd/csrc/solve_plan.h"

using namespace gs;

static void parse_hex(const char* s, uint64_t out[4]) {
  out[0] = out[1] = out[2] = out[3] = 0;
  const size_t len = strlen(s);
  for (size_t i = 0; i < len && i < 64; ++i) {
    const char ch = s[len - 1 - i];
    const uint64_t d = ch >= 'a' ? ch - 'a' + 10 : ch >= 'A' ? ch - 'A' + 10 : ch - '0';
    out[i / 16] |= d << (4 * (i % 16));
  }
}

int main() {
  size_t n, m, ninputs;
  unsigned narrow, run_max;
  if (scanf("%zu %zu %zu %u %u", &n, &m, &ninputs, &narrow, &run_max) != 5) return 2;
  std::vector<uint32_t> inputs(ninputs);
  for (auto& v : inputs) if (scanf("%u", &v) != 1) return 2;
  std::vector<uint32_t> rp[3], cl[3];
  std::vector<uint64_t> vl[3];
  SolveCsr mat[3];
  char buf[128];
  for (int k = 0; k < 3; ++k) {
    rp[k].push_back(0);
    for (size_t r = 0; r < n; ++r) {
      unsigned cnt;
      if (scanf("%u", &cnt) != 1) return 2;
      for (unsigned e = 0; e < cnt; ++e) {
        unsigned c;
        if (scanf("%u %100s", &c, buf) != 2) return 2;
        uint64_t w[4];
        parse_hex(buf, w);
        cl[k].push_back(c);
        vl[k].insert(vl[k].end(), w, w + 4);
      }
      rp[k].push_back((uint32_t)cl[k].size());
    }
    cl[k].push_back(0); vl[k].resize(vl[k].size() + 4);      // never empty
    mat[k] = SolveCsr{rp[k].data(), cl[k].data(), vl[k].data()};
  }
  SolvePlan plan;
  size_t bad = 0;
  const SolvePlanStatus st = plan_solve_levels(mat, n, m, inputs.data(), ninputs, plan, &bad);
  printf("STATUS %d %zu\n", (int)st, bad);
  if (st != kSpOk) return 0;
  printf("ENTRIES %zu\n", plan.entries.size());
  for (const SolveEntry& e : plan.entries) {
    uint32_t w[8];
    pack32<ModR>(from_mont(unpack32<ModR>(e.elem)), w);
    printf("%u %u %u ", e.row, e.target, e.form);
    for (int i = 7; i >= 0; --i) printf("%08x", w[i]);
    printf("\n");
  }
  printf("LEVELS");
  for (uint32_t v : plan.level_off) printf(" %u", v);
  printf("\nUNSOLVED");
  for (uint32_t v : plan.unsolved) printf(" %u", v);
  printf("\nCOUNTS %llu %llu\n", (unsigned long long)plan.checks, (unsigned long long)plan.stuck);
  SolveOptions opts;
  opts.narrow = narrow; opts.run_max_rows = run_max;
  std::vector<SolveLaunch> ls;
  plan_solve_launches(plan.level_off, opts, ls);
  printf("LAUNCHES %zu\n", ls.size());
  for (const SolveLaunch& l : ls) printf("%u %u %d\n", l.lo, l.hi, (int)l.run);
  printf("DEFAULTS %u %u\n", kSolveNarrow, kSolveRunMaxRows);
  return 0;
}
