// Device side of gs_r1cs_solve (r1cs_solve.hip): the resident plan of solve_plan.h as the kernels read it, and the launches.
#pragma once
#include "runtime.h"

namespace gs {

struct SolveDev {                         // kernel argument
  const uint32_t* rowptr[3];              // the system: A, B, C in CSR, values in standard form
  const uint32_t* col[3];
  const uint32_t* val[3];
  const uint32_t* rows;                   // the plan in solve order: row, target, form (solve_plan.h, SolveForm), and per entry 8 words
  const uint32_t* targets;                //   in Montgomery form: 1 / c_x, a_x or b_x
  const uint32_t* forms;
  const uint32_t* elems;
  uint32_t m;
};

// All enqueue only, on c.stream.  wtab: nwit device pointers to vectors of m elements; fail: per witness [failure count | first plan
// position, 0xffffffff = none].
// solve_begin_dev: every vector becomes 0 except variable 0 = 1 and the inputs (inputs_std: nwit x ninputs elements, any 256-bit
// value), all in Montgomery form -- the working form of the vectors until solve_finish_dev makes them canonical standard form.
void solve_begin_dev(Ctx& c, uint32_t* const* wtab, size_t nwit, size_t m, const uint32_t* inputs_std, const uint32_t* input_vars, size_t ninputs,
                     uint32_t* fail);
void solve_level_dev(Ctx& c, const SolveDev& plan, uint32_t lo, uint32_t hi, uint32_t* const* wtab, size_t nwit, uint32_t* fail);
void solve_run_dev(Ctx& c, const SolveDev& plan, uint32_t lo, uint32_t hi, uint32_t* const* wtab, size_t nwit, uint32_t* fail);
void solve_finish_dev(Ctx& c, uint32_t* const* wtab, size_t nwit, size_t m);

}  // namespace gs
