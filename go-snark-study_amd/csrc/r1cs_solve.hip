// Kernels of gs_r1cs_solve: witnesses solved from the system, level by level (solve_plan.h holds the plan and its definition).
//
// One __device__ solve_row(plan, i, w) under two kernels:
//   k_solve_level  one thread per (row i of the level, witness b).  Rows run along x, so the plan arrays are read coalesced; witnesses
//                  run along y.  The rows of one level are independent of each other.
//   k_solve_run    one thread per witness walks the plan positions [lo, hi) in order: the narrow levels, where a launch per level
//                  would cost more than its rows.  A lane only ever reads what it wrote itself (or what earlier launches wrote, in
//                  stream order), so it needs no barrier, no fence and no flag, and every lane of a wave is on the same row.  For
//                  the same reason the witness pointer is neither __restrict__ nor read through a read-only path anywhere here.
// Everything between launches is ordered by the stream.
//
// solve_row takes the three sparse dot products of k_spmv's inner loop (values in standard form times a Montgomery-form vector gives
// standard-form sums), then the form's formula, then one store of w[target] in Montgomery form: the vectors themselves are the working
// storage, zero where nothing is known yet -- which is what lets the sums run over the whole row, the target included.
// Forms A and B divide by Fermat inversion (fp29.h: 0 gives 0, no data-dependent loop).  A zero divisor stores 0, adds one to that
// witness's failure count and takes the minimum of the plan position into its first-failure word.
// A row of more than 512 entries is walked by its one thread: slow, the same sums (k_spmv hands such rows to a workgroup each; a
// hand-off between launches of a triangular solve is not built).
#include "r1cs_solve.h"

#include "fp29.h"
#include "solve_plan.h"

namespace gs {

using Fr2 = Fe<ModR, 2>;
using Fr6 = Fe<ModR, 6>;

static __device__ __forceinline__ Fr6 sv_load(const uint32_t* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 lo = q[0], hi = q[1];
  uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  return unpack32<ModR>(w);
}
static __device__ __forceinline__ void sv_store_canon(uint32_t* p, const Fe<ModR, 1>& a) {
  uint32_t w[8];
  pack32<ModR>(a, w);
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(w[0], w[1], w[2], w[3]);
  q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}

// sum_k val[k] * w[col[k]] over one matrix row: standard form, < 2r
static __device__ __forceinline__ Fr2 solve_dot(const uint32_t* __restrict__ rowptr, const uint32_t* __restrict__ col, const uint32_t* __restrict__ val,
                                                uint32_t row, const uint32_t* w, uint32_t m) {
  Fr2 acc = fe_zero<ModR, 2>();
  const uint32_t lo = rowptr[row], hi = rowptr[row + 1];
  for (uint32_t k = lo; k < hi; ++k) {
    const uint32_t cidx = col[k];
    if (cidx >= m) continue;                           // validated on the host; never trust an index on the device
    acc = reduce2(add(acc, mul(sv_load(val + (size_t)k * 8), sv_load(w + (size_t)cidx * 8))));
  }
  return acc;
}

// plan position i for one witness; fail = [count | first position] of that witness
static __device__ __forceinline__ void solve_row(const SolveDev& P, uint32_t i, uint32_t* w, uint32_t* fail) {
  const uint32_t row = P.rows[i], x = P.targets[i], form = P.forms[i];
  if (x >= P.m) return;
  const Fr2 sa = solve_dot(P.rowptr[0], P.col[0], P.val[0], row, w, P.m);
  const Fr2 sb = solve_dot(P.rowptr[1], P.col[1], P.val[1], row, w, P.m);
  const Fr2 sc = solve_dot(P.rowptr[2], P.col[2], P.val[2], row, w, P.m);
  const Fr2 ab = mul(to_mont(sa), sb);                 // SA SB, standard form
  const Fr6 e = sv_load(P.elems + (size_t)i * 8);      // Montgomery
  Fr2 out;
  if (form == kSolveFormC) {
    out = mul(to_mont(reduce2(sub(ab, sc))), e);       // (SA SB - SC) / c_x, Montgomery
  } else {
    const Fr2 den = mul(form == kSolveFormA ? sb : sa, e);            // a_x SB or b_x SA, standard form
    if (is_zero(den)) {
      out = fe_zero<ModR, 2>();
      atomicAdd(fail, 1u);
      atomicMin(fail + 1, i);
    } else {
      // inv of a standard-form v is v^-1 R^2 (it multiplies as if v were v R^-1 in Montgomery form), so the product is x R
      out = mul(reduce2(sub(sc, ab)), inv(den));
    }
  }
  sv_store_canon(w + (size_t)x * 8, canon(out));
}

__global__ void __launch_bounds__(256) k_solve_level(SolveDev P, uint32_t lo, uint32_t hi, uint32_t* const* __restrict__ wtab, uint32_t nwit,
                                                      uint32_t* fail) {
  wave_priority<GS_PRIO_POLY>();
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= hi - lo) return;
  for (uint32_t b = blockIdx.y; b < nwit; b += gridDim.y) solve_row(P, lo + t, wtab[b], fail + 2 * (size_t)b);
}

__global__ void __launch_bounds__(64) k_solve_run(SolveDev P, uint32_t lo, uint32_t hi, uint32_t* const* __restrict__ wtab, uint32_t nwit,
                                                   uint32_t* fail) {
  wave_priority<GS_PRIO_POLY>();
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= nwit) return;
  uint32_t* w = wtab[b];
  for (uint32_t i = lo; i < hi; ++i) solve_row(P, i, w, fail + 2 * (size_t)b);
}

// every element 0, variable 0 = 1 (Montgomery), the failure words reset
__global__ void __launch_bounds__(256) k_solve_clear(uint32_t* const* __restrict__ wtab, uint32_t nwit, uint32_t m, uint32_t* __restrict__ fail) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  for (uint32_t b = blockIdx.y; b < nwit; b += gridDim.y) {
    Fe<ModR, 1> v = fe_one<ModR>();
    if (j != 0) {
#pragma unroll
      for (int l = 0; l < NL; ++l) v.l[l] = 0;
    } else {
      fail[2 * (size_t)b] = 0;
      fail[2 * (size_t)b + 1] = 0xffffffffu;
    }
    sv_store_canon(wtab[b] + (size_t)j * 8, canon(v));
  }
}
// the inputs, any 256-bit value -> Montgomery
__global__ void __launch_bounds__(256) k_solve_inputs(uint32_t* const* __restrict__ wtab, uint32_t nwit, uint32_t m, const uint32_t* __restrict__ inputs,
                                                       const uint32_t* __restrict__ vars, uint32_t ninputs) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= ninputs) return;
  const uint32_t x = vars[k];
  if (x >= m) return;
  for (uint32_t b = blockIdx.y; b < nwit; b += gridDim.y)
    sv_store_canon(wtab[b] + (size_t)x * 8, canon(to_mont(sv_load(inputs + ((size_t)b * ninputs + k) * 8))));
}
// Montgomery -> canonical standard form
__global__ void __launch_bounds__(256) k_solve_finish(uint32_t* const* __restrict__ wtab, uint32_t nwit, uint32_t m) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  for (uint32_t b = blockIdx.y; b < nwit; b += gridDim.y) {
    uint32_t* p = wtab[b] + (size_t)j * 8;
    sv_store_canon(p, from_mont(sv_load(p)));
  }
}

static dim3 grid_xy(size_t nx, size_t nwit) { return dim3((unsigned)((nx + 255) / 256), (unsigned)std::min<size_t>(nwit, 65535)); }

void solve_begin_dev(Ctx& c, uint32_t* const* wtab, size_t nwit, size_t m, const uint32_t* inputs_std, const uint32_t* input_vars, size_t ninputs,
                     uint32_t* fail) {
  hipLaunchKernelGGL(k_solve_clear, grid_xy(m, nwit), dim3(256), 0, c.stream, wtab, (uint32_t)nwit, (uint32_t)m, fail);
  if (ninputs)
    hipLaunchKernelGGL(k_solve_inputs, grid_xy(ninputs, nwit), dim3(256), 0, c.stream, wtab, (uint32_t)nwit, (uint32_t)m, inputs_std, input_vars,
                       (uint32_t)ninputs);
  GS_HIP(hipGetLastError());
}
void solve_level_dev(Ctx& c, const SolveDev& plan, uint32_t lo, uint32_t hi, uint32_t* const* wtab, size_t nwit, uint32_t* fail) {
  if (hi > lo) hipLaunchKernelGGL(k_solve_level, grid_xy(hi - lo, nwit), dim3(256), 0, c.stream, plan, lo, hi, wtab, (uint32_t)nwit, fail);
  GS_HIP(hipGetLastError());
}
void solve_run_dev(Ctx& c, const SolveDev& plan, uint32_t lo, uint32_t hi, uint32_t* const* wtab, size_t nwit, uint32_t* fail) {
  if (hi > lo) hipLaunchKernelGGL(k_solve_run, dim3((unsigned)((nwit + 63) / 64)), dim3(64), 0, c.stream, plan, lo, hi, wtab, (uint32_t)nwit, fail);
  GS_HIP(hipGetLastError());
}
void solve_finish_dev(Ctx& c, uint32_t* const* wtab, size_t nwit, size_t m) {
  hipLaunchKernelGGL(k_solve_finish, grid_xy(m, nwit), dim3(256), 0, c.stream, wtab, (uint32_t)nwit, (uint32_t)m);
  GS_HIP(hipGetLastError());
}

}  // namespace gs
