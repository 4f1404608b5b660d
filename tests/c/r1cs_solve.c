/* gosnarkhip.R1csSolvePlan / R1csSolveUnsolved / R1csSolve (go/gosnarkhip/r1cs_solve.go), as C: a process without Python uploads a
 * sparse R1CS, plans its solve for the given input variables, solves nwit witnesses from their input values in one call -- the first
 * into a vector it created itself --, and prints the plan's counts and every witness.
 * argv: an instance file of tests/c_util.py's write_r1cs whose trailing scalars are the input values (nwit x ninputs), then the
 * input variables. */
#include <inttypes.h>

#include "instance.h"

int main(int argc, char** argv) {
  if (argc < 3) return 9;
  r1cs_instance g;
  if (read_r1cs_instance(argv[1], &g)) { printf("FAIL: cannot read the input\n"); return 8; }
  const size_t ninputs = (size_t)argc - 2;
  if (g.ntoxic == 0 || g.ntoxic % ninputs) { printf("FAIL: %zu values for %zu inputs\n", g.ntoxic, ninputs); return 8; }
  const size_t nwit = g.ntoxic / ninputs;
  uint32_t* vars = (uint32_t*)malloc(ninputs * sizeof(uint32_t));
  for (size_t k = 0; k < ninputs; ++k) vars[k] = (uint32_t)strtoul(argv[2 + k], NULL, 10);

  size_t ob = 0, sb = 0;
  CHECK(gs_solve_abi_sizes(&ob, &sb));
  if (ob != sizeof(gs_solve_opts) || sb != sizeof(gs_solve_stats)) { printf("FAIL: struct sizes %zu %zu\n", ob, sb); return 2; }

  int dev = 0;
  gs_handle sys, plan = 77;
  gs_solve_stats st;
  CHECK(gs_init(&dev, 1));
  CHECK(gs_r1cs_upload(g.n, g.m, g.rowptr[0], g.col[0], g.val[0], g.rowptr[1], g.col[1], g.val[1], g.rowptr[2], g.col[2], g.val[2], &sys));
  uint32_t zero = 0;
  if (gs_r1cs_solve_plan(sys, &zero, 1, NULL, &plan, NULL) != GS_ERR_ARG || plan != 77) { printf("FAIL: input 0 was accepted\n"); return 3; }
  CHECK(gs_r1cs_solve_plan(sys, vars, ninputs, NULL, &plan, &st));
  CHECK(gs_free(sys));                                   /* the plan keeps its system alive */
  printf("plan solved %" PRIu64 " unsolved %" PRIu64 " checks %" PRIu64 " stuck %" PRIu64 " levels %" PRIu64 "\n", st.solved, st.unsolved, st.checks,
         st.stuck, st.levels);
  uint64_t count = 0;
  uint32_t* unsolved = (uint32_t*)malloc((g.m + 1) * sizeof(uint32_t));
  CHECK(gs_r1cs_solve_unsolved(plan, g.m, unsolved, &count));
  printf("unsolved");
  for (uint64_t i = 0; i < count; ++i) printf(" %" PRIu32, unsolved[i]);
  printf("\n");

  gs_handle* w = (gs_handle*)calloc(nwit, sizeof(gs_handle));
  uint64_t* nfailed = (uint64_t*)malloc(nwit * sizeof(uint64_t));
  uint32_t* first = (uint32_t*)malloc(nwit * sizeof(uint32_t));
  uint64_t* out = (uint64_t*)malloc(g.m * 4 * sizeof(uint64_t));
  if (!w || !nfailed || !first || !out) return 7;
  memset(out, 0xEE, g.m * 4 * sizeof(uint64_t));
  CHECK(gs_scalars_upload(out, g.m, &w[0]));              /* witness 0 overwrites a vector of the caller */
  const gs_handle mine = w[0];
  CHECK(gs_r1cs_solve(plan, nwit, g.toxic, w, nfailed, first));
  if (w[0] != mine) { printf("FAIL: the caller's vector was replaced\n"); return 4; }
  for (size_t b = 0; b < nwit; ++b) {
    CHECK(gs_scalars_download(w[b], out, g.m));
    printf("witness %zu failed %" PRIu64 " first %" PRIu32, b, nfailed[b], first[b]);
    for (size_t t = 0; t < g.m * 4; ++t) printf(" %016" PRIx64, out[t]);
    printf("\n");
    CHECK(gs_free(w[b]));
  }
  CHECK(gs_free(plan));
  gs_shutdown();
  printf("DONE\n");
  return 0;
}
