/* gosnarkhip.R1csCheck (go/gosnarkhip/r1cs.go), as C: a process without Python uploads a sparse R1CS and a witness, asks
 * gs_r1cs_check which constraints the witness breaks -- the first `cap` rows with their values, then the count alone -- and prints
 * what it was told.
 * argv: an instance file of tests/c_util.py's write_r1cs whose trailing scalars are the witness (m of them), and cap. */
#include <inttypes.h>

#include "instance.h"

int main(int argc, char** argv) {
  if (argc != 3) return 9;
  r1cs_instance g;
  if (read_r1cs_instance(argv[1], &g) || g.ntoxic != g.m) { printf("FAIL: cannot read the input\n"); return 8; }
  const size_t cap = (size_t)strtoull(argv[2], NULL, 10);

  int dev = 0;
  gs_handle sys, w;
  CHECK(gs_init(&dev, 1));
  CHECK(gs_r1cs_upload(g.n, g.m, g.rowptr[0], g.col[0], g.val[0], g.rowptr[1], g.col[1], g.val[1], g.rowptr[2], g.col[2], g.val[2], &sys));
  CHECK(gs_scalars_upload(g.toxic, g.m, &w));

  uint32_t* rows = (uint32_t*)malloc((cap + 1) * sizeof(uint32_t));
  uint64_t* values = (uint64_t*)malloc((cap + 1) * 12 * sizeof(uint64_t));
  if (!rows || !values) return 7;
  memset(rows, 0xEE, (cap + 1) * sizeof(uint32_t));
  uint64_t count = 0, again = 0;
  CHECK(gs_r1cs_check(sys, w, cap, &count, rows, values));
  printf("violated %" PRIu64 "\n", count);
  const size_t k = count < cap ? (size_t)count : cap;
  for (size_t i = 0; i < k; ++i) {
    printf("row %" PRIu32, rows[i]);
    for (size_t t = 0; t < 12; ++t) printf(" %016" PRIx64, values[i * 12 + t]);
    printf("\n");
  }
  for (size_t i = k; i <= cap; ++i)
    if (rows[i] != 0xEEEEEEEEu) { printf("FAIL: slot %zu beyond the reported rows was written\n", i); return 2; }
  CHECK(gs_r1cs_check(sys, w, 0, &again, NULL, NULL));
  if (again != count) { printf("FAIL: the count-only call says %" PRIu64 "\n", again); return 3; }
  uint64_t untouched = 77;
  if (gs_r1cs_check(sys, w, 1, &untouched, NULL, NULL) != GS_ERR_ARG || untouched != 77) { printf("FAIL: cap without rows was accepted\n"); return 4; }
  printf("%s\n", count ? "REFUSE" : "PROVE");
  CHECK(gs_free(w));
  CHECK(gs_free(sys));
  gs_shutdown();
  free(rows);
  free(values);
  return 0;
}
