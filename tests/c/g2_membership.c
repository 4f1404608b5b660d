/* gosnarkhip.G2SubgroupCheck (go/gosnarkhip/g2_membership.go), as C: a process without Python uploads an array of G2 points, asks which of
 * them lie outside the order-r subgroup -- over the whole array, over the window in front of the first such point and over the window
 * behind it -- and prints the verdicts.
 * argv: a file of little-endian u64 words: n, then n Jacobian triples of 24 words (tests/c_util.py). */
#include <inttypes.h>

#include "instance.h"

static void show(const char* what, size_t off, size_t n, uint64_t nbad, uint64_t first) {
  if (first == UINT64_MAX) printf("%s [%zu, %zu): %" PRIu64 " outside, first none\n", what, off, off + n, nbad);
  else printf("%s [%zu, %zu): %" PRIu64 " outside, first %" PRIu64 "\n", what, off, off + n, nbad, first);
}

int main(int argc, char** argv) {
  if (argc != 2) return 9;
  size_t words = 0;
  uint64_t* p = gs_read_file(argv[1], &words);
  if (!p || words < 1 || words != 1 + p[0] * 24) { printf("FAIL: cannot read the input\n"); return 8; }
  const size_t n = (size_t)p[0];

  int dev = 0;
  gs_handle pts;
  uint64_t nbad = 0, first = 0;
  CHECK(gs_init(&dev, 1));
  CHECK(gs_g2_upload(p + 1, n, &pts));
  CHECK(gs_g2_subgroup_check(pts, 0, n, &nbad, &first));
  show("all", 0, n, nbad, first);
  const int reject = nbad != 0;
  if (nbad) {
    const size_t at = (size_t)first;
    uint64_t nb = 0, fb = 0;
    CHECK(gs_g2_subgroup_check(pts, 0, at, &nb, &fb));
    show("before", 0, at, nb, fb);
    CHECK(gs_g2_subgroup_check(pts, at, 1, &nb, &fb));
    show("at", at, 1, nb, fb);
    CHECK(gs_g2_subgroup_check(pts, at + 1, n - at - 1, &nb, &fb));
    show("after", at + 1, n - at - 1, nb, fb);
  }
  if (gs_g2_subgroup_check(pts, 1, n, &nbad, &first) != GS_ERR_SHAPE) { printf("FAIL: a window past the end was accepted\n"); return 2; }
  printf("%s\n", reject ? "REJECT" : "ACCEPT");
  CHECK(gs_free(pts));
  gs_shutdown();
  return 0;
}
