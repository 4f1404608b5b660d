/* gosnarkhip.G1Compress / G1Decompress / G2Compress / G2Decompress (go/gosnarkhip/point_codec.go), as C: a process without Python
 * uploads an array of G1 and an array of G2 points, compresses them, decompresses the result and compares the downloads; then it sets
 * one x to 0 -- a value whose right-hand side has no square root on either curve -- and asks for the count and the index of the bad
 * entry and whether every other point came through.
 * argv: a file of little-endian u64 words: n, then n G1 Jacobian triples of 12 words, then n G2 triples of 24 words (tests/c_util.py);
 *       the index to plant the bad x at. */
#include <inttypes.h>

#include "instance.h"

static void show(const char* what, uint64_t nbad, uint64_t first, int rest_equal) {
  if (first == UINT64_MAX) printf("%s: %" PRIu64 " bad, first none, the rest %s\n", what, nbad, rest_equal ? "equal" : "DIFFERENT");
  else printf("%s: %" PRIu64 " bad, first %" PRIu64 ", the rest %s\n", what, nbad, first, rest_equal ? "equal" : "DIFFERENT");
}

/* one group: words = 4 (G1) or 8 (G2) per x, 3 * words per Jacobian triple */
static int run(int g2, const uint64_t* jac, size_t n, size_t at) {
  const size_t cw = g2 ? 8 : 4, jw = 3 * cw;
  gs_handle pts, back;
  uint64_t nbad = 0, first = 0;
  uint64_t* x = (uint64_t*)calloc(n * cw, 8);
  uint64_t* a = (uint64_t*)calloc(n * jw, 8);
  uint64_t* b = (uint64_t*)calloc(n * jw, 8);
  uint8_t* flags = (uint8_t*)calloc(n, 1);
  uint8_t* ok = (uint8_t*)calloc(n, 1);
  if (!x || !a || !b || !flags || !ok) return 7;
  CHECK(g2 ? gs_g2_upload(jac, n, &pts) : gs_g1_upload(jac, n, &pts));
  CHECK(g2 ? gs_g2_compress(pts, 0, n, x, flags) : gs_g1_compress(pts, 0, n, x, flags));
  CHECK(g2 ? gs_g2_download(pts, a, n) : gs_g1_download(pts, a, n));

  CHECK(g2 ? gs_g2_decompress(x, flags, n, &back, ok, &nbad, &first) : gs_g1_decompress(x, flags, n, &back, ok, &nbad, &first));
  CHECK(g2 ? gs_g2_download(back, b, n) : gs_g1_download(back, b, n));
  int all_ok = 1;
  for (size_t i = 0; i < n; ++i) all_ok &= ok[i] == 1;
  show(g2 ? "g2 round trip" : "g1 round trip", nbad, first, all_ok && memcmp(a, b, n * jw * 8) == 0);
  CHECK(gs_free(back));

  memset(x + at * cw, 0, cw * 8);
  flags[at] = 0;
  CHECK(g2 ? gs_g2_decompress(x, flags, n, &back, ok, &nbad, &first) : gs_g1_decompress(x, flags, n, &back, ok, &nbad, &first));
  CHECK(g2 ? gs_g2_download(back, b, n) : gs_g1_download(back, b, n));
  int rest = 1, planted_is_infinity = ok[at] == 0;
  for (size_t i = 0; i < n; ++i) {
    if (i == at) {
      for (size_t k = 0; k < jw; ++k) planted_is_infinity &= b[i * jw + k] == 0;
    } else {
      rest &= ok[i] == 1 && memcmp(a + i * jw, b + i * jw, jw * 8) == 0;
    }
  }
  show(g2 ? "g2 planted" : "g1 planted", nbad, first, rest && planted_is_infinity);
  if ((g2 ? gs_g2_compress(pts, 1, n, x, flags) : gs_g1_compress(pts, 1, n, x, flags)) != GS_ERR_SHAPE) {
    printf("FAIL: a window past the end was accepted\n");
    return 2;
  }
  CHECK(gs_free(back));
  CHECK(gs_free(pts));
  free(x); free(a); free(b); free(flags); free(ok);
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 3) return 9;
  size_t words = 0;
  uint64_t* p = gs_read_file(argv[1], &words);
  if (!p || words < 1 || words != 1 + p[0] * 36) { printf("FAIL: cannot read the input\n"); return 8; }
  const size_t n = (size_t)p[0], at = (size_t)strtoull(argv[2], NULL, 10);
  if (at >= n) return 9;

  int dev = 0;
  CHECK(gs_init(&dev, 1));
  int rc = run(0, p + 1, n, at);
  if (rc) return rc;
  rc = run(1, p + 1 + n * 12, n, at);
  if (rc) return rc;
  gs_shutdown();
  return 0;
}
