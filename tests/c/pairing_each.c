/* gosnarkhip.PairingEach (go/gosnarkhip/pairing_device.go), as C: a process without Python reads n pairs of points, uploads them, asks
 * gs_pairing_each for the n pairing values and prints how many of them equal the host's gs_pairing of the same pair word for word,
 * then the "is one" flags as a string of 0s and 1s.
 * argv: a file of little-endian u64 words: n, then P (n x 12) and Q (n x 24)  (tests/c_util.py). */
#include <inttypes.h>
#include <string.h>

#include "instance.h"

int main(int argc, char** argv) {
  if (argc != 2) return 9;
  size_t words = 0;
  uint64_t* p = gs_read_file(argv[1], &words);
  if (!p || words < 1) { printf("FAIL: cannot read the input\n"); return 8; }
  const size_t n = (size_t)p[0];
  if (n == 0 || words != 1 + n * 36) { printf("FAIL: the input has the wrong length\n"); return 8; }
  uint64_t* q = p + 1;
  const uint64_t* a = gs_take(&q, n * 12);
  const uint64_t* b = gs_take(&q, n * 24);

  int dev = 0;
  CHECK(gs_init(&dev, 1));
  gs_handle ha, hb;
  CHECK(gs_g1_upload(a, n, &ha));
  CHECK(gs_g2_upload(b, n, &hb));
  uint64_t* values = (uint64_t*)malloc(n * 48 * sizeof(uint64_t));
  int* ones = (int*)malloc(n * sizeof(int));
  if (!values || !ones) return 7;
  CHECK(gs_pairing_each(ha, 0, hb, 0, n, values, ones));
  size_t equal = 0;
  for (size_t i = 0; i < n; ++i) {
    uint64_t host[48];
    CHECK(gs_pairing(a + i * 12, b + i * 24, host));
    equal += memcmp(host, values + i * 48, sizeof host) == 0 ? 1 : 0;
  }
  printf("%zu pairings, %zu equal to the host's\nis one: ", n, equal);
  for (size_t i = 0; i < n; ++i) putchar(ones[i] ? '1' : '0');
  putchar('\n');
  if (gs_pairing_each(ha, 1, hb, 0, n, values, ones) != GS_ERR_SHAPE) { printf("FAIL: a range past the end was accepted\n"); return 2; }
  if (gs_pairing_each(ha, 0, hb, 0, n, NULL, NULL) != GS_ERR_ARG) { printf("FAIL: two null out-pointers were accepted\n"); return 2; }
  CHECK(gs_free(ha));
  CHECK(gs_free(hb));
  free(values);
  free(ones);
  gs_shutdown();
  return 0;
}
