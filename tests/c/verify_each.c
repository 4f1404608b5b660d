/* gosnarkhip.Groth16VerifyEach (go/gosnarkhip/pairing_device.go), as C: a process without Python reads a verification key and a batch
 * of proofs, asks gs_groth16_verify_each for a verdict per proof, asks the host's gs_groth16_verify about every proof, and prints both
 * as strings of 0s and 1s with the count of rejected proofs.
 * argv: a file of little-endian u64 words: nic, npublic, nproofs, then alpha (12), beta gamma delta (3 x 24), IC (nic x 12), the public
 * signals (nproofs x npublic x 4), A (nproofs x 12), B (nproofs x 24), C (nproofs x 12)  (tests/c_util.py). */
#include <inttypes.h>

#include "instance.h"

int main(int argc, char** argv) {
  if (argc != 2) return 9;
  size_t words = 0;
  uint64_t* p = gs_read_file(argv[1], &words);
  if (!p || words < 3) { printf("FAIL: cannot read the input\n"); return 8; }
  const size_t nic = (size_t)p[0], npublic = (size_t)p[1], n = (size_t)p[2];
  if (n == 0 || words != 3 + 12 + 72 + nic * 12 + n * npublic * 4 + n * 48) { printf("FAIL: the input has the wrong length\n"); return 8; }
  uint64_t* q = p + 3;
  const uint64_t* alpha = gs_take(&q, 12);
  const uint64_t* beta = gs_take(&q, 24);
  const uint64_t* gamma = gs_take(&q, 24);
  const uint64_t* delta = gs_take(&q, 24);
  const uint64_t* ic = gs_take(&q, nic * 12);
  const uint64_t* pub = gs_take(&q, n * npublic * 4);
  const uint64_t* a = gs_take(&q, n * 12);
  const uint64_t* b = gs_take(&q, n * 24);
  const uint64_t* c = gs_take(&q, n * 12);

  int dev = 0;
  CHECK(gs_init(&dev, 1));
  int* each = (int*)malloc(n * sizeof(int));
  if (!each) return 7;
  uint64_t nbad = 0;
  CHECK(gs_groth16_verify_each(alpha, beta, gamma, delta, ic, nic, pub, npublic, a, b, c, n, each, &nbad));
  printf("device: ");
  for (size_t i = 0; i < n; ++i) putchar(each[i] ? '1' : '0');
  printf(" (%" PRIu64 " rejected)\nhost:   ", nbad);
  for (size_t i = 0; i < n; ++i) {
    int one = 0;
    CHECK(gs_groth16_verify(alpha, beta, gamma, delta, ic, nic, pub + i * npublic * 4, npublic, a + i * 12, b + i * 24, c + i * 12, &one));
    putchar(one ? '1' : '0');
  }
  putchar('\n');
  if (gs_groth16_verify_each(alpha, beta, gamma, delta, ic, npublic, pub, npublic, a, b, c, n, each, &nbad) != GS_ERR_SHAPE) {
    printf("FAIL: too few IC points were accepted\n");
    return 2;
  }
  if (gs_groth16_verify_each(alpha, beta, gamma, delta, ic, nic, pub, npublic, a, b, c, n, NULL, &nbad) != GS_ERR_ARG) {
    printf("FAIL: a null verdict array was accepted\n");
    return 2;
  }
  free(each);
  gs_shutdown();
  return 0;
}
