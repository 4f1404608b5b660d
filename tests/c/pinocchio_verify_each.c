/* gosnarkhip.PinocchioVerifyEach (go/gosnarkhip/pairing_device.go), as C: a process without Python reads a verification key and a batch
 * of proofs, asks gs_pinocchio_verify_each for a verdict and a failing equation per proof, asks the host's gs_pinocchio_verify about
 * every proof, and prints both as strings of digits (0 = accepted, 1..5 = the first equation that does not hold) with the count of
 * rejected proofs.
 * argv: a file of little-endian u64 words: nic, npublic, nproofs, then Vka (24), Vkb (12), Vkc (24), G1Kbg (12), G2Kbg G2Kg Vkz
 * (3 x 24), IC (nic x 12), the public signals (nproofs x npublic x 4), the proofs (nproofs x 108)  (tests/c_util.py). */
#include <inttypes.h>

#include "instance.h"

int main(int argc, char** argv) {
  if (argc != 2) return 9;
  size_t words = 0;
  uint64_t* p = gs_read_file(argv[1], &words);
  if (!p || words < 3) { printf("FAIL: cannot read the input\n"); return 8; }
  const size_t nic = (size_t)p[0], npublic = (size_t)p[1], n = (size_t)p[2];
  if (n == 0 || words != 3 + 144 + nic * 12 + n * npublic * 4 + n * 108) { printf("FAIL: the input has the wrong length\n"); return 8; }
  uint64_t* q = p + 3;
  const uint64_t* vka = gs_take(&q, 24);
  const uint64_t* vkb = gs_take(&q, 12);
  const uint64_t* vkc = gs_take(&q, 24);
  const uint64_t* g1kbg = gs_take(&q, 12);
  const uint64_t* g2kbg = gs_take(&q, 24);
  const uint64_t* g2kg = gs_take(&q, 24);
  const uint64_t* vkz = gs_take(&q, 24);
  const uint64_t* ic = gs_take(&q, nic * 12);
  const uint64_t* pub = gs_take(&q, n * npublic * 4);
  const uint64_t* proofs = gs_take(&q, n * 108);

  int dev = 0;
  CHECK(gs_init(&dev, 1));
  int* each = (int*)malloc(2 * n * sizeof(int));
  if (!each) return 7;
  int* failed = each + n;
  uint64_t nbad = 0;
  CHECK(gs_pinocchio_verify_each(vka, vkb, vkc, g1kbg, g2kbg, g2kg, vkz, ic, nic, pub, npublic, proofs, n, each, failed, &nbad));
  printf("device: ");
  for (size_t i = 0; i < n; ++i) putchar(each[i] ? '0' : (failed[i] ? '0' + failed[i] : 'x'));
  printf(" (%" PRIu64 " rejected)\nhost:   ", nbad);
  for (size_t i = 0; i < n; ++i) {
    int one = 0, which = 0;
    CHECK(gs_pinocchio_verify(vka, vkb, vkc, g1kbg, g2kbg, g2kg, vkz, ic, nic, pub + i * npublic * 4, npublic, proofs + i * 108, &one, &which));
    putchar(one ? '0' : (which ? '0' + which : 'x'));
  }
  putchar('\n');
  if (gs_pinocchio_verify_each(vka, vkb, vkc, g1kbg, g2kbg, g2kg, vkz, ic, npublic, pub, npublic, proofs, n, each, failed, &nbad) != GS_ERR_SHAPE) {
    printf("FAIL: too few IC points were accepted\n");
    return 2;
  }
  if (gs_pinocchio_verify_each(vka, vkb, vkc, g1kbg, g2kbg, g2kg, vkz, ic, nic, pub, npublic, proofs, n, NULL, failed, &nbad) != GS_ERR_ARG) {
    printf("FAIL: a null verdict array was accepted\n");
    return 2;
  }
  CHECK(gs_pinocchio_verify_each(vka, vkb, vkc, g1kbg, g2kbg, g2kg, vkz, ic, nic, pub, npublic, proofs, n, each, NULL, NULL));   /* both optional */
  free(each);
  gs_shutdown();
  return 0;
}
