/* gosnarkhip.Groth16VerifyBatch and gosnarkhip.PairingProduct (go/gosnarkhip/pairing_device.go), as C: a process without Python reads
 * a verification key and a batch of proofs, asks gs_groth16_verify_batch for the verdict on the batch, asks the host's
 * gs_groth16_verify about every proof, and prints both.  Then it uploads the A and B of the batch and prints whether
 * prod_i e(A_i, B_i) is one according to gs_pairing_product and according to the host's gs_pairing_check.
 * argv: a file of little-endian u64 words: nic, npublic, nproofs, then alpha (12), beta gamma delta (3 x 24), IC (nic x 12), the public
 * signals (nproofs x npublic x 4), A (nproofs x 12), B (nproofs x 24), C (nproofs x 12), the challenge (4)  (tests/c_util.py). */
#include <inttypes.h>

#include "instance.h"

int main(int argc, char** argv) {
  if (argc != 2) return 9;
  size_t words = 0;
  uint64_t* p = gs_read_file(argv[1], &words);
  if (!p || words < 3) { printf("FAIL: cannot read the input\n"); return 8; }
  const size_t nic = (size_t)p[0], npublic = (size_t)p[1], n = (size_t)p[2];
  if (words != 3 + 12 + 72 + nic * 12 + n * npublic * 4 + n * 48 + 4) { printf("FAIL: the input has the wrong length\n"); return 8; }
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
  const uint64_t* challenge = gs_take(&q, 4);

  int dev = 0, ok = -1;
  CHECK(gs_init(&dev, 1));
  CHECK(gs_groth16_verify_batch(alpha, beta, gamma, delta, ic, nic, pub, npublic, a, b, c, n, challenge, &ok));
  size_t accepted = 0;
  for (size_t i = 0; i < n; ++i) {
    int one = 0;
    CHECK(gs_groth16_verify(alpha, beta, gamma, delta, ic, nic, pub + i * npublic * 4, npublic, a + i * 12, b + i * 24, c + i * 12, &one));
    accepted += one ? 1 : 0;
  }
  printf("batch of %zu: %s; one at a time: %zu accepted\n", n, ok ? "ACCEPT" : "REJECT", accepted);

  gs_handle ha, hb;
  uint64_t value[48];
  int is_one = -1, host_one = -1;
  CHECK(gs_g1_upload(a, n, &ha));
  CHECK(gs_g2_upload(b, n, &hb));
  CHECK(gs_pairing_product(ha, 0, hb, 0, n, value, &is_one));
  CHECK(gs_pairing_check(a, b, n, &host_one));
  printf("product of %zu pairings: device %s, host %s\n", n, is_one ? "one" : "not one", host_one ? "one" : "not one");
  if (gs_pairing_product(ha, 1, hb, 0, n, value, &is_one) != GS_ERR_SHAPE) { printf("FAIL: a range past the end was accepted\n"); return 2; }
  if (gs_pairing_product(ha, 0, hb, 0, n, NULL, NULL) != GS_ERR_ARG) { printf("FAIL: two null out-pointers were accepted\n"); return 2; }
  CHECK(gs_free(ha));
  CHECK(gs_free(hb));
  gs_shutdown();
  return 0;
}
