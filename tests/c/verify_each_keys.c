/* gosnarkhip.Groth16VkCreate + Groth16VerifyEachKeys (go/gosnarkhip/pairing_device.go), as C: a process without Python reads several
 * verification keys and a batch of proofs that each name their key, prepares every key once (gs_groth16_vk_create), asks
 * gs_groth16_verify_each_keys for a verdict per proof, asks the host's gs_groth16_verify about every proof under the key its label
 * names, and prints both as strings of 0s and 1s with the count of rejected proofs.
 * argv: a file of little-endian u64 words: nkeys, nproofs; per key nic, alpha (12), beta gamma delta (3 x 24), IC (nic x 12); then the
 * key index of every proof (nproofs words), the public signals concatenated in proof order (proof i: nic(key) - 1 signals of 4
 * words), A (nproofs x 12), B (nproofs x 24), C (nproofs x 12)  (tests/c_util.py). */
#include <inttypes.h>

#include "instance.h"

#define MAX_KEYS 16

int main(int argc, char** argv) {
  if (argc != 2) return 9;
  size_t words = 0;
  uint64_t* p = gs_read_file(argv[1], &words);
  if (!p || words < 2) { printf("FAIL: cannot read the input\n"); return 8; }
  const size_t nkeys = (size_t)p[0], n = (size_t)p[1];
  if (nkeys == 0 || nkeys > MAX_KEYS || n == 0) { printf("FAIL: the input has the wrong shape\n"); return 8; }
  uint64_t* q = p + 2;
  const uint64_t *alpha[MAX_KEYS], *beta[MAX_KEYS], *gamma[MAX_KEYS], *delta[MAX_KEYS], *ic[MAX_KEYS];
  size_t nic[MAX_KEYS];
  for (size_t k = 0; k < nkeys; ++k) {
    nic[k] = (size_t)*gs_take(&q, 1);
    alpha[k] = gs_take(&q, 12);
    beta[k] = gs_take(&q, 24);
    gamma[k] = gs_take(&q, 24);
    delta[k] = gs_take(&q, 24);
    ic[k] = gs_take(&q, nic[k] * 12);
  }
  const uint64_t* label = gs_take(&q, n);
  uint32_t* key_of_proof = (uint32_t*)malloc(n * sizeof(uint32_t));
  const uint64_t** pub_of = (const uint64_t**)malloc(n * sizeof(uint64_t*));
  if (!key_of_proof || !pub_of) return 7;
  const uint64_t* pub = q;
  for (size_t i = 0; i < n; ++i) {
    if (label[i] >= nkeys) { printf("FAIL: the input names a key it does not hold\n"); return 8; }
    key_of_proof[i] = (uint32_t)label[i];
    pub_of[i] = gs_take(&q, (nic[label[i]] - 1) * 4);
  }
  const uint64_t* a = gs_take(&q, n * 12);
  const uint64_t* b = gs_take(&q, n * 24);
  const uint64_t* c = gs_take(&q, n * 12);
  if ((size_t)(q - p) != words) { printf("FAIL: the input has the wrong length\n"); return 8; }

  int dev = 0;
  CHECK(gs_init(&dev, 1));
  gs_handle keys[MAX_KEYS];
  for (size_t k = 0; k < nkeys; ++k) CHECK(gs_groth16_vk_create(alpha[k], beta[k], gamma[k], delta[k], ic[k], nic[k], &keys[k]));
  int* each = (int*)malloc(n * sizeof(int));
  if (!each) return 7;
  uint64_t nbad = 0;
  CHECK(gs_groth16_verify_each_keys(keys, nkeys, key_of_proof, pub, a, b, c, n, each, &nbad));
  printf("device: ");
  for (size_t i = 0; i < n; ++i) putchar(each[i] ? '1' : '0');
  printf(" (%" PRIu64 " rejected)\nhost:   ", nbad);
  for (size_t i = 0; i < n; ++i) {
    const size_t k = key_of_proof[i];
    int one = 0;
    CHECK(gs_groth16_verify(alpha[k], beta[k], gamma[k], delta[k], ic[k], nic[k], pub_of[i], nic[k] - 1, a + i * 12, b + i * 24, c + i * 12, &one));
    putchar(one ? '1' : '0');
  }
  putchar('\n');
  key_of_proof[0] = (uint32_t)nkeys;
  each[0] = 7;
  if (gs_groth16_verify_each_keys(keys, nkeys, key_of_proof, pub, a, b, c, n, each, &nbad) != GS_ERR_ARG || each[0] != 7) {
    printf("FAIL: a key index past the end was accepted\n");
    return 2;
  }
  key_of_proof[0] = (uint32_t)label[0];
  if (gs_groth16_verify_each_keys(keys, nkeys, key_of_proof, pub, a, b, c, n, NULL, &nbad) != GS_ERR_ARG) {
    printf("FAIL: a null verdict array was accepted\n");
    return 2;
  }
  for (size_t k = 0; k < nkeys; ++k) CHECK(gs_free(keys[k]));
  free(each);
  free(key_of_proof);
  free(pub_of);
  gs_shutdown();
  return 0;
}
