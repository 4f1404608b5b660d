/* gosnarkhip.UploadR1CSDomain + (*Groth16Key).DeriveEvalBasisDomain / SetEvalBasisDomain (go/gosnarkhip/domain.go), as C: a snarkjs /
 * circom Groth16 key -- a QAP over the domain of the 2^k-th roots of unity, Z = x^m - 1 -- is uploaded like any key, its sparse system
 * with gs_r1cs_upload_domain, and witnesses are proved through the ordinary witness entry points.  Checked here: px of the domain system
 * equals the instance's; the proof is the same from px, from the witness without the coset evaluation-basis array, with the derived
 * array (blocking and as a host-buffer ticket) and with the array read back and attached again; the verifier accepts it for the
 * instance's public signals and rejects it for others.
 * argv: r1cs file, groth16 instance, log2 of the domain, output (32 proof words). */
#include "instance.h"

int main(int argc, char** argv) {
  if (argc != 5) return 9;
  r1cs_instance q;
  groth_instance g;
  if (read_r1cs_instance(argv[1], &q) || read_groth_instance(argv[2], &g)) return 8;
  const size_t k = (size_t)atoi(argv[3]), m = (size_t)1 << k;
  if (q.m != g.m || g.npx != 2 * m - 1 || g.nz != m + 1 || q.n > m) { printf("FAIL: instance shapes\n"); return 7; }
  int dev = 0, inf[3], inf2[3], ok = 0;
  gs_handle key, r1cs, w, px = 0, ebases;
  uint64_t want[32], got[32], jac[48], ticket = 0;
  size_t count = 0;
  uint64_t* pxback = (uint64_t*)malloc(g.npx * 32);
  uint64_t* e = (uint64_t*)malloc(m * 12 * 8);
  CHECK(gs_init(&dev, 1));
  if (upload_groth_pk(&g, &key)) return 3;
  CHECK(gs_r1cs_upload_domain(k, q.n, q.m, q.rowptr[0], q.col[0], q.val[0], q.rowptr[1], q.col[1], q.val[1], q.rowptr[2], q.col[2], q.val[2], &r1cs));
  CHECK(gs_scalars_upload(g.w, g.m, &w));
  /* px of the domain system: 2m - 1 coefficients */
  CHECK(gs_r1cs_px(r1cs, w, &px));
  CHECK(gs_scalars_download(px, pxback, g.npx));
  if (memcmp(pxback, g.px, g.npx * 32) != 0) { printf("FAIL: px differs\n"); return 4; }
  CHECK(gs_groth16_prove_resident(key, w, px, g.rs, g.rs + 4, want, inf));
  /* the witness alone, the key without the array: px and the quotient by x^m - 1 inside */
  CHECK(gs_groth16_prove_witness_host(key, r1cs, g.w, g.m, g.rs, g.rs + 4, got, inf2));
  if (memcmp(want, got, sizeof want) != 0 || memcmp(inf, inf2, sizeof inf) != 0) { printf("FAIL: witness route without the array\n"); return 5; }
  /* ... with the coset evaluation-basis array derived from hExps */
  CHECK(gs_groth16_pk_derive_eval_domain(key, k));
  CHECK(gs_pk_eval_count(key, &count));
  if (count != m) { printf("FAIL: %zu evaluation-basis points\n", count); return 6; }
  memset(got, 0, sizeof got);
  CHECK(gs_groth16_prove_witness_host(key, r1cs, g.w, g.m, g.rs, g.rs + 4, got, inf2));
  if (memcmp(want, got, sizeof want) != 0 || memcmp(inf, inf2, sizeof inf) != 0) { printf("FAIL: evaluation-basis route\n"); return 10; }
  memset(got, 0, sizeof got);
  CHECK(gs_groth16_prove_witness_host_begin(key, r1cs, g.w, g.m, g.rs, g.rs + 4, &ticket));
  CHECK(gs_groth16_prove_end(ticket, got, inf2));
  if (memcmp(want, got, sizeof want) != 0 || memcmp(inf, inf2, sizeof inf) != 0) { printf("FAIL: host-buffer ticket\n"); return 11; }
  /* ... and with the array as a key file would bring it */
  CHECK(gs_groth16_pk_export(key, 7, e, m));
  CHECK(gs_g1_upload(e, m, &ebases));
  CHECK(gs_groth16_pk_set_eval_domain(key, ebases, k));
  CHECK(gs_free(ebases));
  memset(got, 0, sizeof got);
  CHECK(gs_groth16_prove_witness(key, r1cs, w, g.rs, g.rs + 4, got, inf2));
  if (memcmp(want, got, sizeof want) != 0 || memcmp(inf, inf2, sizeof inf) != 0) { printf("FAIL: attached array\n"); return 12; }
  /* verify */
  proof_to_jacobian(got, inf2, jac);
  CHECK(gs_groth16_verify(g.vka, g.vk2, g.vk2 + 24, g.vk2 + 48, g.ic, g.nic, g.pub, g.nic - 1, jac, jac + 12, jac + 36, &ok));
  if (!ok) { printf("FAIL: the proof does not verify\n"); return 13; }
  g.pub[0] += 1;
  CHECK(gs_groth16_verify(g.vka, g.vk2, g.vk2 + 24, g.vk2 + 48, g.ic, g.nic, g.pub, g.nic - 1, jac, jac + 12, jac + 36, &ok));
  if (ok) { printf("FAIL: the proof verifies another statement\n"); return 14; }
  if (write_words(argv[4], got, 32)) return 15;
  CHECK(gs_free(px)); CHECK(gs_free(w)); CHECK(gs_free(r1cs)); CHECK(gs_free(key));
  gs_shutdown();
  free(pxback); free(e);
  printf("OK\n");
  return 0;
}
