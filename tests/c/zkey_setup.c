/* gosnarkhip.SetupZkeyArrays, ScaleG1, DownloadG1AffineMont / DownloadG2AffineMont (go/gosnarkhip/setup_ptau.go), as C: a process
 * without Python walks a powers-of-tau file itself, hands its sections to the device as they lie there, builds the Lagrange bases and the
 * column sums of the circuit's domain R1CS and writes the arrays as a .zkey holds them:  A | B1 | K | H | K / toxic[1]  (G1, 64 bytes a
 * point) and then B2 (G2, 128 bytes a point).
 * argv: r1cs.bin (tests/c_util.write_r1cs: the system with its public rows; toxic[0] = log2 of the domain, toxic[1] = a scalar),
 *       transcript.ptau, output file. */
#include "instance.h"

typedef struct { const uint8_t* p; uint64_t len; } section;

static int walk(const uint8_t* f, size_t size, const char* magic, section* sec, uint32_t max_id) {
  if (size < 12 || memcmp(f, magic, 4) != 0) return 1;
  uint32_t nsec, id;
  uint64_t len;
  memcpy(&nsec, f + 8, 4);
  size_t pos = 12;
  for (uint32_t i = 0; i < nsec; ++i) {
    if (pos + 12 > size) return 1;
    memcpy(&id, f + pos, 4);
    memcpy(&len, f + pos + 4, 8);
    pos += 12;
    if (len > size - pos) return 1;
    if (id <= max_id) { sec[id].p = f + pos; sec[id].len = len; }
    pos += len;
  }
  return 0;
}

static uint8_t* read_bytes(const char* path, size_t* size) {
  FILE* f = fopen(path, "rb");
  if (!f) return NULL;
  fseek(f, 0, SEEK_END);
  *size = (size_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t* b = (uint8_t*)malloc(*size + 1);
  if (b && fread(b, 1, *size, f) != *size) { free(b); b = NULL; }
  fclose(f);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 4) return 9;
  r1cs_instance g;
  size_t psize = 0;
  uint8_t* pf = read_bytes(argv[2], &psize);
  section t[7];
  memset(t, 0, sizeof t);
  if (read_r1cs_instance(argv[1], &g) || g.ntoxic != 2 || !pf || walk(pf, psize, "ptau", t, 6)) { printf("FAIL: cannot read the inputs\n"); return 8; }
  for (int id = 1; id <= 6; ++id) if (!t[id].p) { printf("FAIL: ptau section %d is missing\n", id); return 7; }
  const size_t k = (size_t)g.toxic[0], m = (size_t)1 << k, nvars = g.m;
  uint32_t power;
  memcpy(&power, t[1].p + 36, 4);
  if (power < k) { printf("FAIL: the transcript is too small\n"); return 6; }
  const size_t ntau = power > k ? 2 * m : 2 * m - 1;     /* the points the odd half may read */

  int dev = 0;
  gs_handle tau1, tau2, at1, bt1, sys, l, l2, la, lb, a, b1, b2, kk, h, ks;
  CHECK(gs_init(&dev, 1));
  CHECK(gs_g1_upload_affine_mont(t[2].p, ntau, &tau1));
  CHECK(gs_g2_upload_affine_mont(t[3].p, m, &tau2));
  CHECK(gs_g1_upload_affine_mont(t[4].p, m, &at1));
  CHECK(gs_g1_upload_affine_mont(t[5].p, m, &bt1));
  CHECK(gs_r1cs_upload_domain(k, g.n, nvars, g.rowptr[0], g.col[0], g.val[0], g.rowptr[1], g.col[1], g.val[1], g.rowptr[2], g.col[2], g.val[2], &sys));
  CHECK(gs_g1_lagrange(tau1, 0, k, 0, &l));
  CHECK(gs_g1_lagrange(tau1, 0, k, 1, &h));
  CHECK(gs_g2_lagrange(tau2, 0, k, &l2));
  CHECK(gs_g1_lagrange(at1, 0, k, 0, &la));
  CHECK(gs_g1_lagrange(bt1, 0, k, 0, &lb));
  CHECK(gs_r1cs_colsum_g1(sys, l, 0, 0, &a));
  CHECK(gs_r1cs_colsum_g1(sys, 0, l, 0, &b1));
  CHECK(gs_r1cs_colsum_g2(sys, 0, l2, 0, &b2));
  CHECK(gs_r1cs_colsum_g1(sys, lb, la, l, &kk));
  CHECK(gs_free(l)); CHECK(gs_free(l2)); CHECK(gs_free(la)); CHECK(gs_free(lb));
  CHECK(gs_g1_scale(kk, g.toxic + 4, &ks));

  const size_t g1_bytes = (4 * nvars + m) * 64, total = g1_bytes + nvars * 128;
  uint8_t* out = (uint8_t*)malloc(total);
  CHECK(gs_g1_download_affine_mont(a, out, nvars));
  CHECK(gs_g1_download_affine_mont(b1, out + nvars * 64, nvars));
  CHECK(gs_g1_download_affine_mont(kk, out + 2 * nvars * 64, nvars));
  CHECK(gs_g1_download_affine_mont(h, out + 3 * nvars * 64, m));
  CHECK(gs_g1_download_affine_mont(ks, out + (3 * nvars + m) * 64, nvars));
  CHECK(gs_g2_download_affine_mont(b2, out + g1_bytes, nvars));
  FILE* f = fopen(argv[3], "wb");
  if (!f || fwrite(out, 1, total, f) != total) { printf("FAIL: cannot write %s\n", argv[3]); return 5; }
  fclose(f);
  printf("OK %zu variables, domain 2^%zu, %zu bytes\n", nvars, k, total);
  CHECK(gs_free(a)); CHECK(gs_free(b1)); CHECK(gs_free(b2)); CHECK(gs_free(kk)); CHECK(gs_free(ks)); CHECK(gs_free(h));
  CHECK(gs_free(tau1)); CHECK(gs_free(tau2)); CHECK(gs_free(at1)); CHECK(gs_free(bt1)); CHECK(gs_free(sys));
  gs_shutdown();
  return 0;
}
