/* gosnarkhip.ContributePtauArrays, ScalePowersG1 / ScalePowersG2 (go/gosnarkhip/ptau.go), as C: a process without Python walks a
 * powers-of-tau file itself, hands its sections to the device as they lie there, multiplies one contribution (tau, alpha, beta) into
 * them on the points and writes the contributed sections as the file holds them:  tauG1 | tauG2 | alphaTauG1 | betaTauG1 | betaG2.
 * argv: transcript.ptau, scalars.bin (12 words: tau, alpha, beta as four limbs each), output file. */
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
  size_t psize = 0, swords = 0;
  uint8_t* pf = read_bytes(argv[1], &psize);
  uint64_t* s = gs_read_file(argv[2], &swords);
  section t[7];
  memset(t, 0, sizeof t);
  if (!pf || !s || swords != 12 || walk(pf, psize, "ptau", t, 6)) { printf("FAIL: cannot read the inputs\n"); return 8; }
  for (int id = 1; id <= 6; ++id) if (!t[id].p) { printf("FAIL: ptau section %d is missing\n", id); return 7; }
  uint32_t power;
  memcpy(&power, t[1].p + 36, 4);
  const size_t n = (size_t)1 << power, n1 = 2 * n - 1;
  if (t[2].len != n1 * 64 || t[3].len != n * 128 || t[4].len != n * 64 || t[5].len != n * 64 || t[6].len != 128) { printf("FAIL: section lengths\n"); return 6; }
  const uint64_t *tau = s, *alpha = s + 4, *beta = s + 8, one[4] = {1, 0, 0, 0};

  int dev = 0;
  gs_handle in[5], out[5];
  CHECK(gs_init(&dev, 1));
  CHECK(gs_g1_upload_affine_mont(t[2].p, n1, &in[0]));
  CHECK(gs_g2_upload_affine_mont(t[3].p, n, &in[1]));
  CHECK(gs_g1_upload_affine_mont(t[4].p, n, &in[2]));
  CHECK(gs_g1_upload_affine_mont(t[5].p, n, &in[3]));
  CHECK(gs_g2_upload_affine_mont(t[6].p, 1, &in[4]));
  CHECK(gs_g1_scale_powers(in[0], 0, n1, one, tau, &out[0]));
  CHECK(gs_g2_scale_powers(in[1], 0, n, one, tau, &out[1]));
  CHECK(gs_g1_scale_powers(in[2], 0, n, alpha, tau, &out[2]));
  CHECK(gs_g1_scale_powers(in[3], 0, n, beta, tau, &out[3]));
  CHECK(gs_g2_scale_powers(in[4], 0, 1, beta, one, &out[4]));

  const size_t total = (n1 + 2 * n) * 64 + (n + 1) * 128;
  uint8_t* b = (uint8_t*)malloc(total);
  size_t at = 0;
  CHECK(gs_g1_download_affine_mont(out[0], b + at, n1)); at += n1 * 64;
  CHECK(gs_g2_download_affine_mont(out[1], b + at, n)); at += n * 128;
  CHECK(gs_g1_download_affine_mont(out[2], b + at, n)); at += n * 64;
  CHECK(gs_g1_download_affine_mont(out[3], b + at, n)); at += n * 64;
  CHECK(gs_g2_download_affine_mont(out[4], b + at, 1)); at += 128;
  FILE* f = fopen(argv[3], "wb");
  if (!f || fwrite(b, 1, total, f) != total) { printf("FAIL: cannot write %s\n", argv[3]); return 5; }
  fclose(f);
  printf("OK power %u, %zu bytes\n", power, at);
  for (int i = 0; i < 5; ++i) { CHECK(gs_free(in[i])); CHECK(gs_free(out[i])); }
  gs_shutdown();
  return 0;
}
