/* gosnarkhip.PreparePtauArrays, LagrangeLevelsG1 / LagrangeLevelsG2, CheckLagrangeLevelsG1 / CheckLagrangeLevelsG2
 * (go/gosnarkhip/ptau.go), as C: a process without Python walks a powers-of-tau file itself, hands its array sections to the device as
 * they lie there, computes the Lagrange bases of every power-of-two domain in one call per section, checks each result against its
 * section with two sums, and writes the prepared sections as the file holds them:  12 | 13 | 14 | 15.
 * argv: transcript.ptau, output file. */
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
  if (argc != 3) return 9;
  size_t psize = 0;
  uint8_t* pf = read_bytes(argv[1], &psize);
  section t[7];
  memset(t, 0, sizeof t);
  if (!pf || walk(pf, psize, "ptau", t, 6)) { printf("FAIL: cannot read the input\n"); return 8; }
  for (int id = 1; id <= 6; ++id) if (!t[id].p) { printf("FAIL: ptau section %d is missing\n", id); return 7; }
  uint32_t power;
  memcpy(&power, t[1].p + 36, 4);
  const size_t n = (size_t)1 << power, n1 = 2 * n - 1;
  if (power > 24 || t[2].len != n1 * 64 || t[3].len != n * 128 || t[4].len != n * 64 || t[5].len != n * 64) { printf("FAIL: section lengths\n"); return 6; }
  const uint64_t challenge[4] = {0x9e3779b97f4a7c15ULL, 0x243f6a8885a308d3ULL, 0x13198a2e03707344ULL, 0x0a4093822299f31dULL};

  int dev = 0;
  gs_handle in[4], out[4];
  gs_check_result res[4];
  CHECK(gs_init(&dev, 1));
  CHECK(gs_g1_upload_affine_mont(t[2].p, n1, &in[0]));
  CHECK(gs_g2_upload_affine_mont(t[3].p, n, &in[1]));
  CHECK(gs_g1_upload_affine_mont(t[4].p, n, &in[2]));
  CHECK(gs_g1_upload_affine_mont(t[5].p, n, &in[3]));
  CHECK(gs_g1_lagrange_levels(in[0], 0, power + 1, &out[0]));      /* 2^(power+1) - 1 points: the last of level power + 1 is infinity */
  CHECK(gs_g2_lagrange_levels(in[1], 0, power, &out[1]));
  CHECK(gs_g1_lagrange_levels(in[2], 0, power, &out[2]));
  CHECK(gs_g1_lagrange_levels(in[3], 0, power, &out[3]));
  CHECK(gs_g1_lagrange_levels_check(in[0], out[0], power + 1, challenge, &res[0]));
  CHECK(gs_g2_lagrange_levels_check(in[1], out[1], power, challenge, &res[1]));
  CHECK(gs_g1_lagrange_levels_check(in[2], out[2], power, challenge, &res[2]));
  CHECK(gs_g1_lagrange_levels_check(in[3], out[3], power, challenge, &res[3]));
  for (int i = 0; i < 4; ++i) if (!res[i].ok) { printf("FAIL: section %d does not pass its check\n", 12 + i); return 4; }

  const size_t c12 = 4 * n - 1, c = 2 * n - 1, total = (c12 + 2 * c) * 64 + c * 128;
  uint8_t* b = (uint8_t*)malloc(total);
  size_t at = 0;
  CHECK(gs_g1_download_affine_mont(out[0], b + at, c12)); at += c12 * 64;
  CHECK(gs_g2_download_affine_mont(out[1], b + at, c)); at += c * 128;
  CHECK(gs_g1_download_affine_mont(out[2], b + at, c)); at += c * 64;
  CHECK(gs_g1_download_affine_mont(out[3], b + at, c)); at += c * 64;
  FILE* f = fopen(argv[2], "wb");
  if (!f || fwrite(b, 1, total, f) != total) { printf("FAIL: cannot write %s\n", argv[2]); return 5; }
  fclose(f);
  printf("OK power %u, %zu bytes\n", power, at);
  for (int i = 0; i < 4; ++i) { CHECK(gs_free(in[i])); CHECK(gs_free(out[i])); }
  gs_shutdown();
  return 0;
}
