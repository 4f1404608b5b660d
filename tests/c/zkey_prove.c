/* gosnarkhip.NewGroth16KeyZkey + UploadR1CSZkey (go/gosnarkhip/zkey.go), as C: a process without Python walks circuit.zkey and
 * witness.wtns itself, hands the sections to the device as they lie in the file, takes a host-buffer witness ticket and prints the
 * proof (32 words, hex).  r = s' = the constants below.
 * argv: circuit.zkey, witness.wtns. */
#include "instance.h"

typedef struct { const uint8_t* p; uint64_t len; } section;

/* the container of both files: magic, u32 version, u32 nSections, then (u32 id, u64 length, payload)* in any order */
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
  uint8_t* b = (uint8_t*)malloc(*size + 1);      /* + 1: the sections start at odd offsets; nothing below needs alignment */
  if (b && fread(b, 1, *size, f) != *size) { free(b); b = NULL; }
  fclose(f);
  return b;
}

int main(int argc, char** argv) {
  if (argc != 3) return 9;
  size_t zsize = 0, wsize = 0;
  uint8_t* zf = read_bytes(argv[1], &zsize);
  uint8_t* wf = read_bytes(argv[2], &wsize);
  section z[11], w[3];
  memset(z, 0, sizeof z);
  memset(w, 0, sizeof w);
  if (!zf || !wf || walk(zf, zsize, "zkey", z, 10) || walk(wf, wsize, "wtns", w, 2)) { printf("FAIL: cannot walk the files\n"); return 8; }
  for (int id = 1; id <= 9; ++id) if (!z[id].p) { printf("FAIL: zkey section %d is missing\n", id); return 7; }
  if (!w[1].p || !w[2].p) { printf("FAIL: wtns section missing\n"); return 7; }
  uint32_t nvars, npublic, m, ncoefs, nwitness;
  const uint8_t* h = z[2].p + 4 + 32 + 4 + 32;          /* behind n8q, q, n8r, r */
  memcpy(&nvars, h, 4); memcpy(&npublic, h + 4, 4); memcpy(&m, h + 8, 4);
  h += 12;                                              /* alpha1, beta1, beta2, gamma2, delta1, delta2 */
  const uint8_t *alpha1 = h, *beta1 = h + 64, *beta2 = h + 128, *delta1 = h + 384, *delta2 = h + 448;
  memcpy(&ncoefs, z[4].p, 4);
  memcpy(&nwitness, w[1].p + 36, 4);
  size_t k = 0;
  while (((size_t)1 << k) < m) ++k;
  if (nwitness != nvars || w[2].len != (uint64_t)nwitness * 32 || z[4].len != 4 + (uint64_t)ncoefs * 44) { printf("FAIL: counts\n"); return 6; }

  int dev = 0, inf[3];
  gs_handle at, b1, b2, cd, he, one, key, r1cs;
  uint64_t g1s[36], g2s[48], proof[32], ticket = 0;
  const uint64_t r[4] = {0x1234567890abcdefull, 0x1234567890abcdefull, 0, 0}, s[4] = {0xfedcba0987654321ull, 0xfedcba0987654321ull, 0, 0};
  CHECK(gs_init(&dev, 1));
  CHECK(gs_g1_upload_affine_mont(z[5].p, nvars, &at));
  CHECK(gs_g1_upload_affine_mont(z[6].p, nvars, &b1));
  CHECK(gs_g2_upload_affine_mont(z[7].p, nvars, &b2));
  uint8_t* cfull = (uint8_t*)calloc(nvars, 64);         /* section 8 leaves out the signals 0 .. nPublic: infinity there */
  memcpy(cfull + (size_t)(npublic + 1) * 64, z[8].p, z[8].len);
  CHECK(gs_g1_upload_affine_mont(cfull, nvars, &cd));
  CHECK(gs_g1_upload_affine_mont(z[9].p, m, &he));
  /* the single points of the header: converted on the device like the arrays, read back as Jacobian limbs */
  const uint8_t* singles1[3] = {alpha1, beta1, delta1};
  const uint8_t* singles2[2] = {beta2, delta2};
  for (int i = 0; i < 3; ++i) {
    CHECK(gs_g1_upload_affine_mont(singles1[i], 1, &one));
    CHECK(gs_g1_download(one, g1s + 12 * i, 1));
    CHECK(gs_free(one));
  }
  for (int i = 0; i < 2; ++i) {
    CHECK(gs_g2_upload_affine_mont(singles2[i], 1, &one));
    CHECK(gs_g2_download(one, g2s + 24 * i, 1));
    CHECK(gs_free(one));
  }
  CHECK(gs_groth16_pk_create_domain(at, b1, b2, cd, he, g1s, g1s + 12, g1s + 24, g2s, g2s + 24, k, nvars, npublic, &key));
  CHECK(gs_free(at)); CHECK(gs_free(b1)); CHECK(gs_free(b2)); CHECK(gs_free(cd)); CHECK(gs_free(he));
  CHECK(gs_r1cs_upload_zkey(k, nvars, z[4].p + 4, ncoefs, &r1cs));
  uint64_t* wit = (uint64_t*)malloc((size_t)nwitness * 32);    /* the ABI's w is uint64_t*: give it an aligned copy */
  memcpy(wit, w[2].p, (size_t)nwitness * 32);
  CHECK(gs_groth16_prove_witness_host_begin(key, r1cs, wit, nwitness, r, s, &ticket));
  CHECK(gs_groth16_prove_end(ticket, proof, inf));
  if (inf[0] || inf[1] || inf[2]) { printf("FAIL: a proof element is the point at infinity\n"); return 5; }
  for (int i = 0; i < 32; ++i) printf("%016llx%c", (unsigned long long)proof[i], i == 31 ? '\n' : ' ');
  CHECK(gs_free(key)); CHECK(gs_free(r1cs));
  gs_shutdown();
  return 0;
}
