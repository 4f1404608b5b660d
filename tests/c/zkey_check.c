/* gosnarkhip.CheckKey / CheckPtau (go/gosnarkhip/zkey_check.go), as C: a process without Python walks a circuit.zkey and a powers-of-tau
 * file itself, hands their sections to the device as they lie there and asks gs_ptau_check and gs_groth16_key_check whether the
 * transcript is consistent and the key is the key of this circuit over it.  Prints one line per entry point, "ACCEPT ..." or
 * "REJECT ...: <the failed checks>"; the exit status is 0 either way (anything else is a failure of the driver).
 * argv: r1cs.bin (tests/c_util._blob layout of tests/test_gpu_zkey_check_c.py: the system with its public rows; toxic[0] = log2 of the
 *       domain, toxic[1] = the challenge), transcript.ptau, circuit.zkey. */
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

static void verdict(const char* what, const gs_check_report* rep, const char* const* names) {
  if (!rep->failed) { printf("ACCEPT %s: %u checks\n", what, rep->nchecks); return; }
  printf("REJECT %s:", what);
  for (uint32_t i = 0; i < rep->nchecks; ++i) if (!rep->check[i].ok) printf(" [%s]", names[i]);
  printf("\n");
}

int main(int argc, char** argv) {
  static const char* const key_names[GS_CHECK_MAX] = {"coefs A", "coefs B", "A", "B1", "B2", "IC", "C", "H"};
  static const char* const ptau_names[GS_CHECK_MAX] = {"g1", "g2", "tau", "tauG1", "tauG2", "alphaTauG1", "betaTauG1", "betaG2"};
  if (argc != 4) return 9;
  r1cs_instance g;
  size_t psize = 0, zsize = 0;
  uint8_t* pf = read_bytes(argv[2], &psize);
  uint8_t* zf = read_bytes(argv[3], &zsize);
  section t[7], z[10];
  memset(t, 0, sizeof t);
  memset(z, 0, sizeof z);
  if (read_r1cs_instance(argv[1], &g) || g.ntoxic != 2 || !pf || !zf || walk(pf, psize, "ptau", t, 6) || walk(zf, zsize, "zkey", z, 9)) {
    printf("FAIL: cannot read the inputs\n");
    return 8;
  }
  for (int id = 1; id <= 6; ++id) if (!t[id].p) { printf("FAIL: ptau section %d is missing\n", id); return 7; }
  for (int id = 2; id <= 9; ++id) if (!z[id].p) { printf("FAIL: zkey section %d is missing\n", id); return 7; }
  size_t in_bytes = 0, rep_bytes = 0;
  CHECK(gs_check_abi_sizes(&in_bytes, &rep_bytes));
  if (in_bytes != sizeof(gs_key_check_input) || rep_bytes != sizeof(gs_check_report)) { printf("FAIL: the library was built from another header\n"); return 6; }
  const size_t k = (size_t)g.toxic[0], m = (size_t)1 << k;
  uint32_t power, nvars, npublic, domain;
  memcpy(&power, t[1].p + 36, 4);
  memcpy(&nvars, z[2].p + 72, 4);
  memcpy(&npublic, z[2].p + 76, 4);
  memcpy(&domain, z[2].p + 80, 4);
  if (power < k || domain != m || nvars != g.m || npublic != g.npublic || z[2].len != 84 + 3 * 64 + 3 * 128) { printf("FAIL: the files do not fit each other\n"); return 6; }
  const size_t ntau = power > k ? 2 * m : 2 * m - 1;

  int dev = 0;
  gs_key_check_input in;
  gs_check_report rep;
  gs_handle d2, full1, full2, fulla, fullb, bg2;
  uint64_t jac[24];
  memset(&in, 0, sizeof in);
  CHECK(gs_init(&dev, 1));
  /* the transcript against itself, over all the powers it holds */
  CHECK(gs_g1_upload_affine_mont(t[2].p, ((size_t)2 << power) - 1, &full1));
  CHECK(gs_g2_upload_affine_mont(t[3].p, (size_t)1 << power, &full2));
  CHECK(gs_g1_upload_affine_mont(t[4].p, (size_t)1 << power, &fulla));
  CHECK(gs_g1_upload_affine_mont(t[5].p, (size_t)1 << power, &fullb));
  CHECK(gs_g2_upload_affine_mont(t[6].p, 1, &bg2));
  CHECK(gs_g2_download(bg2, jac, 1));
  CHECK(gs_ptau_check(full1, full2, fulla, fullb, jac, power, g.toxic + 4, &rep));
  verdict("transcript", &rep, ptau_names);
  CHECK(gs_free(full1)); CHECK(gs_free(full2)); CHECK(gs_free(fulla)); CHECK(gs_free(fullb)); CHECK(gs_free(bg2));
  /* the key against circuit and transcript */
  CHECK(gs_g1_upload_affine_mont(t[2].p, ntau, &in.tau_g1));
  CHECK(gs_g2_upload_affine_mont(t[3].p, m, &in.tau_g2));
  CHECK(gs_g1_upload_affine_mont(t[4].p, m, &in.alpha_tau_g1));
  CHECK(gs_g1_upload_affine_mont(t[5].p, m, &in.beta_tau_g1));
  CHECK(gs_g1_upload_affine_mont(z[3].p, npublic + 1, &in.ic));
  CHECK(gs_g1_upload_affine_mont(z[5].p, nvars, &in.a));
  CHECK(gs_g1_upload_affine_mont(z[6].p, nvars, &in.b1));
  CHECK(gs_g2_upload_affine_mont(z[7].p, nvars, &in.b2));
  CHECK(gs_g1_upload_affine_mont(z[8].p, nvars - npublic - 1, &in.c));
  CHECK(gs_g1_upload_affine_mont(z[9].p, m, &in.h));
  CHECK(gs_r1cs_upload_zkey(k, nvars, z[4].p + 4, (z[4].len - 4) / 44, &in.key_system));
  CHECK(gs_r1cs_upload_domain(k, g.n, nvars, g.rowptr[0], g.col[0], g.val[0], g.rowptr[1], g.col[1], g.val[1], g.rowptr[2], g.col[2], g.val[2],
                              &in.circuit_system));
  CHECK(gs_g2_upload_affine_mont(z[2].p + z[2].len - 128, 1, &d2));      /* delta2 ends the header */
  CHECK(gs_g2_download(d2, in.delta2, 1));
  memcpy(in.challenge, g.toxic + 4, 32);
  in.log2_domain = k;
  in.npublic = npublic;
  CHECK(gs_groth16_key_check(&in, &rep));
  verdict("key", &rep, key_names);
  gs_timing tm;
  CHECK(gs_last_timing(&tm));
  printf("device %.3f ms (plans %.3f, accumulate %.3f, reduce %.3f, scalars %.3f)\n", tm.total_ms, tm.plan_ms, tm.accumulate_ms, tm.reduce_ms, tm.poly_ms);
  const gs_handle all[] = {in.a, in.b1, in.b2, in.ic, in.c, in.h, in.key_system, in.circuit_system, in.tau_g1, in.tau_g2, in.alpha_tau_g1, in.beta_tau_g1, d2};
  for (size_t i = 0; i < sizeof all / sizeof all[0]; ++i) CHECK(gs_free(all[i]));
  gs_shutdown();
  return 0;
}
