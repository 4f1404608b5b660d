// The seam between the verifier entry points (verify.hip: host work per key and per proof) and the device pipeline under them
// (pairing_device.hip).  Every function sets the last error and returns a GS_* code; `fn` is the public entry point's name.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "../../include/gosnark_hip.h"
#include "pairing.h"
#include "verify_plan.h"

namespace gs {

constexpr size_t kLineStd = (size_t)pairing::kPreparedSteps * 16;       // u64 words of one prepared list (pairing.h, prepare_g2_lines)

// what verify.hip's prepare_groth16_key makes of alpha, beta, gamma, delta
struct Groth16KeyWords {
  uint64_t ab[48];                                                       // the Miller value of e(alpha, beta), standard encoding
  std::vector<uint64_t> lines;                                           // gamma's prepared list, then delta's; zeros for an infinite point
  bool skip_gamma = false, skip_delta = false;                           // gamma / delta is the point at infinity: its pair contributes one
};

// the keys of one gs_groth16_verify_each* call: prepared objects (gs_groth16_vk_create), or ONE key made for this call only from an
// uploaded IC array and its words, with `npublic` signals per proof (at most the array's points - 1); nothing of it outlives the call
struct Groth16CallKeys {
  const gs_handle* keys = nullptr;
  size_t nkeys = 0;
  gs_handle ic = 0;
  size_t npublic = 0;
  const Groth16KeyWords* words = nullptr;
};

// for gs_groth16_verify_batch: the product of the n Miller values, before the final exponentiation; the caller multiplies its own pairs in
int miller_product(const char* fn, gs_handle g1, size_t poff, gs_handle g2, size_t qoff, size_t n, pairing::Fp12* out);

// for gs_groth16_vk_create: the key object over an uploaded IC array (the object keeps the array alive, the caller frees its handle)
int groth16_vk_install(const char* fn, gs_handle hic, size_t nic, const Groth16KeyWords& words, gs_handle* out);
// npublic of every prepared key; GS_ERR_ARG for a handle that is not one
int groth16_vk_info(const char* fn, const gs_handle* keys, size_t nkeys, uint32_t* npublic);

// per SLOT of the plan (verify_plan.h; 64 per group): is B in G2 and is the exponentiated product of the four pairs one.  a, b, c hold
// the proofs' points in slot order with infinity in the padded slots, pub the signals in slot order without padding.
int groth16_verify_slots_device(const char* fn, const Groth16CallKeys& keys, gs_handle ha, gs_handle hb, gs_handle hc, const VerifyGroup* groups,
                                size_t ngroups, const uint64_t* pub, uint64_t nsignals, int* member, int* is_one);

// for gs_pinocchio_verify_each: per proof, is PiB in G2 (member[i]) and is the exponentiated product of equation e + 1 one
// (one[e * n + i]).  g1 holds the proofs' seven G1 points as slabs of n (PiA, PiAp, PiBp, PiC, PiCp, PiH, PiKp), key = Vkb, G1Kbg;
// lines = the six prepared lists (Vka, Vkc, Vkz, G2Kbg, G2Kg, the generator), zeros for a list whose bit in skip_mask is set.
int pinocchio_verify_each_device(const char* fn, gs_handle g1, gs_handle hb, gs_handle hic, gs_handle key, const uint64_t* pub, size_t npublic, size_t n,
                                 const uint64_t* lines, unsigned skip_mask, int* member, int* one);

}  // namespace gs
