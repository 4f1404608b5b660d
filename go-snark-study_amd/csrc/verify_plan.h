// The slot plan of gs_groth16_verify_each_keys (verify.hip, pairing_device.hip): proofs of many verification keys in one launch.
//
// The Miller-loop kernel is fast because the prepared lines of a key are the same words for every lane of a wave (a broadcast load), so
// a wave must not mix keys.  The plan therefore gives every key its own one-wave workgroups:
//   the proofs are grouped by key, stably (the order inside a key is the order of the input);
//   the run of a key with c proofs becomes ceil(c / 64) GROUPS of 64 SLOTS, the last of them padded (a key with no proof has no group);
//   the groups lie in the order of the keys, slot s belongs to group s / 64, and one group is one workgroup.
// A padded slot holds no proof (kVpNoProof): the point at infinity travels in it, the kernels compute on it and nobody reads the answer.
// The signals are uploaded in slot order without padding: the valid lanes of a group are its first `valid` ones and lane l of group g
// finds its npublic(key) signals at signal number sig_off(g) + l * npublic(key), so sig_off is the running sum of npublic over the
// slots in front that hold a proof.
//
// Pure host code with no dependency on the runtime: verify.hip and tests/host/verify_plan_host_test.hip include it.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace gs {

constexpr uint32_t kVpLanes = 64;                       // slots per group: one wave
constexpr uint32_t kVpNoProof = 0xffffffffu;

struct VerifyGroup {                                    // read by the kernels as it is (16 bytes)
  uint32_t key;                                         // index in the call's key table
  uint32_t valid;                                       // lanes 0 .. valid - 1 hold proofs, 1 <= valid <= 64
  uint64_t sig_off;                                     // number of the group's first signal (units of one 256-bit signal)
};

struct VerifyPlan {
  std::vector<VerifyGroup> groups;
  std::vector<uint32_t> proof_of_slot;                  // 64 per group; kVpNoProof in a padded slot
  std::vector<uint32_t> slot_of_proof;                  // nproofs
  uint64_t nsignals = 0;                                // signals of all proofs together
};

enum VerifyPlanStatus { kVpOk = 0, kVpBadKey = 1, kVpTooLarge = 2 };

// npublic_of_key: nkeys entries.  kVpBadKey: key_of_proof[*bad_proof] >= nkeys; kVpTooLarge: the slots (or the proofs) do not fit 32-bit
// indices.  On an error the plan's contents are unspecified.
inline VerifyPlanStatus plan_verify_slots(const uint32_t* key_of_proof, size_t nproofs, size_t nkeys, const uint32_t* npublic_of_key,
                                          VerifyPlan& plan, size_t* bad_proof = nullptr) {
  plan = VerifyPlan{};
  if (nproofs >= kVpNoProof) return kVpTooLarge;
  std::vector<uint64_t> count(nkeys, 0);
  for (size_t i = 0; i < nproofs; ++i) {
    if (key_of_proof[i] >= nkeys) {
      if (bad_proof) *bad_proof = i;
      return kVpBadKey;
    }
    count[key_of_proof[i]] += 1;
  }
  // the first slot of every key's run, the groups and their signal offsets
  std::vector<uint64_t> next(nkeys, 0);
  uint64_t slots = 0, signals = 0;
  for (size_t k = 0; k < nkeys; ++k) {
    next[k] = slots;
    for (uint64_t left = count[k]; left; left -= left < kVpLanes ? left : kVpLanes) {
      const uint32_t valid = (uint32_t)(left < kVpLanes ? left : kVpLanes);
      plan.groups.push_back(VerifyGroup{(uint32_t)k, valid, signals});
      signals += (uint64_t)valid * npublic_of_key[k];
      slots += kVpLanes;
    }
    if (slots >= kVpNoProof) return kVpTooLarge;
  }
  plan.nsignals = signals;
  plan.proof_of_slot.assign((size_t)slots, kVpNoProof);
  plan.slot_of_proof.resize(nproofs);
  for (size_t i = 0; i < nproofs; ++i) {                // stable: a key's proofs take its slots in input order
    const uint64_t s = next[key_of_proof[i]]++;
    plan.proof_of_slot[(size_t)s] = (uint32_t)i;
    plan.slot_of_proof[i] = (uint32_t)s;
  }
  return kVpOk;
}

}  // namespace gs
