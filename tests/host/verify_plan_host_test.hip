// Host check of the slot plan of gs_groth16_verify_each_keys (verify_plan.h), compiled for the CPU, against a plan made the slow way:
//   every proof occupies exactly one slot, and slot_of_proof / proof_of_slot are inverse to each other;
//   every group holds one key: each of its valid lanes holds a proof of that key, the lanes behind them hold none;
//   the group count is the sum over the keys of ceil(c_k / 64), the groups lie in key order and only the last group of a key is partial;
//   the order inside a key is the input order;
//   the signal offsets are the running sums of npublic over the occupied slots in front, nsignals is the total.
// Cases: random key_of_proof over random npublic; all proofs on one key; one proof per key; counts 63, 64 and 65 (and 1, 127, 128, 129,
// 200) on every key position; a key with none in front, between and behind; no proofs; no keys; an index past the end is refused and
// the offender is named.  The same program runs under -fsanitize=address,undefined when hostbuild is asked to (GS_HOST_SANITIZE).
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../go-snark-study_amd/csrc/verify_plan.h"
using namespace gs;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint32_t rnd(uint32_t below) {
  rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17;
  return (uint32_t)((rng_state >> 11) % below);
}

static bool check(const std::vector<uint32_t>& kop, const std::vector<uint32_t>& npub, const char* what) {
  const size_t n = kop.size(), nkeys = npub.size();
  VerifyPlan plan;
  const VerifyPlanStatus st = plan_verify_slots(kop.data(), n, nkeys, npub.data(), plan);
  const auto fail = [&](const char* why, size_t at) { printf("FAIL %s: %s at %zu\n", what, why, at); return false; };
  if (st != kVpOk) return fail("refused", 0);
  // the slow way
  std::vector<std::vector<uint32_t>> of_key(nkeys);
  for (size_t i = 0; i < n; ++i) of_key[kop[i]].push_back((uint32_t)i);
  size_t want_groups = 0;
  for (size_t k = 0; k < nkeys; ++k) want_groups += (of_key[k].size() + 63) / 64;
  if (plan.groups.size() != want_groups) return fail("group count", plan.groups.size());
  if (plan.proof_of_slot.size() != want_groups * 64) return fail("slot count", plan.proof_of_slot.size());
  if (plan.slot_of_proof.size() != n) return fail("slot_of_proof size", plan.slot_of_proof.size());
  size_t g = 0;
  uint64_t signals = 0;
  for (size_t k = 0; k < nkeys; ++k) {
    for (size_t done = 0; done < of_key[k].size(); done += 64, ++g) {
      const size_t left = of_key[k].size() - done, valid = left < 64 ? left : 64;
      if (plan.groups[g].key != k) return fail("key of group", g);
      if (plan.groups[g].valid != valid) return fail("valid lanes", g);
      if (plan.groups[g].sig_off != signals) return fail("signal offset", g);
      for (size_t l = 0; l < 64; ++l) {
        const uint32_t got = plan.proof_of_slot[g * 64 + l];
        if (l < valid) {
          if (got != of_key[k][done + l]) return fail("order inside a key", g * 64 + l);
          if (kop[got] != k) return fail("a group holds one key", g * 64 + l);
          if (plan.slot_of_proof[got] != g * 64 + l) return fail("slot_of_proof", got);
        } else if (got != kVpNoProof) return fail("padded slot", g * 64 + l);
      }
      signals += (uint64_t)valid * npub[k];
    }
  }
  if (g != want_groups) return fail("groups walked", g);
  if (plan.nsignals != signals) return fail("nsignals", 0);
  std::vector<int> seen(n, 0);
  for (uint32_t p : plan.proof_of_slot)
    if (p != kVpNoProof) { if (p >= n) return fail("proof index", p); seen[p] += 1; }
  for (size_t i = 0; i < n; ++i)
    if (seen[i] != 1) return fail("every proof occupies exactly one slot", i);
  return true;
}

int main() {
  long cases = 0;
  // random
  for (int it = 0; it < 200; ++it) {
    const size_t nkeys = 1 + rnd(9), n = rnd(400);
    std::vector<uint32_t> npub(nkeys), kop(n);
    for (auto& v : npub) v = rnd(5);
    for (auto& v : kop) v = rnd((uint32_t)nkeys);
    if (!check(kop, npub, "random")) return 1;
    ++cases;
  }
  // all proofs on one key, at every position among 3 keys
  for (uint32_t k = 0; k < 3; ++k)
    for (size_t n : {1, 63, 64, 65, 127, 128, 129, 200}) {
      if (!check(std::vector<uint32_t>(n, k), {1, 3, 2}, "one key")) return 1;
      ++cases;
    }
  // one proof per key, in order, reversed and shuffled
  for (size_t nkeys : {1, 2, 64, 65, 256}) {
    std::vector<uint32_t> npub(nkeys), kop(nkeys);
    for (size_t k = 0; k < nkeys; ++k) { npub[k] = (uint32_t)(k % 4); kop[k] = (uint32_t)k; }
    if (!check(kop, npub, "one proof per key")) return 1;
    for (size_t k = 0; k < nkeys; ++k) kop[k] = (uint32_t)(nkeys - 1 - k);
    if (!check(kop, npub, "one proof per key, reversed")) return 1;
    for (size_t k = nkeys; k > 1; --k) std::swap(kop[k - 1], kop[rnd((uint32_t)k)]);
    if (!check(kop, npub, "one proof per key, shuffled")) return 1;
    cases += 3;
  }
  // counts 63, 64, 65 side by side with a key that has none in front, between and behind; interleaved by a fixed stride
  for (int empty_at = 0; empty_at < 4; ++empty_at) {
    const size_t counts[3] = {63, 64, 65};
    std::vector<uint32_t> kop, npub(4, 2);
    npub[empty_at] = 7;
    for (int j = 0, k = 0; k < 4; ++k) {
      if (k == empty_at) continue;
      kop.insert(kop.end(), counts[j++], (uint32_t)k);
    }
    if (!check(kop, npub, "63 64 65 sorted")) return 1;
    std::vector<uint32_t> mixed(kop.size());
    for (size_t i = 0; i < kop.size(); ++i) mixed[i] = kop[(i * 7) % kop.size()];       // 7 and 192 are coprime
    if (!check(mixed, npub, "63 64 65 interleaved")) return 1;
    cases += 2;
  }
  // nothing to do
  if (!check({}, {1, 2}, "no proofs") || !check({}, {}, "no proofs, no keys")) return 1;
  cases += 2;
  // refusals
  {
    VerifyPlan plan;
    const uint32_t kop[4] = {0, 1, 2, 1}, npub[2] = {1, 1};
    size_t bad = 99;
    if (plan_verify_slots(kop, 4, 2, npub, plan, &bad) != kVpBadKey || bad != 2) { printf("FAIL: an index past the end\n"); return 1; }
    if (plan_verify_slots(kop, 1, 0, npub, plan, &bad) != kVpBadKey || bad != 0) { printf("FAIL: a proof but no keys\n"); return 1; }
    if (plan_verify_slots(kop, (size_t)kVpNoProof, 2, npub, plan) != kVpTooLarge) { printf("FAIL: 2^32 - 1 proofs\n"); return 1; }
    cases += 3;
  }
  printf("OK %ld cases, %u lanes\n", cases, kVpLanes);
  return 0;
}
