// Internal: the workgroup size of one k_bucket_accumulate launch -- 64, 128 or 256 threads -- decided on the host per launch.
//
// The kernel uses no LDS and no barrier (one thread per chunk), so its workgroup is only the unit the dispatcher places: a
// 256-thread group needs a free wave slot on all four SIMDs of a CU at the same moment, a one-wave group refills any slot the moment
// it frees.  Alone, the kernels run 10-12 % faster in one-wave groups -- and the slots a 256-thread group leaves empty while it waits
// are where the plans, the polynomial passes and the tails of the side streams get their registers.  Whether a launch may close those
// slots therefore depends on what runs BESIDE it, which the caller knows and the kernel does not: a proof with a polynomial chain
// between plan(w) and plan(h) stalls its own h-accumulation when that chain starves (profiles/r06_ab_accumulate_block.txt); a
// pipelined proof without one has only two 0.3 ms plans and its tails beside it -- and still pays for one-wave groups with a wait
// for the next proof's plan(w) (profiles/acc_group_ab.txt), so today the policy answers 256 for every launch and the sizes below it
// are reached through the switches only.
// Pure host code, no HIP: prove.hip / capi_msm.hip ask, msm.hip launches, tests/host/acc_shape_host_test.hip walks every input.
#pragma once
#include <stdint.h>

namespace gs {

constexpr int kAccGroupDefault = 256;      // the size __launch_bounds__ is written for: the largest a launch may ask for
constexpr bool acc_group_valid(long g) { return g == 64 || g == 128 || g == 256; }

enum class AccCaller { Msm, Proof };       // a plain MSM (gs_msm_*, the key checks) or one of a proof's three accumulations

struct AccLaunch {
  bool g2 = false;                         // curve: G1 (3 waves per SIMD) or G2 (2)
  uint32_t nterms = 0;                     // terms of the plan the launch runs on
  bool table_free = false;                 // the plan's route: window tables, or a bucket set per window
  AccCaller caller = AccCaller::Msm;
  bool pipelined = false;                  // enqueued by a ticket (gs_*_begin): other operations' side work runs beside it
  bool no_poly = false;                    // the proof has no polynomial stage between its plans (h-scalars straight from px: the quotient-basis route)
  int njobs = 1;                           // base arrays summed by the launch (grid.y)
  bool multi_device = false;               // made by a multi-device entry point, or summing one shard of several
};

// Launches below this many terms keep 256: at 2^16-2^18 the accumulations are shorter than the tails beside them
// (profiles/r06_ab_accumulate_block.txt: +4.5 % at 2^16 and 2^18 in one-wave groups).
constexpr uint32_t kAccGroupMinTerms = 1u << 19;
// What a pipelined proof without a polynomial stage takes from kAccGroupMinTerms terms on, per curve.  Measured at 2^20 constraints,
// three proofs in flight, every pair of {64, 128, 256} that matters against the parent build (profiles/acc_group_ab.txt): the kernels
// gain what round 6 saw (the h-accumulation 1.54 -> 1.29 ms, `acc_g1_ms` 4.9 -> 4.5), and the main stream gives it back waiting for
// the next proof's plan(w), whose k_digits / k_scatter then run only while an accumulation launch drains (the gap in front of the G2
// launch grows from 54 to 570 us).  No setting came closer to the parent than the parent's own spread, so both stay at 256.
constexpr int kAccGroupProofG1 = 256;
constexpr int kAccGroupProofG2 = 256;

// Always 256 for: launches below 2^19 terms, blocking calls, plain MSMs, proofs with a polynomial stage, multi-device entry points
// -- each of them measured slower in one-wave groups -- and for the table-free route, which nobody measured in anything else.
constexpr int acc_group_policy(const AccLaunch& a) {
  if (a.caller != AccCaller::Proof || !a.pipelined || !a.no_poly || a.multi_device) return kAccGroupDefault;
  if (a.nterms < kAccGroupMinTerms || a.table_free || a.njobs < 1) return kAccGroupDefault;
  return a.g2 ? kAccGroupProofG2 : kAccGroupProofG1;
}

// The size a launch runs with: a set GS_ACC_GROUP_G1 / GS_ACC_GROUP_G2 (knobs.h; `forced` = its value, 0 = unset) goes before the policy.
constexpr int acc_group_size(const AccLaunch& a, long forced) { return acc_group_valid(forced) ? (int)forced : acc_group_policy(a); }

}  // namespace gs
