// Host-compiled walk over the accumulation launches' workgroup-size policy (go-snark-study_amd/csrc/acc_shape.h) and the two
// switches that go before it (knobs.h).  Driven from tests/test_acc_shape_host.py.
// Every combination of: curve x terms (around 2^19 and the extremes) x route x caller x pipelined x no_poly x njobs x multi-device.
// The policy must answer 64, 128 or 256 everywhere and 256 wherever a launch is below 2^19 terms, blocking, a plain MSM, part of a
// proof with a polynomial stage, or made by a multi-device entry point.  Prints "OK <cases> cases, <n> not 256" or the first failures.
#include <cstdio>
#include <cstdlib>
#include "../../go-snark-study_amd/csrc/acc_shape.h"
#include "../../go-snark-study_amd/csrc/knobs.h"

using namespace gs;

int main() {
  const uint32_t terms[] = {0u, 1u, 4096u, (1u << 16), (1u << 18), (1u << 19) - 1, (1u << 19), (1u << 19) + 1, (1u << 20), (1u << 20) + 1,
                            (1u << 22), (1u << 26) - 1, 0xffffffffu};
  const int jobs[] = {0, 1, 2, 3, 6, 8};
  long cases = 0, other = 0, bad = 0;
  for (int g2 = 0; g2 < 2; ++g2)
    for (uint32_t n : terms)
      for (int tf = 0; tf < 2; ++tf)
        for (int caller = 0; caller < 2; ++caller)
          for (int pipelined = 0; pipelined < 2; ++pipelined)
            for (int no_poly = 0; no_poly < 2; ++no_poly)
              for (int nj : jobs)
                for (int multi = 0; multi < 2; ++multi) {
                  const AccLaunch a{g2 != 0, n, tf != 0, caller ? AccCaller::Proof : AccCaller::Msm, pipelined != 0, no_poly != 0, nj, multi != 0};
                  const int g = acc_group_policy(a);
                  ++cases;
                  const bool must_256 = n < (1u << 19) || !pipelined || caller == 0 || !no_poly || multi;
                  bool ok = acc_group_valid(g) && !(must_256 && g != 256);
                  // a set switch goes before the policy, whatever the launch; an unset one (0) or a value it cannot take leaves the policy
                  for (long f : {64L, 128L, 256L}) ok = ok && acc_group_size(a, f) == (int)f;
                  for (long f : {0L, 1L, 32L, 63L, 65L, 96L, 192L, 255L, 257L, 512L, -64L}) ok = ok && acc_group_size(a, f) == g;
                  if (g != 256) ++other;
                  if (!ok && ++bad <= 10)
                    std::printf("FAIL g2=%d n=%u table_free=%d caller=%d pipelined=%d no_poly=%d njobs=%d multi=%d -> %d\n", g2, n, tf, caller, pipelined,
                                no_poly, nj, multi, g);
                }
  // the switches themselves: strictly parsed, 64 / 128 / 256 only
  struct { const char* text; long want; } env[] = {{"64", 64}, {"128", 128}, {"256", 256}, {"0", 0}, {"32", 0}, {"96", 0}, {"100", 0}, {"192", 0},
                                                   {"512", 0}, {"-64", 0}, {"64x", 0}, {"", 0}, {"1e2", 0}, {"0x40", 0}};
  for (const auto& e : env) {
    setenv("GS_ACC_GROUP_TEST", e.text, 1);
    const long got = acc_group_env("GS_ACC_GROUP_TEST");
    if (got != e.want && ++bad <= 10) std::printf("FAIL switch '%s' -> %ld, expected %ld\n", e.text, got, e.want);
  }
  unsetenv("GS_ACC_GROUP_TEST");
  if (acc_group_env("GS_ACC_GROUP_TEST") != 0 && ++bad <= 10) std::printf("FAIL unset switch\n");
  if (bad) { std::printf("%ld failures\n", bad); return 1; }
  std::printf("OK %ld cases, %ld not 256\n", cases, other);
  return 0;
}
