// Host-compiled view of the prover's route decision (go-snark-study_amd/csrc/route.h): which of a key's h arrays a proof's h-sum runs
// against, and its lengths.  Driven from tests/test_route_host.py, which checks every line against a table written out from the rules.
// Protocol: one request per line on stdin, 18 unsigned numbers:
//   kind npx eval_open nodes_r1cs   nz len_h shard_index shard_count h_lo n_h n_eval e_lo n_e n_q coset_only serves_quot   call_index call_count
// (kind: 0 px resident, 1 px on the host, 2 px from the R1CS, 3 witness, 4 values slice; call_*: the shard the call asks for)
//   ->   ok <values|quot|hx> nh hlo hhi hbase     or     err <coset_only|hx_too_long|shard_mismatch>
#include <iostream>
#include "../../go-snark-study_amd/csrc/route.h"

using namespace gs;

int main() {
  size_t v[18];
  for (;;) {
    for (size_t& x : v) if (!(std::cin >> x)) return 0;
    if (v[0] > 4 || v[17] == 0 || v[7] == 0) { std::cout << "bad\n"; continue; }
    const HQuery q{(HSourceKind)v[0], v[1], v[2] != 0, v[3] != 0};
    const KeyFacts k{v[4], v[5], v[6], v[7], v[8], v[9], v[10], v[11], v[12], v[13], v[14] != 0, v[15] != 0};
    Shard sh; sh.index = v[16]; sh.count = v[17];
    const RoutePlan r = decide_route(k, q, sh);
    switch (r.err) {
      case RouteError::CosetOnly: std::cout << "err coset_only\n"; continue;
      case RouteError::HxTooLong: std::cout << "err hx_too_long\n"; continue;
      case RouteError::ShardMismatch: std::cout << "err shard_mismatch\n"; continue;
      case RouteError::None: break;
    }
    std::cout << "ok " << (r.route == HRoute::Values ? "values" : r.route == HRoute::Quot ? "quot" : "hx") << " " << r.nh << " " << r.hlo << " "
              << r.hhi << " " << r.hbase << "\n";
  }
}
