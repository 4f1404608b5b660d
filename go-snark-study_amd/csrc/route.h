// Internal: which way a proof's h-sum goes -- the most consequential decision of the prover engine (prove.hip, proof_enqueue), written
// down once.  It picks the key array whose table the call prepares, refuses a coset-only key, and fixes the lengths of the h-sum.
// Plain host C++, nothing of HIP: tests/host/route_host_test.hip runs it alone.
#pragma once
#include <algorithm>
#include <cstddef>

namespace gs {

// Shard of the term ranges a call sums over (multi-GPU: rank k of N takes [k/N, (k+1)/N) of both ranges).
struct Shard { size_t index = 0, count = 1; };
inline void shard_range(size_t n, const Shard& sh, size_t& lo, size_t& hi) {
  const size_t q = n / sh.count, rem = n % sh.count;
  lo = sh.index * q + std::min(sh.index, rem);
  hi = lo + q + (sh.index < rem ? 1 : 0);
}
inline size_t quotient_len(size_t npx, size_t nz) { return npx >= nz ? npx - nz + 1 : 0; }

// What the h-sum runs over, by who hands it to the engine (prove.hip, HSource: the alternatives in this order).
enum class HSourceKind { PxResident, PxOnHost, PxFromR1cs, Witness, Values };
// The route names the key array it sums against:
//   Values  H's values                        against h_eval   (evaluation basis)
//   Quot    px's coefficients from deg Z up   against h_quot   (quotient basis: nothing is divided by Z)
//   Hx      hx = floor(px / Z)                against h
enum class HRoute { Values, Quot, Hx };
enum class RouteError { None, CosetOnly, HxTooLong, ShardMismatch };

struct KeyFacts {                 // what the decision reads of a ProverKey (prove.h)
  size_t nz, len_h;
  size_t shard_index, shard_count, h_lo, n_h;
  size_t n_eval, e_lo, n_e;
  size_t n_q;
  bool coset_only, serves_quot;
};
struct HQuery {                   // ... and of the source
  HSourceKind kind;
  size_t npx;                     // len(px) that the source holds or would produce (unused by a values source)
  bool eval_open;                 // witness: the key's evaluation-basis array is the basis of this R1CS, and the route is not closed
  bool nodes_r1cs;                // witness: an R1CS over the nodes 1..n (it may compute hx directly), not over a power-of-two domain
};
struct RoutePlan {
  RouteError err = RouteError::None;
  HRoute route = HRoute::Hx;
  size_t nh = 0;                  // length of the whole h-sum: n_eval, or len(hx)
  size_t hlo = 0, hhi = 0;        // the terms of it this call sums
  size_t hbase = 0;               // where term hlo sits in the array the key holds
};

inline RoutePlan decide_route(const KeyFacts& k, const HQuery& q, const Shard& shard) {
  RoutePlan r;
  const bool eval = q.kind == HSourceKind::Values || (q.kind == HSourceKind::Witness && q.eval_open);
  if (!eval && k.coset_only) { r.err = RouteError::CosetOnly; return r; }      // every px route ends up here
  r.nh = eval ? k.n_eval : quotient_len(q.npx, k.nz);
  if (!eval && r.nh > k.len_h) { r.err = RouteError::HxTooLong; return r; }
  const bool sliced = k.shard_count > 1;
  // (a nodes-R1CS witness may compute H itself and keeps its route, and with it the division when that attempt does not apply)
  const bool quot = !eval && !(q.kind == HSourceKind::Witness && q.nodes_r1cs) && !sliced && r.nh >= 1 && k.serves_quot && r.nh <= k.n_q;
  r.route = eval ? HRoute::Values : quot ? HRoute::Quot : HRoute::Hx;
  if (sliced && (shard.index != k.shard_index || shard.count != k.shard_count)) { r.err = RouteError::ShardMismatch; return r; }
  if (sliced && eval) { r.hlo = k.e_lo; r.hhi = k.e_lo + k.n_e; }
  else if (sliced) {                // a slice's range of the h array was fixed at key creation (split of len_h, clipped to len(hx))
    r.hlo = std::min(k.h_lo, r.nh);
    r.hhi = std::min(k.h_lo + k.n_h, r.nh);
  } else shard_range(r.nh, shard, r.hlo, r.hhi);
  r.hbase = r.hlo - std::min(eval ? k.e_lo : k.h_lo, r.hlo);
  return r;
}

}  // namespace gs
