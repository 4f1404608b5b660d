// The prover engine: one proof of either scheme -- Groth16 (groth16.GenerateProofs, groth16/groth16.go:225-278) or Pinocchio
// (snark.GenerateProofs, snark.go:254-289) -- on top of the MSM and polynomial engines, read off the key's description
// (prove.h, ProverKey); the Groth16 tail; and the extern "C" fronts of both schemes, each a few lines over the engine.
#include "prove.h"

#include <algorithm>
#include <cstring>
#include <functional>
#include <chrono>
#include <future>
#include <variant>
#include <vector>

#include "hostcopy.h"
#include "point_io.h"

using namespace gs;

// upload host scalars into a scratch buffer
const uint32_t* gs::upload_tmp(Ctx& c, DevBuf& buf, const uint64_t* host, size_t n) {
  buf.ensure(std::max<size_t>(n, 1) * 32);
  if (n) {
    PhaseTimer th(c.stream);
    staged_h2d(c, buf.p, host, n * 32, c.stream);
    th.stop();
    c.timing.h2d_ms += th.ms();
  }
  return buf.as<uint32_t>();
}
void gs::download(Ctx& c, uint64_t* host, const void* dev, size_t n) {
  if (n) GS_HIP(hipMemcpyAsync(host, dev, n * 32, hipMemcpyDeviceToHost, c.stream));
  GS_HIP(hipStreamSynchronize(c.stream));
}

namespace {

struct DevVec { const uint32_t* p; size_t n; };   // the witness of a prove call (device, not owned): landed, or ordered on the stream that reads it
DevVec resident(const Scalars* s) { return DevVec{s->buf.as<uint32_t>(), s->n}; }

// What the h-sum of a proof runs over, by who hands it to the engine -- plain data; route.h (HSourceKind, in this order) decides
// from it and from the key which of the key's h arrays the sum goes against.
struct PxResident { const uint32_t* px; size_t n; };     // px on the device: a resident vector, or a host-buffer ticket's after staging
struct PxOnHost {                                        // px still in host memory (the blocking gs_*_prove): copied into `stage` on the
  uint32_t* stage; const uint64_t* host; size_t n;       // polynomial stream, behind the enqueue of the accumulations over w (h2d_ms)
};
struct PxFromR1cs { R1csObj* r1cs; const uint32_t* w; uint32_t* px_out; };   // px = r1csqap.go:161-210 of w, into the caller's vector
// A witness (the witness routes below): H's values when the evaluation-basis route is open, else hx directly (nodes R1CS) or through
// px, which goes into the exact-px buffer of `slot` -- allocated only when that route is taken.  `check`: count the violated
// constraints on the evaluation-basis route, so that the proof can be redone on the exact route.
struct WitnessSource { R1csObj* r1cs; const uint32_t* w; int slot; bool check, eval_open; };
// H's values of this key slice's range [e_lo, e_lo + n_e), computed by another rank and scattered (gs_*_prove_partials_values)
struct ValuesSlice { const uint32_t* values; size_t n_e; };
using HSource = std::variant<PxResident, PxOnHost, PxFromR1cs, WitnessSource, ValuesSlice>;
HSourceKind kind_of(const HSource& s) { return (HSourceKind)s.index(); }
static_assert(std::is_same_v<std::variant_alternative_t<(size_t)HSourceKind::Witness, HSource>, WitnessSource> &&
              std::is_same_v<std::variant_alternative_t<(size_t)HSourceKind::Values, HSource>, ValuesSlice>, "HSource follows HSourceKind");
PxResident resident_px(const Scalars* s) { return PxResident{s->buf.as<uint32_t>(), s->n}; }
ValuesSlice values_slice(const Scalars* hv) { return ValuesSlice{hv->buf.as<uint32_t>(), hv->n}; }
// the exact-route retry: this witness source with the evaluation-basis route closed, as a blocking proof of `slot`
HSource exact_retry(const HSource& src, int slot) {
  const WitnessSource& wit = std::get<WitnessSource>(src);
  return WitnessSource{wit.r1cs, wit.w, slot, wit.check, false};
}

// internal status of proof_collect: the witness violates a constraint, so the optimistic evaluation-basis result is void --
// run the exact route (px, floor quotient) instead.  Never crosses the C ABI.
constexpr int kRetryExact = 1;

// Stream layout of one proof (all device work is enqueued before the host waits once):
//   main  : plan(w) -> accumulate G2 over w -> accumulate the G1 arrays over w -> [wait plan(h)] accumulate G1 over h -> its tail
//   aux 0 / aux 2 : the tails (bucket combine, reduction, download) of the G2 / G1 groups over w, each after its accumulation
//   aux 1 : H(x) = P(x)/Z(x) -> plan(h)
// The ALU-bound accumulation kernels run back to back on one stream (they would only fight for the
// instruction cache if overlapped), and everything latency- or bandwidth-bound runs in their shadow.

// The raw MSM results of a proof in key order (prove.h: g1w with the B array put back in place, g2w, h): a Pinocchio proof is
// these points, a Groth16 proof its O(1) tail over them.
struct ProofSums {
  std::vector<G1Xyzz> g1w;
  G2Xyzz g2w;
  G1Xyzz h;
};

// The streams ONE proof's device work is enqueued on, decided once per proof (round 4 toggled a context flag between two
// evaluations of an accessor instead).  plan(w) of a pipelined proof gets its own stream (aux 2, every tail then shares aux 0) where
// the polynomial stage is long: on aux 1 the NEXT proof's plan(w) queues behind this proof's H stage and plan(h), and the
// accumulation stream then waits ~0.3 ms twice per proof.  Measured (profiles/r04_ab_plan_w_stream.txt): witness route at 2^20
// 10.2-10.3 -> 9.8 ms, at 2^19 5.55 -> 5.17, px route at 2^22 35.9 -> 35.4 ms, but the px route at 2^20 (H(x) is only 0.7 ms there)
// 8.7-8.9 -> 9.0-9.1: hence the rule.  GS_PLANW_STREAM: 0 never, 1 this rule, 2 always (identical results).
struct ProofStreams {
  hipStream_t planw = nullptr, poly = nullptr, tail_g2 = nullptr, tail_g1 = nullptr;
  bool poly_first = false;      // enqueue H(x) and plan(h) right behind plan(w), in front of the accumulations' tails (slot layout below)
};
// GS_SLOT_STREAMS (scheduling only, same results; round 6): 1 = a pipelined proof keeps ALL its side work -- plan(w), H(x), plan(h), then the
// three reduction tails -- on the aux stream of its ticket slot, so the side chains of the three proofs in flight run beside each
// other instead of queueing on one plan / polynomial stream.  For witnesses full of zeros and small values the accumulations of a 2^20
// proof are 2.5 ms but plan(w) + H(x) + plan(h) of consecutive proofs on ONE stream take 3.6 ms per proof beside them
// (profiles/r05_timeline_realistic_px_steady.txt: the accumulation stream idles 0.9 + 0.2 ms per proof waiting for a plan).  0 = the layouts above.
static ProofStreams proof_streams(Ctx& c, bool pipelined, size_t nterms, bool from_witness, int parity) {
  static const long mode = run_knob("GS_PLANW_STREAM", 1, 0, 2);
  static const long slot_mode = run_knob("GS_SLOT_STREAMS", 0, 0, 1);
  if (pipelined) c.next_tails((uint32_t)nterms);      // consecutive pipelined operations swap the two tail streams
  ProofStreams ps;
  if (pipelined && slot_mode == 1 && parity >= 0 && parity < Ctx::kAuxStreams && c.aux_stream[parity] != c.main_stream) {
    ps.planw = ps.poly = ps.tail_g2 = ps.tail_g1 = c.aux_stream[parity];
    ps.poly_first = true;
    return ps;
  }
  const bool own = pipelined && c.aux_stream[2] != c.aux_stream[1] &&
                   (mode == 2 || (mode == 1 && nterms >= ((size_t)1 << 19) && (from_witness || nterms >= ((size_t)1 << 21))));
  ps.poly = c.aux_stream[1];
  ps.planw = own ? c.aux_stream[2] : c.aux_stream[1];
  ps.tail_g2 = own ? c.aux_stream[0] : c.tail_stream(0);
  ps.tail_g1 = own ? c.aux_stream[0] : c.tail_stream(1);
  return ps;
}

// the part of a term list that falls into the held range [base, base + nterms): pointer into the device list and count
static const uint32_t* term_list_range(const DevBuf& index_dev, const std::vector<uint32_t>& index_host, size_t base, size_t nterms, uint32_t& count) {
  const auto lo = std::lower_bound(index_host.begin(), index_host.end(), (uint32_t)base);
  const auto hi = std::lower_bound(lo, index_host.end(), (uint32_t)(base + nterms));
  count = (uint32_t)(hi - lo);
  return index_dev.as<uint32_t>() + (lo - index_host.begin());
}

// One proof in flight.  Up to Ctx::kMaxInFlight may be outstanding (slots 0 / 1 / 2 own disjoint plan buffers, bucket workspaces and pinned result
// slots), so the plan and accumulations of proof k+1 are enqueued behind proof k's last accumulation and run while proof
// k's combine/reduce tails, its result download and its host-side tail are still in progress.
struct ProofInFlight : InFlightBase {
  ProverKey* pk = nullptr;
  ProofStreams streams;
  DevVec w{nullptr, 0};                    // what the proof was enqueued with (a ticket's exact-route retry starts from it)
  HSource src;
  std::shared_ptr<PhaseTimer> th2d;        // host-buffer tickets: the staging copies (read when the ticket is collected: a read at once would wait for them)
  // done_g2 / done_g1w / done_h: one per MSM group, recorded behind that group's reduction tail, so the host can add up a
  // group's partial sums while the later groups are still on the device
  hipEvent_t planw = nullptr, planh = nullptr, done_main = nullptr, done_g2 = nullptr, done_g1w = nullptr, done_h = nullptr;
  // keys with sparse B arrays (prove.h, b_index): the two B arrays run over a plan over the listed terms of their own; pend_g1w then
  // carries the other G1 arrays only and pend_g1b the sum over g1w[b_g1]
  bool split_b = false;
  hipEvent_t planb = nullptr, done_g1b = nullptr;
  MsmPending pend_g1b;
  std::shared_ptr<PhaseTimer> tplanb;
  std::unique_ptr<PhaseTimer> total;
  MsmPending pend_g1w, pend_g2w, pend_h;
  std::shared_ptr<PhaseTimer> tpoly, tplanw, tplanh;
  const uint32_t* bad_host = nullptr;      // evaluation-basis route: the violated-constraint count (valid once done_h has fired)
  // The scheme's hook into the fold of the G1 group over w (runs on that group's worker thread, with the sums in key order, while
  // the group over h is still on the device): Groth16's early tail products.
  std::function<void(const std::vector<G1Xyzz>&)> on_g1w;
  ProofInFlight() {
    for (hipEvent_t* e : {&planw, &planh, &done_main, &done_g2, &done_g1w, &done_h, &planb, &done_g1b}) GS_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
  }
  void wait_device() const override {
    for (hipEvent_t e : {done_g2, done_g1w, done_h, done_main}) if (e) GS_HIP(hipEventSynchronize(e));
    if (split_b && done_g1b) GS_HIP(hipEventSynchronize(done_g1b));
  }
  ~ProofInFlight() override {
    for (hipEvent_t e : {planw, planh, done_main, done_g2, done_g1w, done_h, planb, done_g1b}) if (e) (void)hipEventDestroy(e);
  }
};

// Sparse B (prove.h, b_index): when fewer than 55 % of the key's variables have a B entry, the two B arrays are summed over a second plan of
// w without the others -- one more sort (~0.35 ms at 2^20) against that share of 3.8 of a Groth16 proof's 6.8 job-units.  Measured at 2^20
// (profiles/r05_ab_sparse_b_split.txt): a circuit of the reference compiler's shape (33 % of the variables in B, full-width witness)
// 8.3-8.4 -> 6.1-6.2 ms per proof in flight, 8.8 -> 6.9 blocking, witness route 9.15 -> 7.2; the realistic-witness instance (60 % in
// B, and the absent variables are the small ones that carry one or two digits anyway) LOSES 3 % -- hence 55, not 90.  Pinocchio
// (B in G2 and B'): 11.76 -> 9.1 ms per 2^20 proof in flight.  (Window widths of 18 and more -- only by gs_set_window_bits -- keep the single
// plan: their partition-first sort takes no term list.  ADVICE r5: the gate used to say `cw < 19` while build_plan partitions from
// c = 18 on, so a forced width of 18 on a sparse-B key failed every proof.)
static long split_b_percent() {
  static const long pct = run_knob("GS_SPLIT_B_PERCENT", 55, 0, 100);      // split below this share of finite B points; 0 = never (same results)
  return pct;
}

// ---- what a witness source computes, on the polynomial stream --------------------------------------------------------------------
// px of the exact route: one buffer per slot (the three tickets and the blocking entry points), allocated only if that route is
// ever taken.  Round 3 handed every in-flight ticket -- and the blocking entry points' host uploads -- the SAME staging buffer and
// leaned on all polynomial stages being serialised on one stream; a slot's buffer is only ever touched by the
// operation that owns the slot, and a slot is re-used only after its operation was collected.
uint32_t* exact_px_buffer(Ctx& c, R1csObj* o, int slot) {
  const size_t npx = o->npx();
  o->prod.ensure(npx * 32);
  DevBuf& b = prove_state(c).exact_px[slot % Ctx::kSlots];
  b.ensure(npx * 32);
  return b.as<uint32_t>();
}
// The three ways to the h-scalars of a witness proof, in the order the prover tries them (a domain R1CS has two: the coset
// evaluation-basis route, then px -- its quotient by x^m - 1 goes through the key's Divisor / quotient-basis array like any Z).
// 1. Evaluation-basis route: H's values (n_eval of them) into `hv`, the number of violated constraints into the device word `bad`
// (read when the proof is collected).  The check is off for a product system (c = a b by definition: nothing to check) and for a
// coset-only key (no exact route to go to): the count is 0, and a wrong witness gives a proof that the verifier rejects, as in snarkjs.
void witness_values(Ctx& c, const WitnessSource& s, size_t dz, uint32_t* hv, uint32_t* bad) {
  R1csObj* o = s.r1cs;
  r1cs_values_dev(c, *o, s.w);
  if (const int k = o->domain_log2) {
    if (s.check) r1cs_check_domain_dev(c, o->vals.as<uint32_t>(), k, bad);
    else GS_HIP(hipMemsetAsync(bad, 0, 4, c.stream));
    hx_values_domain_dev(c, o->vals.as<uint32_t>(), k, hv);
  } else {
    r1cs_check_dev(c, o->vals.as<uint32_t>(), o->n, dz, bad);
    hx_values_dev(c, o->vals.as<uint32_t>(), o->n, dz, hv);
  }
}
// 2. hx = px / Z directly from the constraint values (poly.h, hx_direct_dev: a nodes R1CS and a satisfying witness); false = not
// applicable, go through px
bool witness_hx(Ctx& c, const WitnessSource& s, size_t dz, uint32_t* hx) {
  R1csObj* o = s.r1cs;
  if (o->domain_log2) return false;
  r1cs_values_dev(c, *o, s.w);
  return hx_direct_dev(c, o->vals.as<uint32_t>(), o->n, dz, hx);
}
// 3. px itself (r1csqap.go:161-210 on the sparse system) -- also what a PxFromR1cs source does; the engine then divides by Z, or not

// Enqueue every device operation of one proof (no host wait).  `wait_inputs`: w / px were uploaded on the main stream
// in this call, so the aux streams must order themselves behind that point.  Ticket `parity` owns plan slots 2p / 2p + 1, workspace
// sets 8p .. 8p + 7 and pinned slots 3p .. 3p + 2.  `shard`: the term ranges this call sums over (several GPUs: rank k of N; the
// sums of the ranks add up to the proof's).
int proof_enqueue(Ctx& c, ProverKey* pk, DevVec w, const HSource& src, const Shard& shard, int parity, bool wait_inputs, bool pipelined,
                  ProofInFlight& st) {
  DevBuf& hxbuf = prove_state(c).hx[parity];
  if (w.n != pk->nvars) return fail(GS_ERR_SHAPE, "len(w) = %zu but the key has %zu variables", w.n, pk->nvars);
  const WitnessSource* wit = std::get_if<WitnessSource>(&src);
  const PxFromR1cs* from_r1cs = std::get_if<PxFromR1cs>(&src);
  const ValuesSlice* values = std::get_if<ValuesSlice>(&src);
  R1csObj* r1cs = wit ? wit->r1cs : from_r1cs ? from_r1cs->r1cs : nullptr;      // the source computes on the polynomial stream, from
  const uint32_t* r1cs_w = wit ? wit->w : from_r1cs ? from_r1cs->w : nullptr;   // this system and this witness
  // px's coefficients where the source has them or puts them, and how many it holds or would produce
  const uint32_t* px = from_r1cs ? from_r1cs->px_out : nullptr;
  size_t npx = r1cs ? r1cs->npx() : 0;
  if (const auto* p = std::get_if<PxResident>(&src)) { px = p->px; npx = p->n; }
  else if (const auto* p = std::get_if<PxOnHost>(&src)) { px = p->stage; npx = p->n; }
  // The route (route.h): which of the key's h arrays the sum runs against -- hence which table this call prepares -- and its lengths
  const RoutePlan rp = decide_route(key_facts(*pk), HQuery{kind_of(src), npx, wit && wit->eval_open, wit && !wit->r1cs->domain_log2}, shard);
  if (rp.err == RouteError::CosetOnly) return refuse_coset_only(pk->kind == Kind::GrothPk ? "gs_groth16_prove" : "gs_pinocchio_prove");
  if (rp.err == RouteError::HxTooLong) return fail(GS_ERR_SHAPE, pk->hx_too_long, rp.nh, pk->len_h);
  if (rp.err == RouteError::ShardMismatch)
    return fail(GS_ERR_ARG, "this key holds shard %zu of %zu of the term ranges only: call gs_%s_prove_partials with that shard "
                "(asked for %zu of %zu)", pk->shard_index, pk->shard_count, pk->scheme, shard.index, shard.count);
  const HRoute route = rp.route; const size_t nh = rp.nh, hlo = rp.hlo, hhi = rp.hhi, hbase = rp.hbase;
  size_t wlo, whi;
  shard_range(w.n, shard, wlo, whi);
  const size_t wbase = wlo - pk->w_lo;      // offset into the arrays over w this key holds
  if (wit && route != HRoute::Values) px = exact_px_buffer(c, wit->r1cs, wit->slot);      // (only here does that buffer come into being)
  // window tables or table-free, per plan (tables.h, prepare_tables: the arrays over w share one plan, so they go one way together)
  // (before any table instalment goes onto the main stream: the plans on the aux streams wait for the inputs, not for the slabs)
  if (wait_inputs) {
    hipEvent_t start;
    GS_HIP(hipEventCreateWithFlags(&start, hipEventDisableTiming));
    GS_HIP(hipEventRecord(start, c.main_stream));
    for (auto a : c.aux_stream) GS_HIP(hipStreamWaitEvent(a, start, 0));
    GS_HIP(hipEventDestroy(start));
  }
  int cw = 0, ch = 0;
  const int ng = pk->n_g1w, bg = pk->b_g1;
  KeyArray& harr = route == HRoute::Values ? pk->h_eval : route == HRoute::Quot ? pk->h_quot : pk->h;
  const size_t n_harr = route == HRoute::Values ? pk->n_e : route == HRoute::Quot ? pk->n_q : pk->n_h;
  // every table of the call is stamped before one is built (an allocation for the first group must not evict the second group's), and
  // under policy `auto` the call grants itself a build credit for its job-units over w and h (a G1 sum = 1, the G2 sum = 2.76: ~6.8
  // for a Groth16 proof; tables.h, prepare_tables)
  std::vector<BaseTable*> stamps;
  std::vector<TableRef> refs_w;
  for (int i = 0; i < ng; ++i) {
    stamps.push_back(&pk->g1w[i].table);
    refs_w.push_back(TableRef{&pk->g1w[i].table, pk->g1w[i].pts.as<uint32_t>(), pk->n_w, false});
  }
  stamps.push_back(&pk->g2w.table); stamps.push_back(&harr.table);
  refs_w.push_back(TableRef{&pk->g2w.table, pk->g2w.pts.as<uint32_t>(), pk->n_w, true});
  stamp_tables(c, stamps);
  double credit = build_credit((double)ng + 2.76 + 1.0, whi - wlo);
  const bool tab_w = prepare_tables(c, refs_w, (uint32_t)(whi - wlo), &cw, &credit);
  const bool tab_h = prepare_tables(c, {TableRef{&harr.table, harr.pts.as<uint32_t>(), n_harr, false}}, (uint32_t)(hhi - hlo), &ch, &credit);
  if (route != HRoute::Quot) hxbuf.ensure(std::max<size_t>(nh, 1) * 32);
  auto base_w = [&](KeyArray& a) { return MsmBase{&a.table, wbase, a.pts.as<uint32_t>(), pk->n_w}; };
  st.pk = pk;
  st.total = std::make_unique<PhaseTimer>(c.main_stream);
  const int ws = 8 * parity, pin = 3 * parity;
  MsmPlan plan_w, plan_h;
  // The main stream carries NOTHING but the ALU-bound bucket accumulations (G2, then the G1 arrays over w, then h),
  // so with two proofs in flight it never idles: both plans, H(x) and every combine/reduce tail run on the aux streams.
  const ProofStreams ps = proof_streams(c, pipelined, whi - wlo, r1cs != nullptr, parity);   // (not a values slice: no polynomial work here)
  st.streams = ps;
  const size_t nterms_w = whi - wlo;
  st.split_b = pk->b_index.p != nullptr && nterms_w >= 4096 && !plan_partitions_first(cw) && pk->b_finite * 100 < (size_t)split_b_percent() * pk->n_w;
  MsmPlan plan_b;
  const bool no_poly = route == HRoute::Quot && !r1cs;           // nothing between px and plan(h): no polynomial phase to time, or to starve
  // threads per workgroup of this proof's accumulation launches (acc_shape.h): one-wave groups only where nothing of the proof's own
  // side chain is long enough to stall the main stream when the accumulations take every wave slot
  const bool multi_device = shard.count > 1 || multi_device_call();
  auto acc_group = [&](bool g2, const MsmPlan& plan, int njobs) {
    return acc_group_policy(AccLaunch{g2, plan.n, plan.table_free, AccCaller::Proof, pipelined, no_poly, njobs, multi_device});
  };
  {                                                              // aux 1 (or aux 2, proof_streams): plan(w) [, the plan over the listed terms for B first: G2 starts the proof]
    StreamScope sc(c, ps.planw);
    if (st.split_b) {
      st.tplanb = std::make_shared<PhaseTimer>(c.stream);
      uint32_t nb = 0;                                             // the listed terms of this call's range only
      const uint32_t* list = term_list_range(pk->b_index, pk->b_index_host, wbase, nterms_w, nb);
      build_plan(c, 2 * Ctx::kSlots + parity, w.p + wlo * 8, nb, plan_b, {{1, true}, {1, false}}, cw, !tab_w, list, (uint32_t)wbase);
      st.tplanb->stop();
      GS_HIP(hipEventRecord(st.planb, c.stream));
    }
    st.tplanw = std::make_shared<PhaseTimer>(c.stream);
    build_plan(c, 0 + 2 * parity, w.p + wlo * 8, (uint32_t)nterms_w, plan_w,
               st.split_b ? std::vector<LaunchShape>{{ng - 1, false}} : std::vector<LaunchShape>{{1, true}, {ng, false}}, cw, !tab_w);
    st.tplanw->stop();
    GS_HIP(hipEventRecord(st.planw, c.stream));
  }
  // Host order: the accumulations over w are enqueued BEFORE the block that may copy px from pageable host memory -- that copy
  // stages through the runtime inside the call (~5 ms for 64 MiB), and the device must already have its 7 ms of work by then.
  // (Slot layout, ps.poly_first: everything of the proof's side chain first -- its tails follow on the same stream.)
  auto enqueue_acc_w = [&] {                                     // main: the accumulations over w, back to back
    StreamScope sc(c, c.main_stream);
    GS_HIP(hipStreamWaitEvent(c.stream, st.split_b ? st.planb : st.planw, 0));
    // The sums that run over i > NPublic only (Groth16's BACDelta, groth16.go:248-250; Pinocchio's A and A', snark.go:265-268) had
    // their first npublic+1 points forced to infinity at key creation, so they equal a full-range MSM sharing w's plan.
    // G2 first: its accumulation (2 waves/SIMD, 256 VGPRs) is the one a foreign wave hurts most, and its long
    // combine/reduce tail then hides behind the G1 accumulations.
    const MsmPlan& plan_g2 = st.split_b ? plan_b : plan_w;
    msm_enqueue_g2(c, plan_g2, {base_w(pk->g2w)}, ws + pk->ws_g2, pin + 1, st.pend_g2w, acc_group(true, plan_g2, 1), ps.tail_g2);
    GS_HIP(hipEventRecord(st.done_g2, ps.tail_g2));
    std::vector<MsmBase> group;                                  // the G1 arrays over plan(w): all of them, or all but the B array
    for (int i = 0; i < ng; ++i) if (!(st.split_b && i == bg)) group.push_back(base_w(pk->g1w[i]));
    if (st.split_b) {
      msm_enqueue_g1(c, plan_b, {base_w(pk->g1w[bg])}, ws + pk->ws_b, 3 * Ctx::kSlots + parity, st.pend_g1b, acc_group(false, plan_b, 1), ps.tail_g1);
      GS_HIP(hipEventRecord(st.done_g1b, ps.tail_g1));
      GS_HIP(hipStreamWaitEvent(c.stream, st.planw, 0));
    }
    msm_enqueue_g1(c, plan_w, group, ws + 0, pin + 0, st.pend_g1w, acc_group(false, plan_w, (int)group.size()), ps.tail_g1);
    GS_HIP(hipEventRecord(st.done_g1w, ps.tail_g1));
  };
  // (Starting H(x) and plan(h) of a lone proof beside plan(w) on another stream instead of behind it was tried: the blocking proof
  // got SLOWER, 11.5-11.7 vs 11.0-11.25 ms -- the NTT passes then overlap the G2 accumulation's first milliseconds more densely.)
  auto enqueue_poly = [&] {                                      // aux 1 again: (late upload of px,) H(x), plan(h)
    StreamScope sc(c, ps.poly);
    if (const auto* h = std::get_if<PxOnHost>(&src); h && h->n) {   // the device is already busy with ~8 ms of accumulations: this copy is off the critical path
      PhaseTimer th(c.stream);
      staged_h2d(c, h->stage, h->host, h->n * 32, c.stream);
      th.stop();
      c.timing.h2d_ms += th.ms();
    }
    if (!no_poly) st.tpoly = std::make_shared<PhaseTimer>(c.stream);
    uint32_t* hx = hxbuf.as<uint32_t>();
    const size_t dz = pk->nz - 1;
    switch (route) {
      case HRoute::Values:                                                       // (a slice of H's values came from another rank)
        if (wit) {
          witness_values(c, *wit, dz, hx, c.bad_dev.as<uint32_t>() + parity);
          GS_HIP(hipMemcpyAsync(c.bad_host + parity, c.bad_dev.as<uint32_t>() + parity, 4, hipMemcpyDeviceToHost, c.stream));
          st.bad_host = c.bad_host + parity;
        }
        break;
      case HRoute::Quot:
        if (r1cs) r1cs_px_dev(c, *r1cs, r1cs_w, const_cast<uint32_t*>(px));
        break;
      case HRoute::Hx:
        if (wit && nh && witness_hx(c, *wit, dz, hx)) break;                     // H from the constraint values (satisfying witness)
        if (r1cs) r1cs_px_dev(c, *r1cs, r1cs_w, const_cast<uint32_t*>(px));
        if (nh) poly_quotient_dev(c, pk->z, px, npx, hx);                        // groth16.go:266, snark.go:280
        break;
    }
    if (st.tpoly) st.tpoly->stop();
    st.tplanh = std::make_shared<PhaseTimer>(c.stream);
    // the scalars of the h-sum: H's values of this slice, px's coefficients from deg Z up (any 256-bit words: k_digits canonicalises), or hx
    const uint32_t* hscal = values ? values->values : route == HRoute::Quot ? px + (dz + hlo) * 8 : hx + hlo * 8;
    build_plan(c, 1 + 2 * parity, hscal, (uint32_t)(hhi - hlo), plan_h, {{1, false}}, ch, !tab_h);
    st.tplanh->stop();
    GS_HIP(hipEventRecord(st.planh, c.stream));
  };
  if (ps.poly_first) { enqueue_poly(); enqueue_acc_w(); } else { enqueue_acc_w(); enqueue_poly(); }
  {                                                              // main again: the accumulation over h
    StreamScope sc(c, c.main_stream);
    GS_HIP(hipStreamWaitEvent(c.stream, st.planh, 0));
    // a lone proof finishes soonest with the last tail right behind its accumulation; in a pipeline that tail must not sit
    // in front of the next proof's accumulations
    msm_enqueue_g1(c, plan_h, {MsmBase{&harr.table, hbase, harr.pts.as<uint32_t>(), n_harr}}, ws + pk->ws_h, pin + 2, st.pend_h,
                   acc_group(false, plan_h, 1), pipelined ? ps.tail_g1 : nullptr);                           // groth16.go:269-271, snark.go:284-286
    GS_HIP(hipEventRecord(st.done_h, pipelined ? ps.tail_g1 : c.main_stream));
  }
  st.total->stop();
  GS_HIP(hipEventRecord(st.done_main, c.main_stream));
  return GS_OK;
}

static double host_now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
static bool host_trace() { static const bool on = run_flag("GS_HOST_TRACE"); return on; }

// Wait for that proof's device work (only its own events: later proofs keep running) and add up the results.
int proof_collect(Ctx& c, ProofInFlight& st, ProofSums& sums) {
  const double t0 = host_trace() ? host_now_ms() : 0;
  double t1 = 0;
  std::vector<G1Xyzz> g1h;
  std::vector<G2Xyzz> g2w;
  {   // The host-side pair sums of the three groups, each as soon as its own tail is through: the groups over w finish milliseconds
      // before the one over h, so only h's handful of additions is left when the device goes idle.
    // (HIP calls stay on the calling thread: a fresh thread pays ~0.3 ms for its first hipSetDevice / event wait.)
    GS_HIP(hipEventSynchronize(st.done_g2));
    auto f2 = std::async(std::launch::async, [&] { msm_finish_g2(c, st.pend_g2w, g2w); });
    struct Join { std::future<void>& f; ~Join() { if (f.valid()) f.wait(); } } j2{f2};     // a throwing wait below must not outrun the threads
    GS_HIP(hipEventSynchronize(st.done_g1w));       // (the B group of a split proof was enqueued before this one on the same tail stream)
    auto f1 = std::async(std::launch::async, [&] {
      msm_finish_g1(c, st.pend_g1w, sums.g1w);
      if (st.split_b) {                              // the sum over the B array goes back to its place in the order of the single plan
        std::vector<G1Xyzz> g1b;
        msm_finish_g1(c, st.pend_g1b, g1b);
        sums.g1w.insert(sums.g1w.begin() + st.pk->b_g1, g1b[0]);
      }
      if (st.on_g1w) st.on_g1w(sums.g1w);
    });
    Join j1{f1};
    GS_HIP(hipEventSynchronize(st.done_h));
    t1 = host_trace() ? host_now_ms() : 0;
    msm_finish_g1(c, st.pend_h, g1h);
    f2.get(); f1.get();
  }
  GS_HIP(hipEventSynchronize(st.done_main));
  if (host_trace()) fprintf(stderr, "[gs host] collect: wait %.3f ms, fold %.3f ms\n", t1 - t0, host_now_ms() - t1);
  msm_book_timing(c, st.pend_g1w); msm_book_timing(c, st.pend_g2w); msm_book_timing(c, st.pend_h);
  if (st.split_b) { msm_book_timing(c, st.pend_g1b); c.timing.plan_ms += st.tplanb->ms(); }
  if (st.tpoly) c.timing.poly_ms += st.tpoly->ms();
  c.timing.plan_ms += st.tplanw->ms() + st.tplanh->ms();
  c.timing.total_ms += st.total->ms();
  if (st.th2d) c.timing.h2d_ms += st.th2d->ms();
  sums.g2w = g2w[0]; sums.h = g1h[0];
  // evaluation-basis route: H's values only determine H when A B - C vanishes at every root of Z
  if (st.bad_host && *st.bad_host != 0) return kRetryExact;
  return GS_OK;
}

// The blocking proof: enqueue, collect, and once more through px and the floor quotient when the evaluation-basis route met a
// violated constraint.  `on_g1w` (ProofInFlight) rides on the first pass only: the sums over w do not depend on the route.
int proof_sums_blocking(Ctx& c, ProverKey* pk, DevVec w, HSource src, const Shard& shard, ProofSums& sums,
                        std::function<void(const std::vector<G1Xyzz>&)> on_g1w = nullptr) {
  for (;;) {
    const double t0 = host_trace() ? host_now_ms() : 0;
    ProofInFlight st;
    st.on_g1w = std::move(on_g1w);
    on_g1w = nullptr;
    int rc = proof_enqueue(c, pk, w, src, shard, c.blocking_slot(), true, false, st);
    if (rc != GS_OK) return rc;
    const double t1 = host_trace() ? host_now_ms() : 0;
    rc = proof_collect(c, st, sums);
    if (host_trace()) fprintf(stderr, "[gs host] prove: enqueue %.3f ms, collect %.3f ms (entered at %.3f)\n", t1 - t0, host_now_ms() - t1, t0);
    if (rc != kRetryExact) return rc;
    src = exact_retry(src, c.blocking_slot());   // violated constraint: once more through px and the floor quotient
    c.timing.fallbacks += 1;
  }
}

// ---- the O(1) Groth16 tail on host cores (groth16.go:253-275) ---------------------------------------------
struct GrothTailPre {             // the tail products that need no MSM result (computed while the device runs)
  std::future<G2Xyzz> sdelta2;
  std::future<G1Xyzz> sdelta;
  G1Xyzz rdelta, rsdelta;
};
static void groth16_tail_pre(GrothPkObj* pk, const uint64_t r[4], const uint64_t s[4], GrothTailPre& pre) {
  // r delta, s delta, s delta2, (r s) delta: multiples of points that belong to the KEY -- fixed-base window tables (msm.h), built by
  // whichever proof of the key comes first; ~64 additions each instead of 256 doublings + 64 additions
  std::call_once(pk->fixed_once, [pk] { pk->delta_fixed.build(pk->delta); pk->delta2_fixed.build(pk->delta2); });
  uint64_t s_copy[4] = {s[0], s[1], s[2], s[3]};
  pre.sdelta2 = std::async(std::launch::async, [pk, s_copy] { return pk->delta2_fixed.mul(s_copy); });
  pre.sdelta = std::async(std::launch::deferred, [pk, s_copy] { return pk->delta_fixed.mul(s_copy); });   // ~60 us: no thread of its own
  pre.rdelta = pk->delta_fixed.mul(r);
  uint64_t rs[4];
  fr_mul_words(r, s, rs);
  pre.rsdelta = pk->delta_fixed.mul(rs);                       // (r s) delta = s (r delta)
}
// One proof's tail: r, s, the result-independent products (started on other host cores when the proof begins) and the two
// result-dependent products, s piA and r piB1 (groth16.go:272-273), which only need the sums over w -- which a proof has milliseconds
// before its sum over h: `early` is the engine's on_g1w hook and starts them (two host cores) as soon as the G1 group over w is
// folded, so that what is left when the device goes idle is a handful of additions and three normalisations.
struct GrothTail {
  GrothPkObj* pk = nullptr;
  uint64_t r[4] = {0, 0, 0, 0}, s[4] = {0, 0, 0, 0};
  GrothTailPre pre;
  std::future<void> fpre;
  bool early_done = false;
  G1Xyzz piA, piB1, sA, rB;
  void start(GrothPkObj* key, const uint64_t r_[4], const uint64_t s_[4]) {      // (the object must stay where it is from here on)
    pk = key;
    memcpy(r, r_, 32); memcpy(s, s_, 32);
    fpre = std::async(std::launch::async, [this] { groth16_tail_pre(pk, r, s, pre); });
  }
  void products(const std::vector<G1Xyzz>& g1w) {
    piA = g1w[GrothPkObj::kAt];
    xyzz_madd(piA, pk->alpha);                                 // + alpha          groth16.go:253
    xyzz_add(piA, pre.rdelta);                                 // + r delta        :254-255
    piB1 = g1w[GrothPkObj::kBacGamma1];
    xyzz_madd(piB1, pk->beta);                                 // + beta           :259
    xyzz_add(piB1, pre.sdelta.get());                          // + s delta        :261-262
    const G1Xyzz b1 = piB1;
    const uint64_t* rr = r;
    auto f_rB = std::async(std::launch::async, [b1, rr] { return g1_mul_scalar(b1, rr); });   // two host cores for the two
    sA = g1_mul_scalar(piA, s);                                // s piA            :272         result-dependent products
    rB = f_rB.get();                                           // r piB1           :273
  }
  void early(const std::vector<G1Xyzz>& g1w) {
    fpre.wait();                                               // r delta, s delta (the owner calls get() after this thread is joined)
    products(g1w);
    early_done = true;
  }
  void finish(const ProofSums& sums, uint64_t out_proof[32], int inf[3]) {
    if (fpre.valid()) fpre.get();
    if (!early_done) products(sums.g1w);                       // (else piA, piB1, s piA, r piB1 came from the fold thread: same sums)
    G2Xyzz piB = sums.g2w;
    xyzz_madd(piB, pk->beta2);                                 // + beta2          :260
    xyzz_add(piB, pre.sdelta2.get());                          // + s delta2       :263-264
    G1Xyzz piC = sums.g1w[GrothPkObj::kBacDelta];
    xyzz_add(piC, sums.h);                                     // + sum h_i PTD_i  :269-271
    xyzz_add(piC, sA);                                         // + s piA          :272
    xyzz_add(piC, rB);                                         // + r piB1         :273
    xyzz_add(piC, xyzz_neg(pre.rsdelta));                      // - (r s) delta    :274-275
    inf[0] = g1_to_affine_std(piA, out_proof) ? 1 : 0;
    inf[1] = g2_to_affine_std(piB, out_proof + 8) ? 1 : 0;
    inf[2] = g1_to_affine_std(piC, out_proof + 24) ? 1 : 0;
  }
  ~GrothTail() { if (fpre.valid()) fpre.wait(); }
};
struct GrothInFlight : ProofInFlight {      // what a Groth16 ticket carries beside the proof (the engine does not look at it)
  bool with_tail = false;                   // false: a partial-sums ticket (gs_groth16_partials_end)
  GrothTail tail;
};

int groth16_prove_impl(Ctx& c, GrothPkObj* pk, DevVec w, const HSource& src, const uint64_t r[4], const uint64_t s[4],
                       uint64_t out_proof[32], int inf[3]) {
  // the result-independent tail products run on other host cores while this thread enqueues and waits for the device
  GrothTail tail;
  tail.start(pk, r, s);
  ProofSums sums;
  const int rc = proof_sums_blocking(c, pk, w, src, Shard{}, sums, [&tail](const std::vector<G1Xyzz>& g1w) { tail.early(g1w); });
  if (rc != GS_OK) return rc;
  const double t2 = host_trace() ? host_now_ms() : 0;
  tail.finish(sums, out_proof, inf);
  if (host_trace()) fprintf(stderr, "[gs host] prove: tail %.3f ms\n", host_now_ms() - t2);
  return GS_OK;
}

// the five sums <-> the 48 words / 5 flags of gs_groth16_prove_partials:  At | BACGamma (G1) | BACGamma (G2) | BACDelta | h
void groth16_pack_sums(const ProofSums& sums, uint64_t out_sums[48], int inf[5]) {
  inf[0] = g1_to_affine_std(sums.g1w[GrothPkObj::kAt], out_sums) ? 1 : 0;
  inf[1] = g1_to_affine_std(sums.g1w[GrothPkObj::kBacGamma1], out_sums + 8) ? 1 : 0;
  inf[2] = g2_to_affine_std(sums.g2w, out_sums + 16) ? 1 : 0;
  inf[3] = g1_to_affine_std(sums.g1w[GrothPkObj::kBacDelta], out_sums + 32) ? 1 : 0;
  inf[4] = g1_to_affine_std(sums.h, out_sums + 40) ? 1 : 0;
}
void groth16_unpack_sums(const uint64_t sums_in[48], const int inf_in[5], ProofSums& sums) {
  auto g1 = [&](const uint64_t* p, int isinf) -> G1Xyzz {
    if (isinf) return xyzz_inf<FqTag>();
    const uint32_t* w32 = reinterpret_cast<const uint32_t*>(p);
    G1Affine a;
    a.x = canon(PointIO<FqTag>::load_std(w32)); a.y = canon(PointIO<FqTag>::load_std(w32 + 8));
    return xyzz_from_affine(a);
  };
  sums.g1w = {g1(sums_in, inf_in[0]), g1(sums_in + 8, inf_in[1]), g1(sums_in + 32, inf_in[3])};
  if (inf_in[2]) sums.g2w = xyzz_inf<Fq2Tag>();
  else {
    const uint32_t* w32 = reinterpret_cast<const uint32_t*>(sums_in + 16);
    G2Affine a;
    a.x = canon(PointIO<Fq2Tag>::load_std(w32)); a.y = canon(PointIO<Fq2Tag>::load_std(w32 + 16));
    sums.g2w = xyzz_from_affine(a);
  }
  sums.h = g1(sums_in + 40, inf_in[4]);
}
// a Pinocchio proof (or the partial sums of a rank) IS its eight sums:  PiA | PiAp | PiB | PiBp | PiC | PiCp | PiH | PiKp
void pinocchio_pack(const ProofSums& sums, uint64_t out[72], int inf[8]) {
  inf[0] = g1_to_affine_std(sums.g1w[PinocchioPkObj::kA], out) ? 1 : 0;
  inf[1] = g1_to_affine_std(sums.g1w[PinocchioPkObj::kAp], out + 8) ? 1 : 0;
  inf[2] = g2_to_affine_std(sums.g2w, out + 16) ? 1 : 0;
  inf[3] = g1_to_affine_std(sums.g1w[PinocchioPkObj::kBp], out + 32) ? 1 : 0;
  inf[4] = g1_to_affine_std(sums.g1w[PinocchioPkObj::kC], out + 40) ? 1 : 0;
  inf[5] = g1_to_affine_std(sums.g1w[PinocchioPkObj::kCp], out + 48) ? 1 : 0;
  inf[6] = g1_to_affine_std(sums.h, out + 56) ? 1 : 0;
  inf[7] = g1_to_affine_std(sums.g1w[PinocchioPkObj::kKp], out + 64) ? 1 : 0;
}
int pinocchio_prove_impl(Ctx& c, PinocchioPkObj* pk, DevVec w, const HSource& src, uint64_t out[72], int inf[8], const Shard& shard = Shard{}) {
  ProofSums sums;
  const int rc = proof_sums_blocking(c, pk, w, src, shard, sums);
  if (rc == GS_OK) pinocchio_pack(sums, out, inf);
  return rc;
}

// ---- host-buffer tickets -----------------------------------------------------------------------------------------------------
// The reference hands GenerateProofs a FRESH w (and px) in host memory on every call (groth16/groth16.go:225, cli/main.go:480-501).
// gs_scalars_upload + gs_*_begin + gs_free costs a hipMalloc, a blocking copy and a hipFree (a device-wide synchronisation) per proof
// and breaks a pipeline of three; a host-buffer ticket instead stages the caller's arrays into buffers its SLOT owns (grow-only:
// nothing is allocated or freed once the three slots have been used), on the copy stream -- the DMA of proof k + 3 runs beside the
// accumulations of proofs k + 1 and k + 2 -- and enqueues the proof when the copies have landed: the host waits for them once, after
// px when px follows w (one DMA tail instead of two), so what the engine sees are ordinary device vectors.  The host has nothing
// else to do then -- the device is busy with the two tickets before this one.  Measured at 2^20, three in flight, eight rotating
// witnesses (profiles/r05_ab_host_stage.txt) against a cross-stream event that the readers wait for, and against copying on the
// readers' own streams:  witness from the host 10.12-10.17 ms against 11.2-11.3 / 10.1-11.0,  w + px from the host 9.45-9.51 against
// 10.9 / 11.4-11.5 (resident: 10.03-10.07 / 8.84-9.01).  The caller's arrays are consumed when _begin returns (cgo pointer rule).
static const uint32_t* stage_on_copy_stream(Ctx& c, DevBuf& b, const uint64_t* host, size_t n) {
  b.ensure(std::max<size_t>(n, 1) * 32);
  if (n) staged_h2d(c, b.p, host, n * 32, c.copy_stream);
  return b.as<uint32_t>();
}
DevVec stage_slot_w(Ctx& c, int parity, const uint64_t* host, size_t n) { return DevVec{stage_on_copy_stream(c, prove_state(c).slot_w[parity], host, n), n}; }
PxResident slot_px_from_host(Ctx& c, int parity, const uint64_t* host, size_t n) {
  return PxResident{stage_on_copy_stream(c, prove_state(c).slot_px[parity], host, n), n};
}
// a resident vector that a ticket reads: gs_scalars_update must wait for these points (runtime.h, Scalars::reads)
void mark_ticket_reads(const ProofStreams& ps, Scalars* w, Scalars* px_or_hv) {
  if (w) { w->mark_read(ps.planw); if (ps.poly != ps.planw) w->mark_read(ps.poly); }
  if (px_or_hv) px_or_hv->mark_read(ps.poly);
}

// ---- witness routes ------------------------------------------------------------------------------------------------------------
// Witness -> proof without ever forming px (the fast form of CombinePolynomials + DivisorPolynomial, r1csqap.go:191-216, for a
// witness that satisfies the R1CS -- the only case in which a proof means anything):
//   * key with an evaluation-basis twin of its h array (the setups build one): the values of H at the nodes n+1..2n come
//     out of ONE batched convolution of the constraint values [A w | B w | C w], and the h-MSM runs over those values.  No
//     interpolation, no Taylor shift, no host wait: the violated-constraint count is read when the proof is collected.
//   * key without one: H's coefficients from the same values by one interpolation and a Taylor shift (poly.h, hx_direct_dev).
// When a constraint is violated the call takes the exact route of gs_groth16_prove_r1cs and returns the same (meaningless) proof
// the reference would.  Same result as the resident px of capi_r1cs.hip + gs_*_prove_resident either way.
bool hx_shape(size_t n, size_t nz) { return n >= 2 && nz >= 1 && (nz - 1 == n - 1 || nz - 1 == n); }

// A domain R1CS (domain.h) proves only with a full Groth16 key whose Z is x^m - 1 for the same m = 2^k and whose h array reaches
// H's m - 1 coefficients; a nodes-1..n R1CS proves with any key, as ever.
int check_domain_pair(const char* fn, const ProverKey* pk, const R1csObj* o) {
  if (!o->domain_log2) return GS_OK;
  const int k = o->domain_log2;
  if (pk->kind != Kind::GrothPk) return fail(GS_ERR_SHAPE, "%s: an R1CS over a power-of-two domain proves with Groth16 keys only", fn);
  if (pk->shard_count != 1) return fail(GS_ERR_SHAPE, "%s: an R1CS over a power-of-two domain proves with a full key, not with a key slice", fn);
  if (pk->domain_log2 != k)
    return fail(GS_ERR_SHAPE, "%s: the R1CS lives on the domain of 2^%d points, but the key's Z (%zu coefficients) is not x^(2^%d) - 1", fn, k, pk->nz, k);
  if (!pk->coset_only && pk->len_h + 1 < ((size_t)1 << k))      // (a coset-only key needs no h array: prove.h)
    return fail(GS_ERR_SHAPE, "%s: the key's h array has %zu points, H needs 2^%d - 1", fn, pk->len_h, k);
  return GS_OK;
}
// the evaluation-basis route is open when the key's array is the basis of this R1CS (and gs_set_eval_basis has not closed it)
bool eval_route(const Ctx& c, const ProverKey* pk, const R1csObj* o) {
  if (!c.eval_basis || pk->n_eval == 0) return false;
  if (o->domain_log2) return pk->eval_domain_log2 == o->domain_log2 && pk->n_eval == o->points();
  return pk->eval_domain_log2 == 0 && pk->n_eval == o->n && hx_shape(o->n, pk->nz);
}

// a coset-only key (prove.h) has one route: refuse the call when that route is not open (another kind of R1CS, gs_set_eval_basis(0))
int check_coset_only_route(const Ctx& c, const char* fn, const ProverKey* pk, const R1csObj* o) {
  return pk->coset_only && !eval_route(c, pk, o) ? refuse_coset_only(fn) : GS_OK;
}

WitnessSource witness_source(const ProverKey* pk, R1csObj* o, const uint32_t* wdev, int slot, bool eval_open) {   // of a proof in `slot`
  return WitnessSource{o, wdev, slot, !o->product && !pk->coset_only, eval_open};
}

// What a blocking witness entry point checks beyond its handles, as each did before they shared this preamble (the two schemes
// differ; DESIGN.md lists the divergences).
struct WitnessChecks {
  bool need_z;              // refuse a key with nz == 0
  bool eval_full_key_only;  // a key slice never takes the evaluation-basis route
};
// The preamble of the blocking witness entry points, after the handle / null checks: shapes, the witness onto the device (`w`
// resident, or `w_host` uploaded as part of the call), the route.
int witness_blocking_inputs(Ctx& c, const char* fn, ProverKey* pk, R1csObj* o, const Scalars* w, const uint64_t* w_host, size_t nw, const WitnessChecks& chk,
                            DevVec& dw, HSource& src) {
  if (nw != o->m) return fail(GS_ERR_SHAPE, "len(w) = %zu but the system has %zu variables", nw, o->m);
  if (chk.need_z && pk->nz == 0) return fail(GS_ERR_SHAPE, "the key has no Z");
  if (int rc = check_domain_pair(fn, pk, o)) return rc;
  if (int rc = check_coset_only_route(c, fn, pk, o)) return rc;
  reset_timing(c);
  const uint32_t* wdev = w ? w->buf.as<uint32_t>() : upload_tmp(c, prove_state(c).up_w, w_host, nw);
  const bool eval = !(chk.eval_full_key_only && pk->shard_count != 1) && eval_route(c, pk, o);
  dw = DevVec{wdev, nw};
  src = witness_source(pk, o, wdev, c.blocking_slot(), eval);
  return GS_OK;
}

// ---- tickets -------------------------------------------------------------------------------------------------------------------
// Pipelined proving: begin enqueues a whole proof and returns; end waits for THAT proof only and runs its tail.  With two
// proofs outstanding the device never idles between proofs (the next plan/accumulations are already queued) and the host
// tail of proof k overlaps the device work of proof k+1.  Both schemes share the three slots.
// One request for a proof ticket: {resident, host-buffer} x {w + px, witness}.
struct TicketRequest {
  const char* fn;                    // the entry point, for its error messages
  Kind kind;                         // of the key
  gs_handle hpk, hr1cs;              // hr1cs: the witness forms (px comes out of the R1CS), 0 otherwise
  bool witness;
  gs_handle hw, hpx;                 // resident form
  const uint64_t* w_host; size_t nw; // host-buffer form (gs_*_host_begin): w_host / px_host non-null, hw / hpx ignored
  const uint64_t* px_host; size_t npx;
  uint64_t* ticket;
  // the entry point's own argument checks, kept as each had them before the fronts shared this helper (DESIGN.md lists the divergences)
  bool null_extra;                   // another null argument of the front (Groth16: r, s); reported as "null argument" with a null ticket
  bool ticket_with_handles;          // a null ticket is reported together with a bad handle instead
  bool refuse_slice;                 // witness forms: refuse a key slice
  bool need_z;                       // witness forms: refuse a key with nz == 0
};
// Install a proof ticket once every check of its front has passed: the free slot (or GS_ERR_BUSY: "<fn>: three operations are already
// outstanding; <busy_hint>"), the in-flight object from `make()` holding `keep` alive, its inputs from `inputs(slot, st)` -- which
// sets st.w / st.src, staging a host-buffer ticket's arrays into the slot --, the enqueue, the read marks on the resident vectors,
// the ticket number.
template <class Make, class Inputs>
int install_ticket(Ctx& c, const char* fn, const char* busy_hint, ProverKey* pk, std::vector<std::shared_ptr<Object>> keep, const Shard& shard,
                   Scalars* w_resident, Scalars* h_resident, uint64_t* ticket, Make make, Inputs inputs) {
  const int parity = c.free_parity();
  if (parity < 0) return fail(GS_ERR_BUSY, "%s: three operations are already outstanding; %s", fn, busy_hint);
  std::unique_ptr<ProofInFlight> st = make();
  st->keep = std::move(keep);
  const double h0 = host_trace() ? host_now_ms() : 0;
  inputs(parity, *st);
  const double h1 = host_trace() ? host_now_ms() : 0;
  const int rc = proof_enqueue(c, pk, st->w, st->src, shard, parity, false, true, *st);
  if (rc != GS_OK) return rc;
  if (host_trace()) fprintf(stderr, "[gs host] begin: inputs %.3f ms, enqueue %.3f ms\n", h1 - h0, host_now_ms() - h1);
  if (st->th2d) st->th2d->stop();
  mark_ticket_reads(st->streams, w_resident, h_resident);
  st->ticket = c.new_ticket();
  *ticket = st->ticket;
  c.inflight[parity] = std::move(st);
  return GS_OK;
}
// `make` builds the in-flight object once every check has passed (Groth16 starts its tail there).
template <class Make>
int begin_ticket(Ctx& c, const TicketRequest& q, Make make) {
  const bool host = q.w_host != nullptr || q.px_host != nullptr;
  ProverKey* pk = c.get<ProverKey>(q.hpk, q.kind);
  R1csObj* o = q.witness ? c.get<R1csObj>(q.hr1cs, Kind::R1cs) : nullptr;
  Scalars* w = host ? nullptr : c.get<Scalars>(q.hw, Kind::Scalars);
  Scalars* px = host || q.witness ? nullptr : c.get<Scalars>(q.hpx, Kind::Scalars);
  const bool bad_handle = !pk || (q.witness && !o) || (!host && (!w || (!q.witness && !px)));
  if (q.ticket_with_handles) {
    if (bad_handle || !q.ticket) return fail(GS_ERR_ARG, "%s: bad handle or null ticket", q.fn);
  } else if (bad_handle) return fail(GS_ERR_ARG, "%s: bad handle", q.fn);
  if (q.null_extra || !q.ticket || (host && !q.witness && ((q.nw && !q.w_host) || (q.npx && !q.px_host)))) return fail(GS_ERR_ARG, "null argument");
  if (host && !q.witness && (q.nw >= (1ull << 31) || q.npx >= (1ull << 31))) return fail(GS_ERR_ARG, "%s: too many scalars", q.fn);
  const size_t nw = host ? q.nw : w->n;
  if (q.witness && nw != o->m) return fail(GS_ERR_SHAPE, "len(w) = %zu but the system has %zu variables", nw, o->m);
  if ((host || q.witness) && nw != pk->nvars) return fail(GS_ERR_SHAPE, "len(w) = %zu but the key has %zu variables", nw, pk->nvars);   // before anything is staged
  if (q.refuse_slice && pk->shard_count != 1) return fail(GS_ERR_ARG, "%s: the key is a slice", q.fn);
  if (q.need_z && pk->nz == 0) return fail(GS_ERR_SHAPE, "the key has no Z");
  if (q.witness) if (int rc = check_domain_pair(q.fn, pk, o)) return rc;
  if (q.witness) if (int rc = check_coset_only_route(c, q.fn, pk, o)) return rc;
  std::vector<std::shared_ptr<Object>> keep = {c.share<Object>(q.hpk, q.kind)};
  if (q.witness) keep.push_back(c.share<Object>(q.hr1cs, Kind::R1cs));
  if (w) keep.push_back(c.share<Object>(q.hw, Kind::Scalars));
  if (px) keep.push_back(c.share<Object>(q.hpx, Kind::Scalars));
  const char* busy_hint = q.kind == Kind::GrothPk ? "call gs_groth16_prove_end first" : "call gs_pinocchio_prove_end first";
  return install_ticket(c, q.fn, busy_hint, pk, std::move(keep), Shard{}, w, px, q.ticket, [&] { return make(pk); }, [&](int parity, ProofInFlight& st) {
    if (host) {                                  // staged on the copy stream; one host wait for what was staged
      if (!c.copy_stream) GS_HIP(hipStreamCreateWithFlags(&c.copy_stream, hipStreamNonBlocking));
      st.th2d = std::make_shared<PhaseTimer>(c.copy_stream);
      // (a host witness lives in the slot's buffer until the ticket is collected -- the exact-route retry still finds it there)
      st.w = stage_slot_w(c, parity, q.w_host, nw);
      if (!q.witness) st.src = slot_px_from_host(c, parity, q.px_host, q.npx);
      GS_HIP(hipStreamSynchronize(c.copy_stream));
    } else {
      st.w = resident(w);
      if (!q.witness) st.src = resident_px(px);
    }
    // (with an evaluation-basis key nothing in the enqueue waits for the device; the other witness routes check on the host in there)
    if (q.witness) st.src = witness_source(pk, o, st.w.p, parity, eval_route(c, pk, o));
  });
}
// Collect a proof ticket that the caller took out of its slot: the sums, by the exact route if the witness broke a constraint.
int collect_ticket(Ctx& c, ProofInFlight& st, ProofSums& sums) {
  reset_timing(c);
  const int rc = proof_collect(c, st, sums);
  if (rc != kRetryExact) return rc;
  c.timing.fallbacks += 1;                       // the retry is a blocking proof at collection time
  return proof_sums_blocking(c, st.pk, st.w, exact_retry(st.src, c.blocking_slot()), Shard{}, sums);
}

// gs_*_prove_partials_values: the vector must hold exactly the values of the shard's evaluation-basis range
int check_values_slice(const char* fn, ProverKey* pk, const Scalars* hv, const Shard& sh, bool say_shard) {
  if (pk->n_eval == 0) return fail(GS_ERR_SHAPE, "%s: the key has no evaluation-basis array", fn);
  if (pk->eval_domain_log2) return fail(GS_ERR_SHAPE, "%s: the key's evaluation-basis array is the coset basis of a power-of-two domain, which the multi-device entry points do not serve", fn);
  size_t lo, hi;
  if (pk->shard_count > 1) { lo = pk->e_lo; hi = pk->e_lo + pk->n_e; } else shard_range(pk->n_eval, sh, lo, hi);
  if (hv->n == hi - lo) return GS_OK;
  if (!say_shard) return fail(GS_ERR_SHAPE, "%s: the shard covers %zu values, the vector holds %zu", fn, hi - lo, hv->n);
  return fail(GS_ERR_SHAPE, "%s: shard %zu of %zu covers %zu of the %zu values, the vector holds %zu", fn, sh.index, sh.count, hi - lo, pk->n_eval, hv->n);
}

}  // namespace

extern "C" {

int gs_groth16_prove(gs_handle hpk, const uint64_t* w, size_t nw, const uint64_t* px, size_t npx,
                     const uint64_t r[4], const uint64_t s[4], uint64_t out_proof[32], int inf[3]) {
  return guarded([&](Ctx& c) -> int {
    GrothPkObj* pk = c.get<GrothPkObj>(hpk, Kind::GrothPk);
    if (!pk) return fail(GS_ERR_ARG, "gs_groth16_prove: bad proving-key handle");
    if (!w || !px || !r || !s || !out_proof || !inf) return fail(GS_ERR_ARG, "null argument");
    reset_timing(c);
    const DevVec dw{upload_tmp(c, prove_state(c).up_w, w, nw), nw};
    prove_state(c).up_px.ensure(std::max<size_t>(npx, 1) * 32);
    const PxOnHost dp{prove_state(c).up_px.as<uint32_t>(), px, npx};            // copied inside, behind the work that only needs w
    return groth16_prove_impl(c, pk, dw, dp, r, s, out_proof, inf);
  }, true, false, hpk);
}

int gs_groth16_prove_resident(gs_handle hpk, gs_handle hw, gs_handle hpx, const uint64_t r[4], const uint64_t s[4],
                              uint64_t out_proof[32], int inf[3]) {
  return guarded([&](Ctx& c) -> int {
    GrothPkObj* pk = c.get<GrothPkObj>(hpk, Kind::GrothPk);
    Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
    Scalars* px = c.get<Scalars>(hpx, Kind::Scalars);
    if (!pk || !w || !px) return fail(GS_ERR_ARG, "gs_groth16_prove_resident: bad handle");
    if (!r || !s || !out_proof || !inf) return fail(GS_ERR_ARG, "null argument");
    reset_timing(c);
    return groth16_prove_impl(c, pk, resident(w), resident_px(px), r, s, out_proof, inf);
  }, true, false, hpk);
}

// A Groth16 proof ticket: the engine's, with the tail started on other host cores and its early products hooked into the fold.
static int groth16_begin(Ctx& c, TicketRequest q, const uint64_t r[4], const uint64_t s[4]) {
  q.kind = Kind::GrothPk;
  q.null_extra = !r || !s;
  q.ticket_with_handles = false;
  q.need_z = false;
  return begin_ticket(c, q, [r, s](ProverKey* pk) {
    auto st = std::make_unique<GrothInFlight>();
    GrothInFlight* raw = st.get();
    raw->with_tail = true;
    raw->tail.start(static_cast<GrothPkObj*>(pk), r, s);
    raw->on_g1w = [raw](const std::vector<G1Xyzz>& g1w) { raw->tail.early(g1w); };
    return st;
  });
}

int gs_groth16_prove_begin(gs_handle hpk, gs_handle hw, gs_handle hpx, const uint64_t r[4], const uint64_t s[4], uint64_t* ticket) {
  return guarded([&](Ctx& c) -> int {
    TicketRequest q{};
    q.fn = "gs_groth16_prove_begin"; q.hpk = hpk; q.hw = hw; q.hpx = hpx; q.ticket = ticket;
    return groth16_begin(c, q, r, s);
  }, true, true, hpk);
}

// groth16.GenerateProofs' own call shape, pipelined: w and px in caller memory, new ones with every call (host-buffer ticket, above).
int gs_groth16_prove_host_begin(gs_handle hpk, const uint64_t* w, size_t nw, const uint64_t* px, size_t npx, const uint64_t r[4], const uint64_t s[4],
                                uint64_t* ticket) {
  return guarded([&](Ctx& c) -> int {
    if (!w || !px) return fail(GS_ERR_ARG, "gs_groth16_prove_host_begin: null w or px");
    TicketRequest q{};
    q.fn = "gs_groth16_prove_host_begin"; q.hpk = hpk; q.w_host = w; q.nw = nw; q.px_host = px; q.npx = npx; q.ticket = ticket;
    return groth16_begin(c, q, r, s);
  }, true, true, hpk);
}

// The `_end` functions refuse a ticket that is not theirs BEFORE the in-flight object leaves its slot.
int gs_groth16_prove_end(uint64_t ticket, uint64_t out_proof[32], int inf[3]) {
  wait_ticket_unlocked(ticket);          // the device wait, outside the context lock (runtime.h)
  return guarded([&](Ctx& c) -> int {
    if (!out_proof || !inf) return fail(GS_ERR_ARG, "null argument");
    const int parity = find_ticket(c, "gs_groth16_prove_end", ticket);
    if (parity < 0) return GS_ERR_ARG;
    GrothInFlight* g = dynamic_cast<GrothInFlight*>(c.inflight[parity].get());
    if (!g) return fail(GS_ERR_ARG, "gs_groth16_prove_end: ticket %llu belongs to an MSM (use gs_msm_end)", (unsigned long long)ticket);
    if (!g->with_tail)
      return fail(GS_ERR_ARG, "gs_groth16_prove_end: ticket %llu is a partial-sums operation (use gs_groth16_partials_end)", (unsigned long long)ticket);
    std::shared_ptr<InFlightBase> base = std::move(c.inflight[parity]);
    ProofSums sums;
    const int rc = collect_ticket(c, *g, sums);
    if (rc != GS_OK) return rc;
    g->tail.finish(sums, out_proof, inf);
    return GS_OK;
  }, true, true, ticket);
}

// Sharded proving: the five raw sums over this rank's term ranges, as affine points.
int gs_groth16_prove_partials(gs_handle hpk, gs_handle hw, gs_handle hpx, size_t shard_index, size_t shard_count,
                              uint64_t out_sums[48], int inf[5]) {
  return guarded([&](Ctx& c) -> int {
    GrothPkObj* pk = c.get<GrothPkObj>(hpk, Kind::GrothPk);
    Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
    Scalars* px = c.get<Scalars>(hpx, Kind::Scalars);
    if (!pk || !w || !px) return fail(GS_ERR_ARG, "gs_groth16_prove_partials: bad handle");
    if (!out_sums || !inf || bad_shard(shard_index, shard_count)) return fail(GS_ERR_ARG, "gs_groth16_prove_partials: bad shard or null output");
    reset_timing(c);
    ProofSums sums;
    Shard sh; sh.index = shard_index; sh.count = shard_count;
    const int rc = proof_sums_blocking(c, pk, resident(w), resident_px(px), sh, sums);
    if (rc == GS_OK) groth16_pack_sums(sums, out_sums, inf);
    return rc;
  }, true, false, hpk);
}

// Strong scaling without a replicated polynomial stage ("run on GPU 0 and broadcast hx shards"), in two
// entry points.  gs_groth16_witness_values: ONE rank (the proof's owner; with a stream of proofs the ranks take turns) turns the
// resident witness into the n values H(n+1..2n) -- the whole polynomial stage of the evaluation-basis route -- as a resident scalar
// vector (*hv_inout as the px_inout of capi_r1cs.hip's resident px); *violated = number of roots of Z at which the witness breaks a constraint (the values are
// then meaningless: take the resident px + gs_groth16_prove_partials).  The owner scatters slice k of the vector to rank k
// (gs_scalars_clone between the logical devices of one process, gs_scalars_scatter over RCCL between processes), and ...
// (The same H for both schemes: the key only says which Z and how many constraints.)
static int witness_values_impl(Ctx& c, const char* fn, Kind kind, gs_handle hpk, gs_handle hr1cs, gs_handle hw, gs_handle* hv_inout, uint32_t* violated) {
  ProverKey* pk = c.get<ProverKey>(hpk, kind);
  if (!pk) return fail(GS_ERR_ARG, "%s: bad proving-key handle", fn);
  const size_t nz = pk->nz;
  R1csObj* o = c.get<R1csObj>(hr1cs, Kind::R1cs);
  Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
  if (!o || !w || !hv_inout || !violated) return fail(GS_ERR_ARG, "%s: bad handle or null output", fn);
  if (w->n != o->m) return fail(GS_ERR_SHAPE, "len(w) = %zu but the system has %zu variables", w->n, o->m);
  if (o->domain_log2) return fail(GS_ERR_SHAPE, "%s: an R1CS over a power-of-two domain is not served by the multi-device entry points", fn);
  if (!hx_shape(o->n, nz) || pk->n_eval != o->n || pk->eval_domain_log2)
    return fail(GS_ERR_SHAPE, "%s: the key has no evaluation-basis array for a system of %zu constraints", fn, o->n);
  Scalars* hv = inout_scalars(c, hv_inout, o->n, "%s: the output handle does not hold n = %zu values", fn);
  if (!hv) return GS_ERR_ARG;
  StreamScope sc(c, c.aux_stream[1]);             // the stream that carries every proof's polynomial stage (as capi_r1cs.hip's resident px)
  PhaseTimer t(c.stream);
  uint32_t* bad = c.bad_dev.as<uint32_t>() + c.blocking_slot();
  r1cs_values_dev(c, *o, w->buf.as<uint32_t>());
  r1cs_check_dev(c, o->vals.as<uint32_t>(), o->n, nz - 1, bad);
  hx_values_dev(c, o->vals.as<uint32_t>(), o->n, nz - 1, hv->buf.as<uint32_t>());
  GS_HIP(hipMemcpyAsync(c.bad_host + c.blocking_slot(), bad, 4, hipMemcpyDeviceToHost, c.stream));
  t.stop();
  GS_HIP(hipStreamSynchronize(c.stream));
  *violated = c.bad_host[c.blocking_slot()];
  if (!c.any_inflight()) reset_timing(c);
  c.timing.poly_ms = t.ms();
  c.timing.total_ms = c.timing.poly_ms;
  return GS_OK;
}

int gs_groth16_witness_values(gs_handle hpk, gs_handle hr1cs, gs_handle hw, gs_handle* hv_inout, uint32_t* violated) {
  return guarded([&](Ctx& c) -> int {
    return witness_values_impl(c, "gs_groth16_witness_values", Kind::GrothPk, hpk, hr1cs, hw, hv_inout, violated);
  }, true, true, hpk);
}

// ... every rank sums its term ranges: the four sums over its slice of w as gs_groth16_prove_partials does, the fifth over ITS slice
// of H's values (`hv_slice`: the n_e values of the key slice's evaluation-basis range) -- no polynomial work at all on this rank.
int gs_groth16_prove_partials_values(gs_handle hpk, gs_handle hw, gs_handle hv_slice, size_t shard_index, size_t shard_count,
                                     uint64_t out_sums[48], int inf[5]) {
  return guarded([&](Ctx& c) -> int {
    const char* fn = "gs_groth16_prove_partials_values";
    GrothPkObj* pk = c.get<GrothPkObj>(hpk, Kind::GrothPk);
    Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
    Scalars* hv = c.get<Scalars>(hv_slice, Kind::Scalars);
    if (!pk || !w || !hv) return fail(GS_ERR_ARG, "%s: bad handle", fn);
    if (!out_sums || !inf || bad_shard(shard_index, shard_count)) return fail(GS_ERR_ARG, "%s: bad shard or null output", fn);
    Shard sh; sh.index = shard_index; sh.count = shard_count;
    if (int rc = check_values_slice(fn, pk, hv, sh, true)) return rc;
    reset_timing(c);
    ProofSums sums;
    const int rc = proof_sums_blocking(c, pk, resident(w), values_slice(hv), sh, sums);
    if (rc == GS_OK) groth16_pack_sums(sums, out_sums, inf);
    return rc;
  }, true, false, hpk);
}

// The same, pipelined (a rank streams its shards of consecutive proofs: the plan and accumulations of shard work k + 1 queue behind
// those of k): gs_groth16_partials_values_begin enqueues and returns a ticket, gs_groth16_partials_end collects the five sums.
int gs_groth16_partials_values_begin(gs_handle hpk, gs_handle hw, gs_handle hv_slice, size_t shard_index, size_t shard_count, uint64_t* ticket) {
  return guarded([&](Ctx& c) -> int {
    const char* fn = "gs_groth16_partials_values_begin";
    GrothPkObj* pk = c.get<GrothPkObj>(hpk, Kind::GrothPk);
    Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
    Scalars* hv = c.get<Scalars>(hv_slice, Kind::Scalars);
    if (!pk || !w || !hv || !ticket) return fail(GS_ERR_ARG, "%s: bad handle or null ticket", fn);
    if (bad_shard(shard_index, shard_count)) return fail(GS_ERR_ARG, "%s: bad shard", fn);
    Shard sh; sh.index = shard_index; sh.count = shard_count;
    if (int rc = check_values_slice(fn, pk, hv, sh, false)) return rc;
    return install_ticket(c, fn, "collect one first", pk, {c.share<Object>(hpk, Kind::GrothPk), c.share<Object>(hw, Kind::Scalars), c.share<Object>(hv_slice, Kind::Scalars)},
                          sh, w, hv, ticket, [] { return std::make_unique<GrothInFlight>(); },
                          [&](int, ProofInFlight& st) { st.w = resident(w); st.src = values_slice(hv); });
  }, true, true, hpk);
}

int gs_groth16_partials_end(uint64_t ticket, uint64_t out_sums[48], int inf[5]) {
  wait_ticket_unlocked(ticket);          // the device wait, outside the context lock (runtime.h)
  return guarded([&](Ctx& c) -> int {
    if (!out_sums || !inf) return fail(GS_ERR_ARG, "null argument");
    const int parity = find_ticket(c, "gs_groth16_partials_end", ticket);
    if (parity < 0) return GS_ERR_ARG;
    GrothInFlight* g = dynamic_cast<GrothInFlight*>(c.inflight[parity].get());
    if (!g || g->with_tail) return fail(GS_ERR_ARG, "gs_groth16_partials_end: ticket %llu is not a partial-sums operation", (unsigned long long)ticket);
    std::shared_ptr<InFlightBase> base = std::move(c.inflight[parity]);
    reset_timing(c);
    ProofSums sums;
    const int rc = proof_collect(c, *g, sums);
    if (rc == GS_OK) groth16_pack_sums(sums, out_sums, inf);
    return rc;
  }, true, true, ticket);
}

// ... and the O(1) tail of groth16.go:253-275 on the combined sums (same layout as gs_groth16_prove_partials emits).
int gs_groth16_finish(gs_handle hpk, const uint64_t sums_in[48], const int inf_in[5], const uint64_t r[4], const uint64_t s[4],
                      uint64_t out_proof[32], int inf[3]) {
  return guarded([&](Ctx& c) -> int {
    GrothPkObj* pk = c.get<GrothPkObj>(hpk, Kind::GrothPk);
    if (!pk) return fail(GS_ERR_ARG, "gs_groth16_finish: bad proving-key handle");
    if (!sums_in || !inf_in || !r || !s || !out_proof || !inf) return fail(GS_ERR_ARG, "null argument");
    ProofSums sums;
    groth16_unpack_sums(sums_in, inf_in, sums);
    GrothTail tail;
    tail.start(pk, r, s);
    tail.finish(sums, out_proof, inf);
    return GS_OK;
  }, true, false, hpk);
}

// R1CS + witness -> proof in one call: the px stage (three interpolations and a product, r1csqap.go:161-210) runs on the aux
// stream BEHIND which H(x) waits anyway, while the main stream is already accumulating the four sums over w, which do not
// need px.  *px_inout as for capi_r1cs.hip's resident px (px stays available to the caller, as CombinePolynomials returns it).
int gs_groth16_prove_r1cs(gs_handle hpk, gs_handle hr1cs, gs_handle hw, gs_handle* px_inout, const uint64_t r[4], const uint64_t s[4],
                          uint64_t out_proof[32], int inf[3]) {
  return guarded([&](Ctx& c) -> int {
    GrothPkObj* pk = c.get<GrothPkObj>(hpk, Kind::GrothPk);
    R1csObj* o = c.get<R1csObj>(hr1cs, Kind::R1cs);
    Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
    if (!pk || !o || !w || !px_inout) return fail(GS_ERR_ARG, "gs_groth16_prove_r1cs: bad handle");
    if (!r || !s || !out_proof || !inf) return fail(GS_ERR_ARG, "null argument");
    if (w->n != o->m) return fail(GS_ERR_SHAPE, "len(w) = %zu but the system has %zu variables", w->n, o->m);
    if (int rc = check_domain_pair("gs_groth16_prove_r1cs", pk, o)) return rc;
    Scalars* px = inout_scalars(c, px_inout, o->npx(), "%s: the px handle does not hold 2n - 1 = %zu coefficients", "gs_groth16_prove_r1cs");
    if (!px) return GS_ERR_ARG;
    reset_timing(c);
    const uint32_t* wdev = w->buf.as<uint32_t>();
    return groth16_prove_impl(c, pk, DevVec{wdev, w->n}, PxFromR1cs{o, wdev, px->buf.as<uint32_t>()}, r, s, out_proof, inf);
  }, true, false, hpk);
}

// Witness -> proof (the witness routes above), blocking: the witness resident, or in host memory (the upload is part of the call,
// as in gs_groth16_prove).
static int groth16_prove_witness_impl(Ctx& c, const char* fn, gs_handle hpk, gs_handle hr1cs, bool host, gs_handle hw, const uint64_t* w_host, size_t nw_host,
                                      const uint64_t r[4], const uint64_t s[4], uint64_t out_proof[32], int inf[3]) {
  GrothPkObj* pk = c.get<GrothPkObj>(hpk, Kind::GrothPk);
  R1csObj* o = c.get<R1csObj>(hr1cs, Kind::R1cs);
  Scalars* w = host ? nullptr : c.get<Scalars>(hw, Kind::Scalars);
  if (!pk || !o || (!host && !w)) return fail(GS_ERR_ARG, "%s: bad handle", fn);
  if ((host && !w_host) || !r || !s || !out_proof || !inf) return fail(GS_ERR_ARG, "null argument");
  DevVec dw;
  HSource dp;
  if (int rc = witness_blocking_inputs(c, fn, pk, o, w, w_host, w ? w->n : nw_host, WitnessChecks{false, true}, dw, dp)) return rc;
  return groth16_prove_impl(c, pk, dw, dp, r, s, out_proof, inf);
}
int gs_groth16_prove_witness(gs_handle hpk, gs_handle hr1cs, gs_handle hw, const uint64_t r[4], const uint64_t s[4], uint64_t out_proof[32], int inf[3]) {
  return guarded([&](Ctx& c) -> int {
    return groth16_prove_witness_impl(c, "gs_groth16_prove_witness", hpk, hr1cs, false, hw, nullptr, 0, r, s, out_proof, inf);
  }, true, false, hpk);
}
int gs_groth16_prove_witness_host(gs_handle hpk, gs_handle hr1cs, const uint64_t* w, size_t nw, const uint64_t r[4], const uint64_t s[4],
                                  uint64_t out_proof[32], int inf[3]) {
  return guarded([&](Ctx& c) -> int {
    return groth16_prove_witness_impl(c, "gs_groth16_prove_witness_host", hpk, hr1cs, true, 0, w, nw, r, s, out_proof, inf);
  }, true, false, hpk);
}

// The same, pipelined: a ticket for gs_groth16_prove_end (which also runs the exact route, blocking, should the witness turn out
// to violate a constraint).
int gs_groth16_prove_witness_begin(gs_handle hpk, gs_handle hr1cs, gs_handle hw, const uint64_t r[4], const uint64_t s[4], uint64_t* ticket) {
  return guarded([&](Ctx& c) -> int {
    TicketRequest q{};
    q.fn = "gs_groth16_prove_witness_begin"; q.hpk = hpk; q.hr1cs = hr1cs; q.witness = true; q.hw = hw; q.ticket = ticket; q.refuse_slice = true;
    return groth16_begin(c, q, r, s);
  }, true, true, hpk);
}

// The reference's call shape for a server that keeps circuit and key resident: every call brings a NEW witness in host memory
// (cli/main.go:480-501 computes w per proof) and nothing else -- a host-buffer ticket (see stage_slot_w).  Collect with gs_groth16_prove_end.
int gs_groth16_prove_witness_host_begin(gs_handle hpk, gs_handle hr1cs, const uint64_t* w, size_t nw, const uint64_t r[4], const uint64_t s[4],
                                        uint64_t* ticket) {
  return guarded([&](Ctx& c) -> int {
    if (!w) return fail(GS_ERR_ARG, "gs_groth16_prove_witness_host_begin: null witness");
    if (nw >= (1ull << 31)) return fail(GS_ERR_ARG, "gs_groth16_prove_witness_host_begin: too many scalars");
    TicketRequest q{};
    q.fn = "gs_groth16_prove_witness_host_begin"; q.hpk = hpk; q.hr1cs = hr1cs; q.witness = true; q.w_host = w; q.nw = nw; q.ticket = ticket;
    q.refuse_slice = true;
    return groth16_begin(c, q, r, s);
  }, true, true, hpk);
}

// ---- Pinocchio ----------------------------------------------------------------------------------------------
int gs_pinocchio_prove(gs_handle hpk, const uint64_t* w, size_t nw, const uint64_t* px, size_t npx, uint64_t out_proof[72], int inf[8]) {
  return guarded([&](Ctx& c) -> int {
    PinocchioPkObj* pk = c.get<PinocchioPkObj>(hpk, Kind::PinocchioPk);
    if (!pk) return fail(GS_ERR_ARG, "gs_pinocchio_prove: bad proving-key handle");
    if (!w || !px || !out_proof || !inf) return fail(GS_ERR_ARG, "null argument");
    reset_timing(c);
    const DevVec dw{upload_tmp(c, prove_state(c).up_w, w, nw), nw};
    prove_state(c).up_px.ensure(std::max<size_t>(npx, 1) * 32);
    const PxOnHost dp{prove_state(c).up_px.as<uint32_t>(), px, npx};            // copied inside, behind the work that only needs w
    return pinocchio_prove_impl(c, pk, dw, dp, out_proof, inf);
  }, true, false, hpk);
}

// Pipelined Pinocchio proving: same ticket discipline as gs_groth16_prove_begin / _end (they share the three slots).
static int pinocchio_begin(Ctx& c, TicketRequest q) {
  q.kind = Kind::PinocchioPk;
  q.ticket_with_handles = true;
  q.need_z = q.witness;
  return begin_ticket(c, q, [](ProverKey*) { return std::make_unique<ProofInFlight>(); });
}

int gs_pinocchio_prove_begin(gs_handle hpk, gs_handle hw, gs_handle hpx, uint64_t* ticket) {
  return guarded([&](Ctx& c) -> int {
    TicketRequest q{};
    q.fn = "gs_pinocchio_prove_begin"; q.hpk = hpk; q.hw = hw; q.hpx = hpx; q.ticket = ticket;
    return pinocchio_begin(c, q);
  }, true, true, hpk);
}

int gs_pinocchio_prove_host_begin(gs_handle hpk, const uint64_t* w, size_t nw, const uint64_t* px, size_t npx, uint64_t* ticket) {
  return guarded([&](Ctx& c) -> int {
    if (!w || !px) return fail(GS_ERR_ARG, "gs_pinocchio_prove_host_begin: null w or px");
    TicketRequest q{};
    q.fn = "gs_pinocchio_prove_host_begin"; q.hpk = hpk; q.w_host = w; q.nw = nw; q.px_host = px; q.npx = npx; q.ticket = ticket;
    return pinocchio_begin(c, q);
  }, true, true, hpk);
}

int gs_pinocchio_prove_end(uint64_t ticket, uint64_t out_proof[72], int inf[8]) {
  wait_ticket_unlocked(ticket);          // the device wait, outside the context lock (runtime.h)
  return guarded([&](Ctx& c) -> int {
    if (!out_proof || !inf) return fail(GS_ERR_ARG, "null argument");
    const int parity = find_ticket(c, "gs_pinocchio_prove_end", ticket);
    if (parity < 0) return GS_ERR_ARG;
    ProofInFlight* st = dynamic_cast<ProofInFlight*>(c.inflight[parity].get());
    if (!st || st->pk->kind != Kind::PinocchioPk)
      return fail(GS_ERR_ARG, "gs_pinocchio_prove_end: ticket %llu is not a Pinocchio proof", (unsigned long long)ticket);
    std::shared_ptr<InFlightBase> base = std::move(c.inflight[parity]);
    ProofSums sums;
    const int rc = collect_ticket(c, *st, sums);
    if (rc == GS_OK) pinocchio_pack(sums, out_proof, inf);
    return rc;
  }, true, true, ticket);
}

int gs_pinocchio_prove_resident(gs_handle hpk, gs_handle hw, gs_handle hpx, uint64_t out_proof[72], int inf[8]) {
  return guarded([&](Ctx& c) -> int {
    PinocchioPkObj* pk = c.get<PinocchioPkObj>(hpk, Kind::PinocchioPk);
    Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
    Scalars* px = c.get<Scalars>(hpx, Kind::Scalars);
    if (!pk || !w || !px) return fail(GS_ERR_ARG, "gs_pinocchio_prove_resident: bad handle");
    if (!out_proof || !inf) return fail(GS_ERR_ARG, "null argument");
    reset_timing(c);
    return pinocchio_prove_impl(c, pk, resident(w), resident_px(px), out_proof, inf);
  }, true, false, hpk);
}

// ---- Pinocchio over several GPUs (SURVEY 8e applied to snark.go:254-289) ------------------------------------------------------
// A Pinocchio proof IS its eight MSM sums (there is no tail): rank k of N sums its term ranges, the eight partial points of the
// ranks add up to the proof.  Key slices, partial sums (from px, or from the owner's slice of H's values), and the addition.
// the eight sums over this rank's term ranges, in the layout of a proof (PiA | PiAp | PiB | PiBp | PiC | PiCp | PiH | PiKp)
int gs_pinocchio_prove_partials(gs_handle hpk, gs_handle hw, gs_handle hpx, size_t shard_index, size_t shard_count, uint64_t out_sums[72], int inf[8]) {
  return guarded([&](Ctx& c) -> int {
    PinocchioPkObj* pk = c.get<PinocchioPkObj>(hpk, Kind::PinocchioPk);
    Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
    Scalars* px = c.get<Scalars>(hpx, Kind::Scalars);
    if (!pk || !w || !px) return fail(GS_ERR_ARG, "gs_pinocchio_prove_partials: bad handle");
    if (!out_sums || !inf || bad_shard(shard_index, shard_count)) return fail(GS_ERR_ARG, "gs_pinocchio_prove_partials: bad shard or null output");
    reset_timing(c);
    Shard sh; sh.index = shard_index; sh.count = shard_count;
    return pinocchio_prove_impl(c, pk, resident(w), resident_px(px), out_sums, inf, sh);
  }, true, false, hpk);
}

// the owner's polynomial stage (as gs_groth16_witness_values)
int gs_pinocchio_witness_values(gs_handle hpk, gs_handle hr1cs, gs_handle hw, gs_handle* hv_inout, uint32_t* violated) {
  return guarded([&](Ctx& c) -> int {
    return witness_values_impl(c, "gs_pinocchio_witness_values", Kind::PinocchioPk, hpk, hr1cs, hw, hv_inout, violated);
  }, true, true, hpk);
}

// ... and the ranks' sums with PiH over THEIR slice of those values (no polynomial work on this rank)
int gs_pinocchio_prove_partials_values(gs_handle hpk, gs_handle hw, gs_handle hv_slice, size_t shard_index, size_t shard_count,
                                       uint64_t out_sums[72], int inf[8]) {
  return guarded([&](Ctx& c) -> int {
    const char* fn = "gs_pinocchio_prove_partials_values";
    PinocchioPkObj* pk = c.get<PinocchioPkObj>(hpk, Kind::PinocchioPk);
    Scalars* w = c.get<Scalars>(hw, Kind::Scalars);
    Scalars* hv = c.get<Scalars>(hv_slice, Kind::Scalars);
    if (!pk || !w || !hv) return fail(GS_ERR_ARG, "%s: bad handle", fn);
    if (!out_sums || !inf || bad_shard(shard_index, shard_count)) return fail(GS_ERR_ARG, "%s: bad shard or null output", fn);
    Shard sh; sh.index = shard_index; sh.count = shard_count;
    if (int rc = check_values_slice(fn, pk, hv, sh, true)) return rc;
    reset_timing(c);
    return pinocchio_prove_impl(c, pk, resident(w), values_slice(hv), out_sums, inf, sh);
  }, true, false, hpk);
}

// the addition: n records of eight sums (the layout above, n x 72 words and n x 8 flags) -> the proof.  Host arithmetic on 8 n points.
int gs_pinocchio_combine(const uint64_t* sums, const int* inf_in, size_t n, uint64_t out_proof[72], int inf[8]) {
  if (!sums || !inf_in || !out_proof || !inf || n == 0) return fail(GS_ERR_ARG, "gs_pinocchio_combine: null argument or no records");
  static const int off[8] = {0, 8, 16, 32, 40, 48, 56, 64};
  std::vector<uint64_t> pts(n * 16);
  std::vector<int> fl(n);
  for (int k = 0; k < 8; ++k) {
    const bool g2 = k == 2;
    const size_t words = g2 ? 16 : 8;
    for (size_t i = 0; i < n; ++i) { memcpy(&pts[i * words], sums + i * 72 + off[k], words * 8); fl[i] = inf_in[i * 8 + k]; }
    const int rc = g2 ? gs_g2_sum_affine(pts.data(), fl.data(), n, out_proof + off[k], &inf[k]) : gs_g1_sum_affine(pts.data(), fl.data(), n, out_proof + off[k], &inf[k]);
    if (rc != GS_OK) return rc;
  }
  return GS_OK;
}

// snark.GenerateProofs straight from the witness (the Pinocchio twin of gs_groth16_prove_witness): CombinePolynomials + Div
// (r1csqap.go:191-216, snark.go:280) collapse into H's values (evaluation-basis key) or H(x) from the constraint values; the exact
// px route when a constraint is violated.
static int pinocchio_prove_witness_impl(Ctx& c, const char* fn, gs_handle hpk, gs_handle hr1cs, bool host, gs_handle hw, const uint64_t* w_host, size_t nw_host,
                                        uint64_t out_proof[72], int inf[8]) {
  PinocchioPkObj* pk = c.get<PinocchioPkObj>(hpk, Kind::PinocchioPk);
  R1csObj* o = c.get<R1csObj>(hr1cs, Kind::R1cs);
  Scalars* w = host ? nullptr : c.get<Scalars>(hw, Kind::Scalars);
  if (!pk || !o || (!host && !w)) return fail(GS_ERR_ARG, "%s: bad handle", fn);
  if ((host && !w_host) || !out_proof || !inf) return fail(GS_ERR_ARG, "null argument");
  DevVec dw;
  HSource dp;
  if (int rc = witness_blocking_inputs(c, fn, pk, o, w, w_host, w ? w->n : nw_host, WitnessChecks{true, false}, dw, dp)) return rc;
  return pinocchio_prove_impl(c, pk, dw, dp, out_proof, inf);
}
int gs_pinocchio_prove_witness(gs_handle hpk, gs_handle hr1cs, gs_handle hw, uint64_t out_proof[72], int inf[8]) {
  return guarded([&](Ctx& c) -> int {
    return pinocchio_prove_witness_impl(c, "gs_pinocchio_prove_witness", hpk, hr1cs, false, hw, nullptr, 0, out_proof, inf);
  }, true, false, hpk);
}
int gs_pinocchio_prove_witness_host(gs_handle hpk, gs_handle hr1cs, const uint64_t* w, size_t nw, uint64_t out_proof[72], int inf[8]) {
  return guarded([&](Ctx& c) -> int {
    return pinocchio_prove_witness_impl(c, "gs_pinocchio_prove_witness_host", hpk, hr1cs, true, 0, w, nw, out_proof, inf);
  }, true, false, hpk);
}

int gs_pinocchio_prove_witness_begin(gs_handle hpk, gs_handle hr1cs, gs_handle hw, uint64_t* ticket) {
  return guarded([&](Ctx& c) -> int {
    TicketRequest q{};
    q.fn = "gs_pinocchio_prove_witness_begin"; q.hpk = hpk; q.hr1cs = hr1cs; q.witness = true; q.hw = hw; q.ticket = ticket;
    return pinocchio_begin(c, q);
  }, true, true, hpk);
}

// host-buffer tickets of snark.GenerateProofs (see gs_groth16_prove_witness_host_begin / gs_groth16_prove_host_begin)
int gs_pinocchio_prove_witness_host_begin(gs_handle hpk, gs_handle hr1cs, const uint64_t* w, size_t nw, uint64_t* ticket) {
  return guarded([&](Ctx& c) -> int {
    if (!w) return fail(GS_ERR_ARG, "gs_pinocchio_prove_witness_host_begin: null witness");
    if (nw >= (1ull << 31)) return fail(GS_ERR_ARG, "gs_pinocchio_prove_witness_host_begin: too many scalars");
    TicketRequest q{};
    q.fn = "gs_pinocchio_prove_witness_host_begin"; q.hpk = hpk; q.hr1cs = hr1cs; q.witness = true; q.w_host = w; q.nw = nw; q.ticket = ticket;
    return pinocchio_begin(c, q);
  }, true, true, hpk);
}

}  // extern "C"
