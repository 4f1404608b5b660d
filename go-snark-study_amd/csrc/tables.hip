// Window tables: the builders' launches and a table's life cycle (tables.h).  Every transition between a table's states -- none,
// building k of n, resident -- is made here and nowhere else.
#include "msm.h"

#include "table_kernels.h"

namespace gs {

struct TableState {                                // per context (device memory belongs to one device)
  DevBuf scratch;                                  // slab of the batched window-table builder: blocking builds, on the call's stream
  DevBuf scratch_pending;                          // ... and the instalments of pending builds, on the main stream
};
static TableState& table_state(Ctx& c) { return c.state<TableState>(c.table_state); }

// Enqueue the kernels that fill rows [first, last) of every row of `rows` (W rows of n points, allocated) from row 0 on `stream`.
// slab: points per launch (2^18 = 1024 workgroups).
template <class T>
static void enqueue_table_slabs(hipStream_t stream, DevBuf& scratch, const uint32_t* src, size_t n, int cbits, DevBuf& rows, size_t first, size_t last,
                                size_t slab) {
  const int W = 254 / cbits + 1;
  if (first >= last) return;
  static const bool per_row = dev_flag("GS_TABLE_PER_ROW");               // the one-inversion-per-row builder, for comparison
  if (per_row || W <= 2) {
    // (whole table at once: this builder has no range form; only reached with W <= 2, i.e. never for BN254 widths <= 20)
    if (first == 0) hipLaunchKernelGGL(k_build_table<T>, grid1(n), dim3(256), 0, stream, src, (uint32_t)n, cbits, W, rows.as<uint32_t>());
  } else {
    // slabs: (W - 1) rows of [XYZZ | running product] raw limbs per point (<= 1.4 GiB for G2 at 2^18 points), reused per slab
    constexpr size_t sw = PointIO<T>::kXyzzWords + PointIO<T>::kXyzzWords / 4;
    slab = std::min<size_t>(std::max<size_t>(slab, 1), n);
    scratch.ensure(slab * (size_t)(W - 1) * sw * 4);
    for (size_t at = first; at < last; at += slab) {
      const size_t count = std::min(slab, last - at);
      hipLaunchKernelGGL(k_build_table_batched<T>, grid1(count), dim3(256), 0, stream, src, (uint32_t)n, (uint32_t)at, (uint32_t)count, cbits, W,
                         rows.as<uint32_t>(), scratch.as<uint32_t>());
    }
  }
  GS_HIP(hipGetLastError());
}
static void enqueue_table_slabs(bool g2, hipStream_t stream, DevBuf& scratch, const uint32_t* src, size_t n, int cbits, DevBuf& rows, size_t first,
                                size_t last, size_t slab) {
  if (g2) enqueue_table_slabs<Fq2Tag>(stream, scratch, src, n, cbits, rows, first, last, slab);
  else enqueue_table_slabs<FqTag>(stream, scratch, src, n, cbits, rows, first, last, slab);
}

// (Re)build the table for window width cbits from row 0 (`row0` = packed affine points; nullptr = the table's own row 0), blocking.
// No-op when the table already matches.
void BaseTable::ensure(Ctx& ctx, const uint32_t* row0, size_t n_, int cbits, bool g2) {
  if (ready(n_, cbits)) return;
  discard();                                    // a pending build of another width: superseded
  const uint32_t* src = row0 ? row0 : rows.as<uint32_t>();
  if (!src || (!row0 && n != n_)) throw HipError{hipErrorInvalidValue, "window table rebuild without its points", __LINE__};
  const int W_ = 254 / cbits + 1;
  DevBuf fresh;
  fresh.alloc(std::max<size_t>(n_, 1) * W_ * (g2 ? PointIO<Fq2Tag>::kAffineWords : PointIO<FqTag>::kAffineWords) * 4);
  enqueue_table_slabs(g2, ctx.stream, table_state(ctx).scratch, src, n_, cbits, fresh, 0, n_, (size_t)1 << 18);
  GS_HIP(hipStreamSynchronize(ctx.stream));     // the old rows (possibly the source) are released below
  rows = std::move(fresh);
  n = n_; c = cbits; W = W_;
  uses = 0;
}

// ---- when a base array gets its table (gs_set_table_policy) ---------------------------------------------------------------------
// The reference proves ONCE per key load (cli/main.go:330-349); 15-row tables cost ~140 ms and 15x the key's memory at 2^20 -- fifteen
// proofs' worth of work before the first one.  Under `auto` a base array is summed table-free until it has been used
// kTableAfterUses times; from then on every call that finds it without a table builds a few more slabs of it.
//
// Round 6: IN INSTALMENTS, in front of the call's own accumulations, on the accumulation stream.  Round 5 enqueued
// all five builds of a key at once on a lowest-priority stream and let the hardware share the chip: proofs 2-10 of a fresh 2^20 key took
// 19-35 ms each, unpredictably, and a proof could not use a table the moment it was complete.  The work is what it is -- ~125 ms of
// full-chip time per 2^20 Groth16 key, and whatever runs beside it is slowed by what it takes ("what overlap can and
// cannot buy") -- so the only choice is how it is spread over the calls: each call gets a build CREDIT proportional to its own work
// (tables.h, kBuildCreditPerUnitTerm: ~+80 % of a table-free call), spends it on whole slabs of the pending table (the balance, at most one
// slab either way, stays on the context), and the call that enqueues the last slab installs the table and uses it -- stream order makes
// that safe without a host wait.  A fresh 2^20 key: 24 ms, then ~16 proofs of <= 2x the steady time, then steady; a proof never waits for
// more than its own instalment.  GS_TABLE_BUDGET_PCT scales the credit (100 = as described; 100000 = everything inside the second call).
constexpr uint32_t kTableAfterUses = 2;

static size_t instalment_slab(size_t n, bool g2) {
  // As LARGE as possible: a builder thread walks its point through 14 x 17 dependent doublings, ~1.3 ms for a lone wave whatever the
  // slab holds, so a slab must fill the chip to be worth its launch.  2^18 points for G1 (4 waves per SIMD: 5 ms) and 2^17 for G2
  // (5.7 ms), the whole table when it is smaller (GS_TABLE_BG_SLAB_LOG2 caps the G1 figure).  Measured on fresh keys
  // (profiles/r06_auto_instalments.txt): with slabs of n / 8 points a 2^16 key's tables took 75 ms of instalments instead of 9, and
  // 2^17-point G1 slabs cost a 2^20 key 168 ms against the 130 ms `always` spends in 2^18-point launches.
  static const size_t cap = (size_t)1 << run_knob("GS_TABLE_BG_SLAB_LOG2", 18, 10, 18);
  return std::min(g2 ? std::max<size_t>(cap / 2, (size_t)1 << 12) : cap, std::max<size_t>(n, 1));
}

bool BaseTable::begin(Ctx& ctx, const TableRef& r, int cbits) {
  if (!pending.done) GS_HIP(hipEventCreateWithFlags(&pending.done, hipEventDisableTiming));
  const int W_ = 254 / cbits + 1;
  const size_t aw = r.g2 ? PointIO<Fq2Tag>::kAffineWords : PointIO<FqTag>::kAffineWords;
  try {
    // the slab scratch at its G2 size BEFORE the first launch: growing it later releases the old buffer, and hipFree waits for the
    // device -- for the slabs just enqueued (round 5: that, not the builds' share of the chip, was most of a second proof's 88 ms)
    constexpr size_t sw2 = PointIO<Fq2Tag>::kXyzzWords + PointIO<Fq2Tag>::kXyzzWords / 4;
    if (W_ > 2) {     // (a G1 slab may be twice a G2 slab's points, and a G1 point's scratch is half a G2 point's: the same bytes)
      constexpr size_t sw1 = PointIO<FqTag>::kXyzzWords + PointIO<FqTag>::kXyzzWords / 4;
      const size_t s2 = instalment_slab(r.n, true), s1 = instalment_slab(r.n, false);
      const size_t bytes = std::max((s2 + s2 / 4) * sw2, (s1 + s1 / 4) * sw1);
      table_state(ctx).scratch_pending.ensure(bytes * (size_t)(W_ - 1) * 4);
    }
    pending.rows.alloc(std::max<size_t>(r.n, 1) * W_ * aw * 4);
  } catch (const HipError& e) {
    if (e.e != hipErrorOutOfMemory) throw;      // no room for a table: keep summing table-free
    pending.rows.release();
    return false;
  }
  pending.c = cbits; pending.n = r.n; pending.next = 0; pending.src = r.row0; pending.g2 = r.g2;
  return true;
}

// launches for points [next, last) of the pending table, `slab` points each, on the main stream
void BaseTable::enqueue(Ctx& ctx, size_t last, size_t slab) {
  enqueue_table_slabs(pending.g2, ctx.main_stream, table_state(ctx).scratch_pending, pending.src, pending.n, pending.c, pending.rows, pending.next,
                      last, slab);
  pending.next = last;
}

// spend credit on the next slabs of the pending table; true when the last slab has been enqueued
bool BaseTable::advance(Ctx& ctx, double& credit) {
  const double unit = pending.g2 ? kG2BuildCost : 1.0;
  const size_t slab = instalment_slab(pending.n, pending.g2), first = pending.next;
  while (pending.next < pending.n) {
    // (a remainder of up to a quarter slab rides with the last one: a key of 2^k + 1 variables must not end on a one-point launch)
    const size_t last = pending.n - pending.next <= slab + slab / 4 ? pending.n : pending.next + slab;
    // a slab is bought when the credit covers at least half of it (the call overdraws by at most half a slab, ~2.5 ms at 2^20, and the
    // next call's grant is that much smaller): the instalments of consecutive calls then differ by one slab at most
    if (credit < 0.5 * (double)(last - pending.next) * unit) break;
    credit -= (double)(last - pending.next) * unit;
    enqueue(ctx, last, last - pending.next);
  }
  // behind every instalment, not only the last: whoever discards the build waits for the slabs it has in flight
  if (pending.next > first) GS_HIP(hipEventRecord(pending.done, ctx.main_stream));
  return pending.next >= pending.n;
}

// the one place where a build becomes the table ...
void BaseTable::install() {
  rows = std::move(pending.rows);               // (old rows, if any, are released by the move: hipFree waits for every reader of them)
  n = pending.n; c = pending.c; W = 254 / pending.c + 1;
  uses = 0;
  clear_build();
}
// ... and the one that forgets it
void BaseTable::clear_build() {
  pending.rows.release();
  pending.c = 0; pending.n = 0; pending.next = 0; pending.src = nullptr;
}

// install a table whose last slab has been ENQUEUED (not necessarily executed): everything that reads it is ordered behind the slab.
// Accumulations run on the main stream, where the slabs are; the other streams of the context wait for the event.
void BaseTable::install_enqueued(Ctx& ctx) {
  if (hipEventQuery(pending.done) != hipSuccess)
    for (auto a : ctx.aux_stream) if (a && a != ctx.main_stream) GS_HIP(hipStreamWaitEvent(a, pending.done, 0));
  (void)hipGetLastError();                                                     // hipErrorNotReady is not an error
  install();
}

// finish the missing instalments now, wait for them on the host and install (gs_build_tables on a key that was warming up)
void BaseTable::finish_now(Ctx& ctx) {
  if (pending.next < pending.n) {
    enqueue(ctx, pending.n, (size_t)1 << 18);
    GS_HIP(hipEventRecord(pending.done, ctx.main_stream));
  }
  if (pending.next > 0) GS_HIP(hipEventSynchronize(pending.done));
  install();
}

// give up a build: wait for the slabs it has in flight (they write its rows and the slab scratch), then free the rows
void BaseTable::discard() {
  if (!building()) return;
  if (pending.next > 0) GS_HIP(hipEventSynchronize(pending.done));
  clear_build();
}

void BaseTable::build_now(Ctx& ctx, const uint32_t* row0, size_t n_, int cbits, bool g2) {
  if (building(n_, cbits)) finish_now(ctx);
  else discard();
  ensure(ctx, row0, n_, cbits, g2);
}

void stamp_tables(Ctx& c, const std::vector<BaseTable*>& tables) {
  for (BaseTable* t : tables) if (t) t->last_use = c.call_clock;
}

bool prepare_tables(Ctx& c, const std::vector<TableRef>& group, uint32_t nterms, int* cbits, double* credit) {
  int cb = choose_window_bits(std::max<uint32_t>(nterms, 1u), c.window_bits);
  // A group whose tables are all resident at ONE width next to the model's serves at that width (gs_build_tables sizes a
  // key's tables for the arrays it holds, a proof asks for the width of its term range -- near a boundary of the model the warmed
  // table was silently ignored or rebuilt, and callers alternating two MSM lengths over one array flip-flopped it).
  if (c.window_bits == 0 && !group.empty() && group[0].t->rows.p) {
    const int tc = group[0].t->c;
    bool same = tc >= cb - 1 && tc <= cb + 1;
    for (const TableRef& r : group) same = same && r.t->ready(r.n, tc);
    if (same) cb = tc;
  }
  bool all_ready = true;
  for (const TableRef& r : group) {
    r.t->last_use = c.call_clock;
    all_ready = all_ready && r.t->ready(r.n, cb);
  }
  if (all_ready) {
    for (const TableRef& r : group) r.t->last_table_use = c.call_clock;
    *cbits = cb;
    return true;
  }
  if (c.table_policy == 1) {                                                   // always: inside the call, as rounds 1-4 did
    for (const TableRef& r : group) {
      r.t->ensure(c, r.row0, r.n, cb, r.g2);
      r.t->last_table_use = c.call_clock;
    }
    *cbits = cb;
    return true;
  }
  if (c.table_policy == 0) {
    static const double scale = (double)run_knob("GS_TABLE_BUDGET_PCT", 100, 1, 1000000) / 100.0;
    // what this call may still enqueue: its grant (what an earlier group of the same call left of it) minus the last call's overdraft
    const double grant = credit ? *credit : 0.0;
    double avail = grant * scale + c.build_balance;
    // G2 arrays first: the G2 sum is the longest of a proof, so its table is the one that pays most per call
    std::vector<const TableRef*> order;
    for (const TableRef& r : group) if (r.g2) order.push_back(&r);
    for (const TableRef& r : group) if (!r.g2) order.push_back(&r);
    for (const TableRef* pr : order) {
      const TableRef& r = *pr;
      BaseTable& t = *r.t;
      if (t.ready(r.n, cb)) continue;
      if (!t.building(r.n, cb, r.row0)) t.discard();                              // a build of another shape: superseded
      if (!t.building()) {
        t.uses += 1;
        // a table of another width that still serves other calls stays (callers alternating two lengths over one array)
        const bool serving = t.rows.p && c.call_clock - t.last_table_use <= 8;
        if (t.uses < kTableAfterUses || !r.n || serving) continue;
        if (!t.begin(c, r, cb)) continue;
      }
      if (t.advance(c, avail)) t.install_enqueued(c);
    }
    c.build_balance = std::min(avail, 0.0);                       // an overdraft (less than one slab) comes off the next call's grant
    if (credit) *credit = std::max(avail, 0.0) / scale;           // the rest of the grant is the call's next group's
    bool now_ready = true;
    for (const TableRef& r : group) now_ready = now_ready && r.t->ready(r.n, cb);
    if (now_ready) {                                              // this call enqueued the last slab: it is the first to use the tables
      for (const TableRef& r : group) r.t->last_table_use = c.call_clock;
      *cbits = cb;
      return true;
    }
  }
  *cbits = choose_window_bits_free(std::max<uint32_t>(nterms, 1u), c.window_bits);
  return false;
}

}  // namespace gs
