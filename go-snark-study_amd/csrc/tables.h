// Window tables of base arrays and their life cycle (implemented in tables.hip, the only place that starts, advances, installs or
// discards a build).
#pragma once
#include <algorithm>
#include <vector>

#include "runtime.h"

namespace gs {

struct TableRef;

// Window table of a base array: rows[j][i] = 2^(c j) * P_i (packed affine), j < W = 254 / c + 1.
// A table is in one of three states: none, building (k of n points enqueued, policy auto only) or resident.  A resident table of
// one width may stand beside the build of another; the build replaces it when its last slab has been enqueued.
struct BaseTable {
  DevBuf rows;
  size_t n = 0;
  int c = 0, W = 0;
  uint64_t last_use = 0;           // Ctx::call_clock of the last call that used the array (LRU order of evict_tables_for)
  uint64_t last_table_use = 0;     // ... of the last call that summed it over its TABLE: under policy auto a table that serves is not
                                   //     replaced by one of another width just because one call wanted that width
  uint32_t uses = 0;               // proofs / MSMs that found no table since it last had one (table policy auto)
  bool ready(size_t n_, int c_) const { return rows.p != nullptr && n == n_ && c == c_; }
  uint64_t bytes() const { return rows.bytes + pending.rows.bytes; }
  // what evict_tables_for may take: rows that no build is about to replace and that the running call has not stamped
  bool evictable(uint64_t call_clock) const { return rows.p && !building() && last_use != call_clock; }
  void evict() { drop(); uses = 0; }
  // The array's points were replaced or detached: discard any build and drop the rows.  The use count stays, so an array that had
  // earned its table starts the next one with its next call.
  void invalidate() { discard(); drop(); }
  // gs_release_tables: the same, and the array earns its next table from the start
  void release() { invalidate(); uses = 0; }
  // gs_build_tables: the table of width cbits NOW, blocking, whatever the policy -- a build of that shape is finished, any other discarded
  void build_now(Ctx& c, const uint32_t* row0, size_t n_, int cbits, bool g2);
  BaseTable() = default;
  BaseTable(const BaseTable&) = delete;
  BaseTable& operator=(const BaseTable&) = delete;
  ~BaseTable() { if (pending.done && !process_exiting()) (void)hipEventDestroy(pending.done); }

 private:
  friend bool prepare_tables(Ctx& c, const std::vector<TableRef>& group, uint32_t nterms, int* cbits, double* credit);
  // A build under policy auto, in instalments.  `rows` are those of the table to be; every call that finds the array without its
  // table enqueues the next slabs of points [next, ...) on the accumulation stream, as many as its build credit pays for
  // (prepare_tables), and the call that enqueues the last slab installs the table: its accumulation kernel runs behind the slabs on
  // the same stream.
  struct {
    DevBuf rows;
    int c = 0;
    size_t n = 0, next = 0;
    const uint32_t* src = nullptr;      // row 0 (the base array: lives as long as the object that owns this table)
    bool g2 = false;
    hipEvent_t done = nullptr;          // recorded on the main stream behind every instalment
  } pending;
  bool building() const { return pending.rows.p != nullptr; }
  bool building(size_t n_, int c_) const { return building() && pending.n == n_ && pending.c == c_; }                          // ... of this shape
  bool building(size_t n_, int c_, const uint32_t* src) const { return building(n_, c_) && pending.src == src; }             // ... from these points
  void drop() { rows.release(); n = 0; c = 0; W = 0; }
  void ensure(Ctx& c, const uint32_t* row0, size_t n_, int cbits, bool g2);     // the blocking build
  bool begin(Ctx& c, const TableRef& r, int cbits);
  bool advance(Ctx& c, double& credit);
  void enqueue(Ctx& c, size_t last, size_t slab);
  void install();
  void clear_build();
  void install_enqueued(Ctx& c);
  void finish_now(Ctx& c);
  void discard();
};

// The base arrays one plan will be multiplied with (a proof's At / BACGamma / BACDelta / BACGamma2 over w; one array for an MSM).
struct TableRef { BaseTable* t; const uint32_t* row0; size_t n; bool g2; };
// a resident base array's table (created on first use) and its reference
inline BaseTable& table_of(Bases& b) {
  if (!b.table) b.table = std::make_shared<BaseTable>();
  return *b.table;
}
inline TableRef table_ref(Bases& b) { return TableRef{&table_of(b), b.buf.as<uint32_t>(), b.n, b.kind == Kind::G2Bases}; }

// Decides how the group is summed THIS time and prepares it: true = window tables, all of width *cbits and resident (built now
// under policy `always`, or found); false = table-free with *cbits from choose_window_bits_free.  Under policy `auto` an array that
// has been used twice gets its table IN INSTALMENTS: every call enqueues, in front of its own accumulations, as many slabs of the
// pending table as `*credit` pays for (in G1-point builds; a G2 point costs kG2BuildCost of them; the caller grants ~0.055 points per
// (job-unit x term) of its own work, i.e. a proof pays ~60 % of its own table-free time on top) and takes what it spent off
// *credit.  Stamps the tables for the LRU.
constexpr double kG2BuildCost = 2.3;              // a G2 row costs 2.3 G1 rows (40 vs 17.5 ms per 2^20 points)
constexpr double kBuildCreditPerUnitTerm = 0.055; // 17.5 ms per 2^20 G1 points built (Jacobian doublings) / 1.5 ms per 2^20 (job-unit x term) summed table-free: 0.055 -> +60 % (6.5 ms per 2^20 proof)
// The credit a call of `units` job-units (a G1 sum = 1, a G2 sum = 2.76) over n terms grants itself; never less than 2^18 G1 points
// (~5 ms of building): the tables of a 2^16 key cost 9 ms in all while its table-free proofs take 5.5 ms instead of 2, so small keys are
// warm after two or three calls instead of sixteen.
inline double build_credit(double units, size_t n) { return std::max(kBuildCreditPerUnitTerm * units * (double)n, (double)((size_t)1 << 18)); }
bool prepare_tables(Ctx& c, const std::vector<TableRef>& group, uint32_t nterms, int* cbits, double* credit = nullptr);
// the tables one call will use, stamped for the LRU BEFORE any of them is built: an allocation made while the first group's tables are
// built must not evict the second group's (prepare_tables only stamped the group it was called for)
void stamp_tables(Ctx& c, const std::vector<BaseTable*>& tables);

}  // namespace gs
