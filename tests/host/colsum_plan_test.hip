// Host check of the column sums' index arithmetic (colsum_plan.h), compiled for the CPU: the levels of the segmented reduction are run
// with cs_reduce_chunk itself -- the loop the kernels run -- over integer "points" (a count and a sum of term numbers):
//   every entry of every level is added exactly once, every slot of the next level is written exactly once and the list stays sorted;
//   every non-empty column is handed out exactly once, with all of its terms (heads and tails meet), and no empty column ever is;
//   the chunk arithmetic partitions a list; the coefficient classes and magnitudes are what the header says.
#include <cstdio>
#include <cstdint>
#include <vector>
#include "../../go-snark-study_amd/csrc/colsum_plan.h"
using namespace gs;

struct Val { uint64_t cnt = 0, sum = 0; };

struct Sink {
  const std::vector<Val>* in;
  std::vector<int>* covered;
  std::vector<Val>* result;
  std::vector<int>* handed;
  std::vector<uint32_t>* nkeys;
  std::vector<Val>* nvals;
  std::vector<int>* written;
  Val acc;
  bool fail = false;
  void begin() { acc = Val(); }
  void add(uint32_t i) { (*covered)[i] += 1; acc.cnt += (*in)[i].cnt; acc.sum += (*in)[i].sum; }
  void out(uint32_t key) { (*handed)[key] += 1; (*result)[key] = acc; }
  void put(uint32_t slot, uint32_t key, Val v) {
    if (slot >= nkeys->size()) { fail = true; return; }
    (*written)[slot] += 1; (*nkeys)[slot] = key; (*nvals)[slot] = v;
  }
  void partial(uint32_t slot, uint32_t key) { put(slot, key, acc); }
  void empty(uint32_t slot, uint32_t key) { put(slot, key, Val()); }
};

// the columns' lengths -> 0 when every check holds
static int run(const std::vector<uint32_t>& lens, long& levels) {
  const uint32_t ncols = (uint32_t)lens.size();
  std::vector<uint32_t> keys;
  std::vector<Val> vals, want(ncols), result(ncols);
  for (uint32_t s = 0; s < ncols; ++s)
    for (uint32_t j = 0; j < lens[s]; ++j) {
      Val v; v.cnt = 1; v.sum = keys.size() + 1;
      want[s].cnt += 1; want[s].sum += v.sum;
      keys.push_back(s); vals.push_back(v);
    }
  std::vector<int> handed(ncols, 0);
  if (cs_chunks(0) != 0) return 1;
  while (!keys.empty()) {
    const uint32_t n = (uint32_t)keys.size(), nch = cs_chunks(n);
    // the chunks partition [0, n) and cs_chunk_of inverts them
    uint32_t at = 0;
    for (uint32_t c = 0; c < nch; ++c) {
      if (cs_chunk_begin(c) != at || cs_chunk_end(c, n) <= at || cs_chunk_end(c, n) - at > kCsChunk) return 2;
      for (uint32_t i = at; i < cs_chunk_end(c, n); ++i) if (cs_chunk_of(i) != c) return 3;
      at = cs_chunk_end(c, n);
    }
    if (at != n) return 4;
    const bool last = cs_last_level(n);
    if (last != (nch == 1)) return 5;
    const uint32_t nn = last ? 0 : cs_next_len(n);
    if (!last && nn >= n) return 6;
    std::vector<int> covered(n, 0), written(nn, 0);
    std::vector<uint32_t> nkeys(nn);
    std::vector<Val> nvals(nn);
    for (uint32_t c = 0; c < nch + 2; ++c) {                // two threads past the end, as a rounded-up grid has: they do nothing
      Sink s;
      s.in = &vals; s.covered = &covered; s.result = &result; s.handed = &handed; s.nkeys = &nkeys; s.nvals = &nvals; s.written = &written;
      cs_reduce_chunk(keys.data(), n, c, s);
      if (s.fail) return 7;
    }
    for (int v : covered) if (v != 1) return 8;
    for (int v : written) if (v != 1) return 9;
    for (uint32_t i = 1; i < nn; ++i) if (nkeys[i - 1] > nkeys[i]) return 10;
    keys.swap(nkeys); vals.swap(nvals);
    ++levels;
  }
  for (uint32_t s = 0; s < ncols; ++s) {
    if (handed[s] != (lens[s] ? 1 : 0)) return 11;
    if (lens[s] && (result[s].cnt != want[s].cnt || result[s].sum != want[s].sum)) return 12;
  }
  return 0;
}

static void words_of(const unsigned __int128 hi, const unsigned __int128 lo, uint32_t (&w)[8]) {
  for (int i = 0; i < 4; ++i) { w[i] = (uint32_t)(lo >> (32 * i)); w[4 + i] = (uint32_t)(hi >> (32 * i)); }
}

int main() {
  const uint32_t C = kCsChunk;
  long profiles = 0, levels = 0;
  const std::vector<uint32_t> base = {0, 1, C - 1, C, C + 1, 3 * C + 1};
  std::vector<std::vector<uint32_t>> all;
  for (size_t rot = 0; rot < base.size(); ++rot) {           // the same lengths at every offset against the chunk grid
    std::vector<uint32_t> p;
    for (size_t i = 0; i < base.size(); ++i) p.push_back(base[(i + rot) % base.size()]);
    all.push_back(p);
    std::vector<uint32_t> twice = p;
    twice.insert(twice.end(), p.begin(), p.end());
    all.push_back(twice);
  }
  for (uint32_t n : {1u, C, C + 1, 2 * C, 5000u, 1u << 16, (1u << 16) + 1u}) {
    all.push_back({n});                                       // one column holds every term
    all.push_back({0, 0, n, 0});
    all.push_back({1, n, 1});
    all.push_back(std::vector<uint32_t>(n, 1));               // every column one term
    all.push_back(std::vector<uint32_t>(n, 3));
  }
  all.push_back({});                                          // no columns
  all.push_back(std::vector<uint32_t>(100, 0));               // all columns empty
  for (const auto& p : all) {
    const int rc = run(p, levels);
    if (rc) { printf("FAIL check %d on profile %ld (%zu columns)\n", rc, profiles, p.size()); return 1; }
    ++profiles;
  }
  // coefficients: r = ModR's prime as 8 words
  uint32_t r[8];
  for (int i = 0; i < 8; ++i) r[i] = ModR::p32(i);
  auto sub_from_r = [&](uint32_t small, uint32_t (&w)[8]) {   // r - small
    uint64_t borrow = small;
    for (int i = 0; i < 8; ++i) { const uint64_t d = (uint64_t)r[i] - borrow; w[i] = (uint32_t)d; borrow = (d >> 32) & 1u; }
  };
  struct Case { uint32_t w[8]; uint32_t cls; bool neg; int bits; uint32_t mag0; };
  std::vector<Case> cases;
  auto push_small = [&](uint32_t v, bool from_r, uint32_t cls, int bits) {
    Case c{};
    if (from_r) sub_from_r(v, c.w); else c.w[0] = v;
    c.cls = cls; c.neg = from_r; c.bits = bits; c.mag0 = v;
    cases.push_back(c);
  };
  push_small(0, false, kCsZero, 0);
  push_small(1, false, kCsUnit, 1);
  push_small(1, true, kCsUnit, 1);
  push_small(2, false, kCsShort, 2);
  push_small(2, true, kCsShort, 2);
  push_small(65535, false, kCsShort, 16);
  push_small(65535, true, kCsShort, 16);
  push_small(0xffffffffu, false, kCsShort, 32);
  push_small(0xffffffffu, true, kCsShort, 32);
  { Case c{}; words_of(1, 0, c.w); c.cls = kCsLong; c.neg = false; c.bits = 129; c.mag0 = 0; cases.push_back(c); }           // 2^128
  { Case c{}; c.w[1] = 1; c.cls = kCsLong; c.neg = false; c.bits = 33; c.mag0 = 0; cases.push_back(c); }                      // 2^32
  { Case c{}; for (int i = 0; i < 8; ++i) c.w[i] = r[i]; c.cls = kCsZero; c.neg = false; c.bits = 0; c.mag0 = 0; cases.push_back(c); }   // r
  { Case c{}; for (int i = 0; i < 8; ++i) c.w[i] = r[i]; c.w[0] += 1; c.cls = kCsUnit; c.neg = false; c.bits = 1; c.mag0 = 1; cases.push_back(c); }   // r + 1
  long coefs = 0;
  for (const Case& c : cases) {
    uint32_t mag[8];
    bool neg;
    int bits;
    const uint32_t cls = cs_classify(c.w, mag, neg, bits);
    if (cls != c.cls || bits != c.bits || (cls != kCsZero && (neg != c.neg || mag[0] != c.mag0))) {
      printf("FAIL coefficient %ld: class %u (want %u), bits %d (want %d), neg %d, mag0 %u\n", coefs, cls, c.cls, bits, c.bits, (int)neg, mag[0]);
      return 1;
    }
    ++coefs;
  }
  // 2^256 - 1 = 5 r + rest: the magnitude is rest or r - rest, whichever is shorter, and below r
  {
    uint32_t w[8], mag[8];
    for (int i = 0; i < 8; ++i) w[i] = 0xffffffffu;
    bool neg;
    int bits;
    const uint32_t cls = cs_classify(w, mag, neg, bits);
    // rebuild the value: (neg ? r - mag : mag) + 5 r == 2^256 - 1
    unsigned __int128 carry = 0;
    uint32_t v[8];
    uint64_t borrow = 0;
    for (int i = 0; i < 8; ++i) {
      if (neg) { const uint64_t d = (uint64_t)r[i] - mag[i] - borrow; v[i] = (uint32_t)d; borrow = (d >> 32) & 1u; }
      else v[i] = mag[i];
    }
    bool ok = cls == kCsLong && bits == cs_bitlen(mag);
    for (int i = 0; i < 8; ++i) {
      carry += (unsigned __int128)v[i] + (unsigned __int128)5 * r[i];
      ok = ok && (uint32_t)carry == 0xffffffffu;
      carry >>= 32;
    }
    if (!ok || carry != 0) { printf("FAIL coefficient 2^256 - 1\n"); return 1; }
    ++coefs;
  }
  printf("OK %ld profiles, %ld levels, %ld coefficients, chunk %u\n", profiles, levels, coefs, C);
  return 0;
}
