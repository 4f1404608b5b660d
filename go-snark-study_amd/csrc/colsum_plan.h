// The index arithmetic of the column sums of an R1CS over points (zkey_setup.hip, gs_r1cs_colsum_g1 / _g2), host and device.
//
// The terms of the matrices are sorted by signal into one list of ENTRIES (key = signal, entry = a signed reference to a point).  The
// sum of every run of equal keys is a segmented reduction; it is carried out in LEVELS so that no column is ever one thread's loop:
//   a level cuts its list of n entries into chunks of kCsChunk, one per thread;
//   a run that lies strictly inside a chunk (its key is neither the chunk's first nor its last key) is complete: its sum is the result;
//   the run of the first key (the HEAD) and the run of the last key (the TAIL) may go on in the neighbouring chunks: their sums become
//   entries 2c and 2c + 1 of the next level's list (a chunk whose keys are all equal has no tail: entry 2c + 1 is that key with the point
//   at infinity), which is sorted again because the chunks are taken in order;
//   a level of at most kCsChunk entries is the last: one thread, every run complete.
// A list of n entries becomes one of 2 ceil(n / kCsChunk): a column of 2^20 terms is summed in 7 levels of 16-term loops.
// cs_reduce_chunk is the loop of one thread; the kernels and tests/host/colsum_plan_test.hip instantiate it with their own sinks.
//
// An entry: bit 31 = subtract; bits 30..29 = the array the point lies in (0, 1, 2: the basis of A, B, C at the term's row; 3: the array of
// products of the general terms); bits 28..0 = the index in that array (a general term: bit 28 = the list of long ones, bits 27..0 = its
// number in its list; the products of the long list lie behind those of the short one).
// A coefficient v is classified by its value mod r (cs_classify): zero (no entry), +-1 (the basis point itself), and the general ones,
// which are multiplied through min(bitlen(v), bitlen(r - v)) bits in a dense kernel of their own -- in two lists, short (<= 32 bits: small
// constants and their negatives) and long, so that a wave of multiplications does not wait for one 254-bit scalar among 2-bit ones.
#pragma once
#include <stdint.h>

#include "fp29.h"

namespace gs {

constexpr uint32_t kCsChunk = 16;
constexpr uint32_t kCsSignBit = 0x80000000u;
constexpr int kCsSrcShift = 29;
constexpr uint32_t kCsIdxMask = (1u << kCsSrcShift) - 1u;
constexpr uint32_t kCsSrcGeneral = 3;
constexpr uint32_t kCsLongFlag = 1u << 28;                  // in the index of a general term: it is in the list of long ones
constexpr uint32_t kCsMaxEntries = kCsLongFlag;             // terms of one call (and rows of a basis)
constexpr int kCsShortBits = 32;

GS_HD uint32_t cs_chunks(uint32_t n) { return n / kCsChunk + (n % kCsChunk != 0u); }
GS_HD uint32_t cs_chunk_of(uint32_t i) { return i / kCsChunk; }
GS_HD uint32_t cs_chunk_begin(uint32_t c) { return c * kCsChunk; }
GS_HD uint32_t cs_chunk_end(uint32_t c, uint32_t n) { return n - c * kCsChunk < kCsChunk ? n : (c + 1u) * kCsChunk; }
GS_HD bool cs_last_level(uint32_t n) { return n <= kCsChunk; }
GS_HD uint32_t cs_next_len(uint32_t n) { return 2u * cs_chunks(n); }
GS_HD uint32_t cs_entry(bool negate, uint32_t src, uint32_t idx) { return (negate ? kCsSignBit : 0u) | (src << kCsSrcShift) | idx; }

// One thread of one level: chunk c of the n sorted keys.  Sink:
//   begin()                a run starts: the accumulator is the point at infinity
//   add(i)                 the accumulator takes entry i
//   out(key)               the run is complete: the accumulator is the sum of column `key`
//   partial(slot, key)     the run may go on next door: the accumulator is entry `slot` of the next level, under `key`
//   empty(slot, key)       entry `slot` of the next level is the point at infinity under `key`
// The loop is flat -- one add per iteration for every thread of a wave -- and only the hand-over of a finished run diverges.
template <class Sink>
GS_HD void cs_reduce_chunk(const uint32_t* keys, uint32_t n, uint32_t c, Sink& s) {
  if (c >= cs_chunks(n)) return;
  const uint32_t b = cs_chunk_begin(c), e = cs_chunk_end(c, n);
  const bool last = cs_last_level(n);
  const uint32_t kf = keys[b], kl = keys[e - 1];
  uint32_t prev = kf;
  s.begin();
  for (uint32_t i = b; i <= e; ++i) {
    const uint32_t k = i < e ? keys[i] : ~prev;            // one step past the end hands the last run over
    if (k != prev) {
      if (last || (prev != kf && prev != kl)) s.out(prev);
      else s.partial(2u * c + (prev == kf ? 0u : 1u), prev);
      if (i == e) break;
      s.begin();
      prev = k;
    }
    s.add(i);
  }
  if (!last && kf == kl) s.empty(2u * c + 1u, kl);
}

// ---- coefficients --------------------------------------------------------------------------------------------------------------
enum : uint32_t { kCsZero = 0, kCsUnit = 1, kCsShort = 2, kCsLong = 3 };

GS_HD int cs_bitlen(const uint32_t (&k)[8]) {
  for (int w = 7; w >= 0; --w)
    if (k[w]) return 32 * w + 32 - __builtin_clz(k[w]);
  return 0;
}
// any 256-bit value -> below r (2^256 < 6 r)
GS_HD void cs_canon(uint32_t (&k)[8]) {
  for (int it = 0; it < 5; ++it) {
    uint32_t t[8];
    uint64_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const uint64_t d = (uint64_t)k[i] - ModR::p32(i) - borrow;
      t[i] = (uint32_t)d;
      borrow = (d >> 32) & 1u;
    }
    const bool ge = borrow == 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) k[i] = ge ? t[i] : k[i];
  }
}
// v (any 256-bit value) -> its class; mag = min(v mod r, r - v mod r) by bit length, negate = the second was taken, bits = bitlen(mag)
GS_HD uint32_t cs_classify(const uint32_t (&v)[8], uint32_t (&mag)[8], bool& negate, int& bits) {
#pragma unroll
  for (int i = 0; i < 8; ++i) mag[i] = v[i];
  cs_canon(mag);
  negate = false;
  bits = cs_bitlen(mag);
  if (bits == 0) return kCsZero;
  uint32_t t[8];
  uint64_t borrow = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint64_t d = (uint64_t)ModR::p32(i) - mag[i] - borrow;
    t[i] = (uint32_t)d;
    borrow = (d >> 32) & 1u;
  }
  const int tb = cs_bitlen(t);
  if (tb < bits) {
    negate = true;
    bits = tb;
#pragma unroll
    for (int i = 0; i < 8; ++i) mag[i] = t[i];
  }
  return bits == 1 ? kCsUnit : bits <= kCsShortBits ? kCsShort : kCsLong;
}

}  // namespace gs
