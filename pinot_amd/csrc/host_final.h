// host_final.h -- the record mode of aggregation-only plans: every filter workgroup stores ONE tagged record of its
// partials into mapped host memory at its very end, and the host accepts the records and reduces them in the fixed
// order finalize_all_kernel used (aggregate.hip finalize_slot), so the plan needs no finalize launch, no ticket and no
// fence. This header holds the encoding, the plan-time block table and the host's accept-and-reduce code. No HIP
// dependency (tests build it into a stand-alone program).
//
// Encoding. Every 8-byte word of a record is tag << 48 | field, stored by one relaxed 8-byte store, so a word is valid
// for execution T exactly when its tag is T: a plan serialises its executions and every execution rewrites every
// expected word, so a word carries T, T - 1 or 0 (the area starts zero-filled and no execution has tag 0). A count is
// one word (48-bit field); a 64-bit accumulator is two words, its low 48 and its high 16 bits. A record is, in order:
// matched docs | entries scanned | the block's aggregation partials (two words each) | the matched count of each
// work-list segment entry the block's tile range touches (entry first + j at word j of that part).
#pragma once
#include <stdint.h>

#include <vector>

#include "acc_ops.h"
#include "tile_range.h"

namespace phip {

constexpr int kRecMaxWords = 16;  // a record is 64 B (<= 8 words) or 128 B, aligned to its size
constexpr int kRecSegSlots = 14;  // segment entries a block may touch: kRecMaxWords - 2 without aggregations
constexpr uint64_t kRecFieldMask = (1ull << 48) - 1;

PHIP_HD inline uint64_t rec_word(uint32_t tag, uint64_t field) { return ((uint64_t)tag << 48) | (field & kRecFieldMask); }
PHIP_HD inline uint32_t rec_tag_of(uint64_t word) { return (uint32_t)(word >> 48); }
PHIP_HD inline int rec_num_words(int na, int k) { return 2 + 2 * na + k; }
// the tag after `tag` (16 bits, never 0)
inline uint32_t rec_next_tag(uint32_t tag) {
  const uint32_t t = (tag + 1) & 0xffffu;
  return t == 0 ? 1u : t;
}

// The plan-time table: per block its tile range, the first work-list entry of that range and the number of entries
// it touches. entry_begin[e] = the first tile of entry e (ascending; the kernel's rule: a tile belongs to the LAST
// entry whose first tile is <= it).
struct RecBlocks {
  std::vector<int32_t> begin, end, first, k;
  int max_k = 0;
};

inline int rec_entry_of(const std::vector<int32_t> &entry_begin, int tile) {
  int e = 0;
  const int n = (int)entry_begin.size();
  while (e + 1 < n && entry_begin[e + 1] <= tile) e++;
  return e;
}

inline RecBlocks rec_block_table(int xcd_walk, int total_work, int nblocks, int nwaves,
                                 const std::vector<int32_t> &entry_begin) {
  RecBlocks t;
  t.begin.resize(nblocks);
  t.end.resize(nblocks);
  t.first.resize(nblocks);
  t.k.resize(nblocks);
  for (int b = 0; b < nblocks; b++) {
    const TileRange r = block_tile_range(xcd_walk, total_work, nblocks, b, nwaves);
    t.begin[b] = r.begin;
    t.end[b] = r.end;
    t.first[b] = 0;
    t.k[b] = 0;
    if (r.begin < r.end) {
      t.first[b] = rec_entry_of(entry_begin, r.begin);
      t.k[b] = rec_entry_of(entry_begin, r.end - 1) - t.first[b] + 1;
    }
    if (t.k[b] > t.max_k) t.max_k = t.k[b];
  }
  return t;
}

// What the host reads of one plan's record area.
struct RecPlan {
  int nblocks = 0;
  int na = 0;                // aggregation partials per record
  int stride_words = 8;      // 8 or 16
  const int32_t *kinds = nullptr;       // [na] AccKind
  const int32_t *first = nullptr;       // [nblocks]
  const int32_t *k = nullptr;           // [nblocks]
  const int32_t *entry_slot = nullptr;  // [entries] -> slot of the per-segment matched counts
};

// All expected words of block b carry `tag`?
inline bool rec_block_ready(const RecPlan &p, const volatile uint64_t *area, int b, uint32_t tag) {
  const volatile uint64_t *r = area + (size_t)b * p.stride_words;
  const int n = rec_num_words(p.na, p.k[b]);
  for (int i = 0; i < n; i++)
    if (rec_tag_of(r[i]) != tag) return false;
  return true;
}

// Advances *cursor over the blocks whose records are complete; true when every block is.
inline bool rec_accept(const RecPlan &p, const volatile uint64_t *area, uint32_t tag, int *cursor) {
  while (*cursor < p.nblocks && rec_block_ready(p, area, *cursor, tag)) (*cursor)++;
  return *cursor == p.nblocks;
}

inline uint64_t rec_acc(const uint64_t *r, int a) {
  return (r[2 + 2 * a] & kRecFieldMask) | ((r[3 + 2 * a] & 0xffffull) << 48);
}

// finalize_slot's order: lane b % 64 combines blocks b, b + 64, ... starting from the kind's identity, then the
// butterfly of wave_reduce_f64 as lane 0 sees it (offsets 32, 16, ... 1; lane i takes lane i ^ offset as its second
// operand). Integer kinds wrap mod 2^64 in any order.
inline uint64_t rec_reduce_slot(int kind, const uint64_t *vals, int n) {
  const bool fp = kind == ACC_SUM_F64 || kind == ACC_MIN_F64 || kind == ACC_MAX_F64;
  if (!fp) {
    uint64_t v = 0;
    for (int b = 0; b < n; b++) v += vals[b];
    return v;
  }
  uint64_t lane[64];
  for (int l = 0; l < 64; l++) {
    uint64_t v = acc_init(kind);
    for (int b = l; b < n; b += 64) v = acc_combine(kind, v, vals[b]);
    lane[l] = v;
  }
  for (int o = 32; o > 0; o >>= 1)
    for (int l = 0; l < o; l++) lane[l] = acc_combine(kind, lane[l], lane[l + o]);
  return lane[0];
}

// The reduction of accepted records (every expected word carries the execution's tag): out_aggs[na], matched docs,
// entries scanned, and the per-segment matched counts ADDED into segm (the caller zeroes it).
// scratch: nblocks words the caller keeps (a plan's executions allocate nothing).
inline void rec_reduce(const RecPlan &p, const uint64_t *area, uint64_t *out_aggs, uint64_t *matched, uint64_t *scanned,
                       uint64_t *segm, uint64_t *scratch) {
  uint64_t m = 0, s = 0;
  for (int b = 0; b < p.nblocks; b++) {
    const uint64_t *r = area + (size_t)b * p.stride_words;
    m += r[0] & kRecFieldMask;
    s += r[1] & kRecFieldMask;
    for (int j = 0; j < p.k[b]; j++) segm[p.entry_slot[p.first[b] + j]] += r[2 + 2 * p.na + j] & kRecFieldMask;
  }
  *matched = m;
  *scanned = s;
  for (int a = 0; a < p.na; a++) {
    for (int b = 0; b < p.nblocks; b++) scratch[b] = rec_acc(area + (size_t)b * p.stride_words, a);
    out_aggs[a] = rec_reduce_slot(p.kinds[a], scratch, p.nblocks);
  }
}

}  // namespace phip
