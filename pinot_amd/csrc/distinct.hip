// distinct.hip -- exact DISTINCTCOUNT as bitmaps of query-global dictionary ids.
//
// DistinctCountAggregationFunction (pinot-core/.../query/aggregation/function/DistinctCountAggregationFunction.java)
// over BaseDistinctAggregateAggregationFunction (…/BaseDistinctAggregateAggregationFunction.java:131-160 aggregate,
// :306-330 aggregateGroupBySV) keeps, for a dictionary-encoded column, a bitmap of the segment's dictionary ids per
// group; :671-690 turns it into a value set when the segment's result is extracted and :760-800 merges two segments'
// sets by union. On the GPU the ids are mapped through the query-global dictionary first (DevCol.remap, the sorted union
// of the segments' dictionaries), so ONE bitmap per (group, distinct slot) is already the union over every segment of
// the query: no value is gathered, the pass reads ids only -- for STRING columns too.
//
// A pass of its own after the filter kernel (and the aggregation / group-by launch that handles the query's other
// functions and group presence), over the filter's lane-major tile masks, as select.hip is:
//   1. distinct_mark_kernel    per matched doc and slot: bit `global id` of row `dense group key` (row 0 without a
//                              group-by). Two regimes, chosen by the host per plan (DevDistinctQuery.lds):
//        lds = 1  no group-by and all slots' words fit PHIP_DISTINCT_LDS_WORDS: every workgroup ORs into its own
//                 zeroed LDS copy (ds_or, no return value) and issues one global atomic OR per NON-ZERO word at its
//                 end -- combine on chip, then one global atomic per destination word per workgroup;
//        lds = 0  global bitmap, test before set (see mark_global);
//   2. distinct_finish_kernel  for the groups the result returns: popcount of every slot's words -> the count, and the
//                              rows gathered back to back (phip_result.distinct_words).
// Integer OR is order-free, so the bitmaps are bit-reproducible whatever the schedule.
//
// Value counts (PHIP_AGG_VALUE_COUNTS, the multiset behind PERCENTILE and MODE: PercentileAggregationFunction.java:
// 77-100 collects every value, ModeAggregationFunction.java:81-155 a value -> count map) are the same pass with a u32
// COUNT per (group, global id) where DISTINCTCOUNT keeps a bit: a counts slot is card_s words of the row, word gid = the
// matched docs whose id is gid. lds = 1 adds 1 in LDS (no return value) and flushes each non-zero word with one global
// atomic ADD; lds = 0 is one global atomic add per doc (test-before-set does not apply to a count). Bits and counts
// slots share a row; the kind is per slot (DevDistinctQuery.slot_kind), so a branch on it is wave-uniform. Integer adds
// are order-free too. The finish kernel returns the 64-bit sum of a counts slot's words (= the docs aggregated).
#include "agg_common.h"
#include "launch.h"

namespace phip {

typedef const PHIP_CAS DevDistinctQuery cdst_t;

constexpr int kDstBlock = 256;
constexpr int kDstWaves = kDstBlock / kWave;

// u32 words of slot s inside a row: a bit per global id, or a count per global id
__device__ __forceinline__ int32_t slot_words(cdst_t &q, int s) {
  return q.slot_kind[s] == PHIP_DISTINCT_SLOT_COUNTS ? q.slot_card[s] : (q.slot_card[s] + 31) >> 5;
}

// Dense group key of one doc, by the dense group-by's rule for dictionary keys (agg_common.h group_key): mixed radix
// over query-global ids, column 0 least significant = the group's index in gb_table. Raw keys, doc-order key ids and
// null keys never reach this pass (the host refuses them beside a DISTINCTCOUNT), so group_key's other branches are
// not repeated here.
__device__ __forceinline__ int64_t distinct_key(cdst_t &q, cseg_t &seg, int32_t doc) {
  int64_t key = 0;
  for (int k = 0; k < q.num_group_by; k++) {
    ccol_t &c = seg.cols[q.gb_cols[k]];
    const uint32_t id = col_dict_id(c, doc);
    const int64_t gid = c.remap ? ((const PHIP_GLB int32_t *)c.remap)[id] : (int32_t)id;
    key += gid * q.gb_stride[k];
  }
  return key;
}

// Global regime: test before set. Within one execution a bit only ever goes 0 -> 1 (the bitmap is cleared by a memset
// that precedes the launch on the stream, and nothing clears a bit while the kernel runs), so a relaxed load that sees
// the bit set is final and the atomic can be skipped; a stale load that still sees 0 only costs a redundant atomic OR,
// which is idempotent. No bit can be lost either way. Hot ids (few distinct values, many docs) then cost one cached
// load per doc instead of one memory-side atomic.
__device__ __forceinline__ void mark_global(uint32_t *word, uint32_t bit) {
  glb_u32 *p = (glb_u32 *)word;
  if (__hip_atomic_load(p, PHIP_RLX, PHIP_AG) & bit) return;
  (void)__hip_atomic_fetch_or(p, bit, PHIP_RLX, PHIP_AG);
}

template <bool kLds>
__global__ __launch_bounds__(kDstBlock) void distinct_mark_kernel(const DevDistinctQuery *qp) {
  extern __shared__ uint32_t dst_lds[];  // kLds: row_words words, this workgroup's copy of the one row
  cdst_t &q = *(cdst_t *)qp;
  cseg_t *segs = (cseg_t *)q.segs;
  const int lane = lane_id();
  const int wave = uniform(threadIdx.x >> 6);
  const int32_t row_words = (int32_t)q.row_words;  // (kLds: at most the LDS budget)
  if (kLds) {
    for (int32_t i = threadIdx.x; i < row_words; i += kDstBlock) dst_lds[i] = 0u;
    __syncthreads();
  }
  const int64_t nw = (int64_t)gridDim.x * kDstWaves, w = (int64_t)blockIdx.x * kDstWaves + wave;
  const int b = (int)((int64_t)q.total_work * w / nw), e = (int)((int64_t)q.total_work * (w + 1) / nw);
  int si = 0;
  for (int t = b; t < e; t++) {
    while (si + 1 < q.num_segs && segs[si + 1].work_begin <= t) si++;
    cseg_t &seg = segs[si];
    const int32_t doc0 = (seg.tile0 + (t - seg.work_begin)) * kTileDocs;
    const uint32_t valid = valid_word(min(kTileDocs, seg.num_docs - doc0), lane);
    const uint32_t m =
        q.mask != nullptr ? (((const PHIP_GLB uint32_t *)q.mask)[(size_t)t * 64 + lane] & valid) : valid;
    // bit 31-g of lane l = doc 64 g + l: the wave takes the tile's 64-doc groups one at a time, so consecutive lanes
    // decode consecutive docs' ids (neighbouring bits of the same few words); a group no lane matched is skipped
    uint32_t any = wave_or32(m);
    while (any) {
      const int g = __builtin_clz(any);
      any &= ~(0x80000000u >> g);
      if (!((m << g) & 0x80000000u)) continue;
      const int32_t doc = doc0 + 64 * g + lane;
      const int64_t key = q.num_group_by > 0 ? distinct_key(q, seg, doc) : 0;
      if (key < 0 || key >= q.num_rows) continue;  // (ids are below the cardinalities: a guard, never taken)
      for (int s = 0; s < q.num_slots; s++) {
        ccol_t &c = seg.cols[q.slot_col[s]];
        const uint32_t id = col_dict_id(c, doc);
        const uint32_t gid = c.remap ? (uint32_t)((const PHIP_GLB int32_t *)c.remap)[id] : id;
        if (gid >= (uint32_t)q.slot_card[s]) continue;  // (guard, as above)
        if (q.slot_kind[s] == PHIP_DISTINCT_SLOT_COUNTS) {  // (wave-uniform: the slot's kind)
          // word `gid` of the slot counts the docs. In LDS a plain add per lane (ds_add, no return value) is the fastest
          // form measured, whatever the skew. A global row of a small dictionary puts many of the wave's lanes on one
          // word, and same-address atomics serialise at the L2: there the lanes that share a word are peeled off
          // together (the first active lane's word broadcast, its holders balloted) and ONE of them adds their number.
          // At most combine_rounds rounds; lanes still left (many rows x ids in one wave) add 1 each.
          const uint64_t w = (kLds ? 0ull : (uint64_t)key * (uint64_t)q.row_words) + (uint64_t)q.slot_off[s] + gid;
          uint32_t add = 1u;
          if (!kLds && q.slot_card[s] <= q.combine_card) {
            bool pending = true;
            for (int r = 0; r < q.combine_rounds && pending; r++) {
              const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w);
              const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w >> 32));
              const bool mine = w == (((uint64_t)hi << 32) | lo);
              const uint64_t same = ballot(mine);  // (of the lanes still pending: the holders of this word)
              if (mine) {
                add = mbcnt64(same) == 0 ? (uint32_t)__popcll(same) : 0u;
                pending = false;
              }
            }
          }
          if (add) {
            if (kLds) (void)__hip_atomic_fetch_add((lds_u32 *)&dst_lds[w], add, PHIP_RLX, PHIP_WG);
            else (void)__hip_atomic_fetch_add((glb_u32 *)(q.bitmap + w), add, PHIP_RLX, PHIP_AG);
          }
          continue;
        }
        const uint32_t bit = 1u << (gid & 31);
        if (kLds) {
          (void)__hip_atomic_fetch_or((lds_u32 *)&dst_lds[q.slot_off[s] + (gid >> 5)], bit, PHIP_RLX, PHIP_WG);
        } else {
          mark_global(q.bitmap + (size_t)key * (size_t)q.row_words + (size_t)q.slot_off[s] + (gid >> 5), bit);
        }
      }
    }
  }
  if (kLds) {
    __syncthreads();
    for (int s = 0; s < q.num_slots; s++) {
      const bool counts = q.slot_kind[s] == PHIP_DISTINCT_SLOT_COUNTS;
      const int32_t off = (int32_t)q.slot_off[s], n = slot_words(q, s);
      for (int32_t i = threadIdx.x; i < n; i += kDstBlock) {
        const uint32_t v = dst_lds[off + i];
        if (!v) continue;
        if (counts) (void)__hip_atomic_fetch_add((glb_u32 *)(q.bitmap + off + i), v, PHIP_RLX, PHIP_AG);
        else (void)__hip_atomic_fetch_or((glb_u32 *)(q.bitmap + off + i), v, PHIP_RLX, PHIP_AG);
      }
    }
  }
}

// One wave per returned group: keys[g] = the group's row in the bitmap (null keys: row g). counts[g * num_slots + s] =
// set bits of slot s; out[g * row_words ..] = the row.
__global__ __launch_bounds__(kDstBlock) void distinct_finish_kernel(const DevDistinctQuery *qp, const int64_t *keys,
                                                                    int64_t num_out, int64_t *__restrict__ counts,
                                                                    uint32_t *__restrict__ out) {
  cdst_t &q = *(cdst_t *)qp;
  const int lane = lane_id();
  const int64_t nw = (int64_t)gridDim.x * kDstWaves;
  for (int64_t g = (int64_t)blockIdx.x * kDstWaves + (threadIdx.x >> 6); g < num_out; g += nw) {
    const int64_t key = keys != nullptr ? keys[g] : g;
    const bool ok = key >= 0 && key < q.num_rows;
    const uint32_t *row = q.bitmap + (size_t)(ok ? key : 0) * (size_t)q.row_words;
    uint32_t *dst = out + (size_t)g * (size_t)q.row_words;
    for (int s = 0; s < q.num_slots; s++) {
      const int64_t off = q.slot_off[s], n = slot_words(q, s);
      const bool counts_slot = q.slot_kind[s] == PHIP_DISTINCT_SLOT_COUNTS;
      uint64_t cnt = 0;  // bits: the set bits; counts: the sum of the words = the docs aggregated
      for (int64_t i = lane; i < n; i += kWave) {
        const uint32_t v = ok ? row[off + i] : 0u;
        dst[off + i] = v;
        cnt += counts_slot ? v : (uint32_t)__popc(v);
      }
      for (int o = 32; o > 0; o >>= 1) cnt += (uint64_t)__shfl_xor((long long)cnt, o);
      if (lane == 0) counts[g * q.num_slots + s] = (int64_t)cnt;
    }
  }
}

// ---- host-callable launchers (launch.h) -------------------------------------------------------------------------
hipError_t launch_distinct_mark(const DevDistinctQuery *q, int64_t total_work, int lds, size_t lds_bytes, int max_blocks,
                                hipStream_t s) {
  if (total_work <= 0) return hipSuccess;
  int64_t blocks = (total_work + kDstWaves - 1) / kDstWaves;
  blocks = blocks < 1 ? 1 : (blocks > max_blocks ? max_blocks : blocks);
  if (lds) distinct_mark_kernel<true><<<(int)blocks, kDstBlock, lds_bytes, s>>>(q);
  else distinct_mark_kernel<false><<<(int)blocks, kDstBlock, 0, s>>>(q);
  return hipGetLastError();
}

hipError_t launch_distinct_finish(const DevDistinctQuery *q, const int64_t *keys, int64_t num_out, int64_t *counts,
                                  uint32_t *out, hipStream_t s) {
  if (num_out <= 0) return hipSuccess;
  const int64_t blocks = std::min<int64_t>(4096, (num_out + kDstWaves - 1) / kDstWaves);
  distinct_finish_kernel<<<(int)blocks, kDstBlock, 0, s>>>(q, keys, num_out, counts, out);
  return hipGetLastError();
}

}  // namespace phip
