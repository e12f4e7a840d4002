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
#include "agg_common.h"
#include "launch.h"

namespace phip {

typedef const PHIP_CAS DevDistinctQuery cdst_t;

constexpr int kDstBlock = 256;
constexpr int kDstWaves = kDstBlock / kWave;

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
    for (int32_t i = threadIdx.x; i < row_words; i += kDstBlock) {
      const uint32_t v = dst_lds[i];
      if (v) (void)__hip_atomic_fetch_or((glb_u32 *)(q.bitmap + i), v, PHIP_RLX, PHIP_AG);
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
      const int64_t off = q.slot_off[s], n = ((int64_t)q.slot_card[s] + 31) >> 5;
      uint32_t cnt = 0;
      for (int64_t i = lane; i < n; i += kWave) {
        const uint32_t v = ok ? row[off + i] : 0u;
        dst[off + i] = v;
        cnt += (uint32_t)__popc(v);
      }
      cnt = wave_sum_u32(cnt);
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
