// select_common.h -- what the selection kernel units share (select.hip, select_order.hip): the walk's geometry, a
// work tile's matched docs and one select expression's value of a doc.
#pragma once
#include "agg_common.h"
#include "launch.h"

namespace phip {

typedef const PHIP_CAS DevSelQuery csel_t;

constexpr int kSelBlock = 256;
constexpr int kSelWaves = kSelBlock / kWave;

// Docs of work tile t that the filter kept (lane-major), and the entry it belongs to (si advanced monotonically).
__device__ __forceinline__ uint32_t sel_tile_mask(csel_t &q, cseg_t &seg, int t) {
  const int32_t doc0 = (seg.tile0 + (t - seg.work_begin)) * kTileDocs;
  const uint32_t valid = valid_word(min(kTileDocs, seg.num_docs - doc0), lane_id());
  return q.mask != nullptr ? (((const PHIP_GLB uint32_t *)q.mask)[(size_t)t * 64 + lane_id()] & valid) : valid;
}

__device__ __forceinline__ uint64_t sel_value(cseg_t &seg, const PHIP_CAS DevSelect &s, int32_t doc) {
  ccol_t &a = seg.cols[s.col_a];
  if (s.expr == PHIP_EXPR_COLUMN) {
    if (s.kind == SEL_ID) {
      const uint32_t id = col_dict_id(a, doc);
      return (uint64_t)(int64_t)(a.remap ? ((const PHIP_GLB int32_t *)a.remap)[id] : (int32_t)id);
    }
    if (s.kind == SEL_STR) return ((uint64_t)(uint32_t)seg.seg_index << 32) | (uint32_t)doc;
    if (s.kind == SEL_I64) return (uint64_t)col_i64(a, doc);
    return as_u64(col_f64(a, doc));
  }
  const double x = col_f64(a, doc), y = col_f64(seg.cols[s.col_b], doc);
  return as_u64(s.expr == PHIP_EXPR_ADD ? x + y : (s.expr == PHIP_EXPR_SUB ? x - y : x * y));
}

// Workgroups of a tile walk: one wave per tile until max_blocks caps them.
static inline int sel_blocks(int64_t total_work, int max_blocks) {
  const int64_t b = (total_work + kSelWaves - 1) / kSelWaves;
  return (int)(b < 1 ? 1 : (b > max_blocks ? max_blocks : b));
}

}  // namespace phip
