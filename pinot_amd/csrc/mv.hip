// mv.hip -- multi-value columns (PHIP_FWD_FIXED_BIT_MV): the filter's MV scan leaf and the aggregations' row-reduction
// columns (device.h MvScanTask / MvReduceTask; runtime.cpp load_mv_forward, PlanBuilder::mv_leaf / stage_inverted_leaves,
// ensure_derived).
//
// Resident layout: the dict ids of all rows bit-packed back to back (a single-value fixed-bit column of total_values
// elements) plus num_docs + 1 u32 value offsets.
//
// mv_scan_kernel restates BaseDictionaryBasedPredicateEvaluator.applyMV (pinot-core/.../operator/filter/predicate/
// BaseDictionaryBasedPredicateEvaluator.java:164-180): a doc matches an inclusive predicate when ANY of its values'
// ids is in the matching range / set, an exclusive one (NOT_EQ, NOT_IN) when NONE is in the excluded set -- the
// complement, stored by `invert`. It writes the leaf's dense doc words, which the filter kernels then read as an
// inverted leaf's (PHIP_LEAF_INVERTED): no filter kernel knows of multi-value columns.
//
// Shape: one workgroup per 2048-doc tile, grid-strided. The tile's offsets are staged in LDS; its values are walked in
// passes of kMvPassValues consecutive elements. Per pass the row starts are marked in an LDS bitset (one u64 word per
// 64-element group, one group per wave step) and the words' popcounts prefix-summed, so an element finds its doc
// without a search: the starts before its group (s_base) plus the rank of the starts up to its lane inside the group.
// Lanes take consecutive elements -- a wave's loads cover whole lines of the packed ids; kMvBatch groups' loads are
// issued before the first is tested --, decode with the window
// decode of the single-value scans, test the range or the id bitmap (in LDS up to kMvSetLdsWords words), and OR their
// hit into the tile's 32 u64 doc words in LDS; the words are stored once, with no global atomic. A row of any length
// works: it spans groups, passes (its later elements rank 0 and land on the last doc started before them) and, as the
// last row of a tile, any number of values.
#include "agg_common.h"
#include "launch.h"

namespace phip {

constexpr int kMvBlock = 256;
constexpr int kMvWaves = kMvBlock / 64;
constexpr int kMvPassValues = 64 * kMvBlock;  // one start-bit word per thread
constexpr int kMvBatch = 8;                   // 64-element groups a wave loads before it tests them
constexpr int kMvSetLdsWords = 2048;          // id bitmaps of dictionaries up to 65536 entries sit in LDS

typedef const PHIP_CAS MvScanTask cmvscan_t;

__global__ __launch_bounds__(kMvBlock) void mv_scan_kernel(const MvScanTask *tasks, int32_t ntasks, int32_t total_tiles) {
  __shared__ uint32_t s_off[kTileDocs + 1];
  __shared__ unsigned long long s_start[kMvBlock];
  __shared__ uint32_t s_base[kMvBlock];
  __shared__ uint32_t s_hit[kTileDocs / 32];
  __shared__ uint32_t s_set[kMvSetLdsWords];
  __shared__ uint32_t s_wsum[kMvWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int staged_task = -1;
  for (int32_t w = blockIdx.x; w < total_tiles; w += gridDim.x) {
    int ti = 0;
    while (ti + 1 < ntasks && ((cmvscan_t *)tasks)[ti + 1].tile_begin <= w) ti++;
    cmvscan_t &t = ((cmvscan_t *)tasks)[ti];
    const int32_t tile = w - t.tile_begin;
    const int32_t d0 = tile * kTileDocs;
    const int32_t nd = min(kTileDocs, t.num_docs - d0);  // (<= 0: a padding tile past the segment's docs)
    const uint32_t *set = t.set;
    const bool set_lds = set != nullptr && t.set_words <= kMvSetLdsWords;
    __syncthreads();  // the previous tile's words are stored, its set no longer read
    if (tid < kTileDocs / 32) s_hit[tid] = 0;
    {  // the tile's nd + 1 offsets: a thread's eight loads issued together
      uint32_t o[kTileDocs / kMvBlock];
#pragma unroll
      for (int k = 0; k < kTileDocs / kMvBlock; k++) o[k] = tid + kMvBlock * k <= nd ? t.offsets[d0 + tid + kMvBlock * k] : 0u;
#pragma unroll
      for (int k = 0; k < kTileDocs / kMvBlock; k++) s_off[tid + kMvBlock * k] = o[k];
      if (tid == 0 && nd == kTileDocs) s_off[kTileDocs] = t.offsets[d0 + kTileDocs];
    }
    if (set_lds && staged_task != ti)
      for (int i = tid; i < t.set_words; i += kMvBlock) s_set[i] = set[i];
    staged_task = ti;
    __syncthreads();
    if (nd > 0) {
      const uint32_t v0 = s_off[0], v1 = s_off[nd];
      const uint32_t bits = (uint32_t)t.bits, lo = (uint32_t)t.lo, span = (uint32_t)(t.hi - t.lo);
      uint32_t doc_base = 0;  // docs of the tile that start before the pass
      for (uint32_t p0 = v0; p0 < v1; p0 += kMvPassValues) {
        const uint32_t len = min((uint32_t)kMvPassValues, v1 - p0);
        s_start[tid] = 0;
        __syncthreads();
        for (int i = tid; i < nd; i += kMvBlock) {
          const uint32_t o = s_off[i] - p0;  // (wraps above len for a start before the pass)
          if (o < len) atomicOr(&s_start[o >> 6], 1ull << (o & 63));
        }
        __syncthreads();
        const uint32_t c = (uint32_t)__popcll(s_start[tid]);
        const uint32_t incl = wave_incl_scan(c);
        if (lane == 63) s_wsum[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int k = 0; k < kMvWaves; k++) {
          before += k < wave ? s_wsum[k] : 0;
          total += s_wsum[k];
        }
        s_base[tid] = before + incl - c;
        __syncthreads();
        const uint32_t ngroups = (len + 63) >> 6;
        // kMvBatch groups per wave step: every lane's id windows are loaded first (kMvBatch loads in flight per lane --
        // with one or two the walk waits on HBM latency, not bandwidth), then tested. A lane past the pass's end
        // re-reads the last element (in bounds) and is masked out.
        for (uint32_t g0 = wave; g0 < ngroups; g0 += kMvWaves * kMvBatch) {
          uint32_t ids[kMvBatch];
#pragma unroll
          for (int k = 0; k < kMvBatch; k++) {
            const uint32_t idx = min(64 * (g0 + kMvWaves * k) + lane, len - 1);
            ids[k] = decode_bits(t.words, (uint64_t)(p0 + idx) * bits, bits);
          }
#pragma unroll
          for (int k = 0; k < kMvBatch; k++) {
            const uint32_t g = g0 + kMvWaves * k;
            const uint32_t id = ids[k];
            bool hit;
            if (set == nullptr) hit = id - lo < span;
            else if (set_lds) hit = (s_set[id >> 5] >> (id & 31)) & 1u;
            else hit = (set[id >> 5] >> (id & 31)) & 1u;
            if (hit && 64 * g + lane < len) {
              // the starts up to this lane, this one included: the element's doc is the last one started
              const uint32_t rank = (uint32_t)__popcll(s_start[g] & ((2ull << lane) - 1ull));
              const uint32_t dl = doc_base + s_base[g] + rank - 1u;
              atomicOr(&s_hit[dl >> 5], 1u << (dl & 31));
            }
          }
        }
        doc_base += total;
        __syncthreads();  // the pass's start bits and sums are read
      }
    }
    __syncthreads();
    if (tid < kTileDocs / 64) {
      uint64_t word = (uint64_t)s_hit[2 * tid] | ((uint64_t)s_hit[2 * tid + 1] << 32);
      const int64_t rem = (int64_t)t.num_docs - ((int64_t)d0 + 64 * tid);
      const uint64_t valid = rem >= 64 ? ~0ull : rem <= 0 ? 0ull : ((1ull << rem) - 1ull);
      if (t.invert) word = ~word;
      t.out[(int64_t)tile * t.tile_words + tid] = word & valid;
    }
  }
}

// Row reductions (include/pinot_hip.h PHIP_MV_REDUCE_*): doc-parallel, one 8-byte store per doc, the dictionary values
// gathered through the row's ids. The double SUM adds the row's values left to right (the inner loop of
// SumMVAggregationFunction.aggregate, pinot-core/.../query/aggregation/function/SumMVAggregationFunction.java); MIN /
// MAX fold the row with fmin / fmax from +/-inf (Math.min / Math.max over values that hold no NaN: the planner refuses
// those).
__device__ __forceinline__ int64_t mv_dict_i64(const void *dict, int32_t type, uint32_t id) {
  return type == PHIP_TYPE_INT ? (int64_t)((const int32_t *)dict)[id] : ((const int64_t *)dict)[id];
}
__device__ __forceinline__ double mv_dict_f64(const void *dict, int32_t type, uint32_t id) {
  switch (type) {
    case PHIP_TYPE_INT: return (double)((const int32_t *)dict)[id];
    case PHIP_TYPE_LONG: return (double)((const int64_t *)dict)[id];
    case PHIP_TYPE_FLOAT: return (double)((const float *)dict)[id];
    default: return ((const double *)dict)[id];
  }
}

__global__ __launch_bounds__(kMvBlock) void mv_reduce_kernel(const MvReduceTask t) {
#pragma clang fp contract(off)
  const int64_t d = (int64_t)blockIdx.x * kMvBlock + threadIdx.x;
  if (d >= t.num_docs) return;
  const uint32_t o0 = t.offsets[d], o1 = t.offsets[d + 1];
  const uint32_t bits = (uint32_t)t.bits;
  if (t.kind == PHIP_MV_REDUCE_LENGTH) {
    if (t.integral) ((int64_t *)t.out)[d] = (int64_t)(o1 - o0);
    else ((double *)t.out)[d] = (double)(o1 - o0);
  } else if (t.kind == PHIP_MV_REDUCE_SUM && t.integral) {
    uint64_t s = 0;  // (unsigned: wrapping is defined; the host's bound keeps the row sum inside int64)
    for (uint32_t e = o0; e < o1; e++) s += (uint64_t)mv_dict_i64(t.dict, t.type, decode_bits(t.words, (uint64_t)e * bits, bits));
    ((int64_t *)t.out)[d] = (int64_t)s;
  } else if (t.kind == PHIP_MV_REDUCE_SUM) {
    double s = 0.0;
    for (uint32_t e = o0; e < o1; e++) s = __dadd_rn(s, mv_dict_f64(t.dict, t.type, decode_bits(t.words, (uint64_t)e * bits, bits)));
    ((double *)t.out)[d] = s;
  } else {
    const bool is_min = t.kind == PHIP_MV_REDUCE_MIN;
    double v = is_min ? __builtin_huge_val() : -__builtin_huge_val();
    for (uint32_t e = o0; e < o1; e++) {
      const double x = mv_dict_f64(t.dict, t.type, decode_bits(t.words, (uint64_t)e * bits, bits));
      v = is_min ? fmin(v, x) : fmax(v, x);
    }
    ((double *)t.out)[d] = v;
  }
}

static hipError_t launch_mv_scan(const MvScanTask *tasks, int32_t ntasks, int32_t total_tiles, int max_blocks,
                                 hipStream_t s) {
  if (ntasks <= 0 || total_tiles <= 0) return hipSuccess;
  const int blocks = std::max(1, std::min(total_tiles, max_blocks));
  mv_scan_kernel<<<blocks, kMvBlock, 0, s>>>(tasks, ntasks, total_tiles);
  return hipGetLastError();
}

static hipError_t launch_mv_reduce(const MvReduceTask &t, hipStream_t s) {
  if (t.num_docs <= 0) return hipSuccess;
  const int blocks = (int)(((int64_t)t.num_docs + kMvBlock - 1) / kMvBlock);
  mv_reduce_kernel<<<blocks, kMvBlock, 0, s>>>(t);
  return hipGetLastError();
}

namespace {
const MvLaunchers g_mv_launchers = {&launch_mv_scan, &launch_mv_reduce};
struct MvRegistration {
  MvRegistration() { register_mv_launchers(&g_mv_launchers); }
} g_mv_registration;
}  // namespace

}  // namespace phip
