// distinct_rows.hip -- SELECT DISTINCT: the distinct rows of the matched docs as mixed-radix keys of query-global ids.
//
// DistinctOperator (pinot-core/.../operator/query/DistinctOperator.java:57-87) hands every matched doc's projection
// to a DistinctExecutor (…/query/distinct/DistinctExecutorFactory.java:55-148): over dictionary columns
// DictionaryBasedSingleColumnDistinctExecutor / DictionaryBasedMultiColumnDistinctExecutor keep a set of dict-id
// tuples -- with ORDER BY the best `limit` under a comparator over the order-by columns' dictionary ids (the
// dictionaries are sorted, so id order is value order), without ORDER BY the first `limit` distinct rows met, then they
// stop. DistinctCombineOperator (DistinctResultsBlockMerger, MultiColumnDistinctTable) merges the segments' tables by
// value and DistinctDataTableReducer (…/query/reduce/DistinctDataTableReducer.java:55-79) the servers'. Which of the
// rows that tie on the order-by terms survive, and which `limit` rows a query without ORDER BY returns, depend on the
// arrival order there. Here the rule is fixed: rows are ordered by the ORDER BY terms, then by the remaining select
// columns ascending in select order, and the result is the first `limit` rows of the distinct set in that order -- an
// answer the reference may give.
//
// On the GPU every column's id is mapped through its query-global dictionary (DevCol.remap, the sorted union of the
// segments' dictionaries), so one key space covers every segment: key = sum digit_j x stride_j, digit = id (card - 1 -
// id for a DESC term), the ORDER BY terms the most significant digits. Ascending key order is the rule above. After the
// unfused filter launch, over its lane-major tile masks (the walk of distinct_mark_kernel, distinct.hip):
//   1. distinct_rows_mark_kernel   per matched doc its key, in the regime the host chose per plan:
//        DR_LDS     a bit per key; every workgroup ORs into its own zeroed LDS copy (ds_or, no return value) and
//                   flushes each NON-ZERO word with one global atomic OR;
//        DR_GLOBAL  a bit per key in the global bitmap, test before set (mark_global's argument, distinct.hip);
//        DR_SORTED  the key stored at the doc's rank among the matched docs (select.hip's tile counts, scanned), then
//                   keys.hip launch_sort_unique_u64 leaves the ascending distinct keys;
//   2. bitmaps only: distinct_rows_count_kernel, set bits per chunk of kDistinctRowsChunkWords words; an exclusive
//      scan; distinct_rows_emit_kernel writes the keys of rank < keep in ascending order (a chunk whose first rank is
//      at or past keep returns at once);
//   3. distinct_rows_decode_kernel  per (row, column): the column's digit of the key, a DESC complement undone, the
//      value from the column's query-global dictionary (STRING: the id), column-major -- consecutive lanes write
//      consecutive rows.
// Integer OR and a sort are order-free, so the rows are bit-reproducible whatever the schedule.
#include "agg_common.h"
#include "launch.h"

namespace phip {

typedef const PHIP_CAS DevDistinctRows cdr_t;

constexpr int kDrBlock = 256;
constexpr int kDrWaves = kDrBlock / kWave;
static_assert(kDistinctRowsChunkWords == kDrBlock * 4, "a pick chunk is four words per thread");

// The doc's key. An id is below its cardinality by construction; the clamp keeps a key inside the key space (and a
// bit inside the bitmap) whatever a column holds.
__device__ __forceinline__ uint64_t distinct_rows_key(cdr_t &q, cseg_t &seg, int32_t doc) {
  uint64_t key = 0;
  for (int j = 0; j < q.num_cols; j++) {
    ccol_t &c = seg.cols[q.col[j]];
    const uint32_t id = col_dict_id(c, doc);
    const uint32_t last = (uint32_t)q.card[j] - 1u;
    const uint32_t gid = min(c.remap ? (uint32_t)((const PHIP_GLB int32_t *)c.remap)[id] : id, last);
    key += (uint64_t)(q.desc[j] ? last - gid : gid) * q.stride[j];
  }
  return key;
}

template <int kRegime>
__global__ __launch_bounds__(kDrBlock) void distinct_rows_mark_kernel(const DevDistinctRows *qp,
                                                                      uint64_t *__restrict__ keys, int64_t num_keys) {
  extern __shared__ uint32_t dr_lds[];  // DR_LDS: num_words words, this workgroup's copy of the bitmap
  cdr_t &q = *(cdr_t *)qp;
  cseg_t *segs = (cseg_t *)q.segs;
  const int lane = lane_id();
  const int wave = uniform(threadIdx.x >> 6);
  const int32_t lds_words = (int32_t)q.num_words;  // (DR_LDS: at most the LDS budget)
  if (kRegime == DR_LDS) {
    for (int32_t i = threadIdx.x; i < lds_words; i += kDrBlock) dr_lds[i] = 0u;
    __syncthreads();
  }
  const int64_t nw = (int64_t)gridDim.x * kDrWaves, w = (int64_t)blockIdx.x * kDrWaves + wave;
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
    // decode consecutive docs' ids; a group no lane matched is skipped
    uint32_t any = wave_or32(m);
    if (any == 0u) continue;
    // DR_SORTED: the tile's first rank; its docs rank in the order the groups are taken (any order fills the same
    // slots: the tile's count is the popcount of the same mask, and the sort does not care)
    int64_t rank = kRegime == DR_SORTED ? ((const PHIP_GLB int64_t *)q.tile_off)[t] : 0;
    while (any) {
      const int g = __builtin_clz(any);
      any &= ~(0x80000000u >> g);
      const bool on = ((m << g) & 0x80000000u) != 0u;
      const uint64_t hit = ballot(on);
      if (on) {
        const uint64_t key = distinct_rows_key(q, seg, doc0 + 64 * g + lane);
        if (kRegime == DR_SORTED) {
          const int64_t r = rank + (int64_t)mbcnt64(hit);
          if (r < num_keys) keys[r] = key;
        } else if (kRegime == DR_LDS) {
          (void)__hip_atomic_fetch_or((lds_u32 *)&dr_lds[key >> 5], 1u << (key & 31), PHIP_RLX, PHIP_WG);
        } else {
          glb_u32 *p = (glb_u32 *)(q.bitmap + (size_t)(key >> 5));
          const uint32_t bit = 1u << (key & 31);
          // test before set: within one execution a bit only goes 0 -> 1 (the bitmap is cleared by a memset ahead of
          // the launch on the stream), so a load that sees it set is final and a stale 0 only costs an idempotent OR
          if (!(__hip_atomic_load(p, PHIP_RLX, PHIP_AG) & bit)) (void)__hip_atomic_fetch_or(p, bit, PHIP_RLX, PHIP_AG);
        }
      }
      if (kRegime == DR_SORTED) rank += __popcll(hit);
    }
  }
  if (kRegime == DR_LDS) {
    __syncthreads();
    for (int32_t i = threadIdx.x; i < lds_words; i += kDrBlock) {
      const uint32_t v = dr_lds[i];
      if (v) (void)__hip_atomic_fetch_or((glb_u32 *)(q.bitmap + i), v, PHIP_RLX, PHIP_AG);
    }
  }
}

// A thread's four words of chunk c (zeros past the bitmap's end); the bitmap is 16-byte aligned and a chunk starts at a
// multiple of 1024 words, so the full case is one 16-byte load.
__device__ __forceinline__ void chunk_words(const uint32_t *__restrict__ bitmap, int64_t num_words, int64_t w0,
                                            uint32_t (&v)[4]) {
  if (w0 + 4 <= num_words) {
    const uint4 x = *(const uint4 *)(bitmap + w0);
    v[0] = x.x;
    v[1] = x.y;
    v[2] = x.z;
    v[3] = x.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] = w0 + k < num_words ? bitmap[w0 + k] : 0u;
  }
}

__global__ __launch_bounds__(kDrBlock) void distinct_rows_count_kernel(const uint32_t *__restrict__ bitmap,
                                                                       int64_t num_words, int64_t nchunks,
                                                                       int64_t *__restrict__ chunk_cnt) {
  __shared__ uint32_t wsum[kDrWaves];
  const int wave = threadIdx.x >> 6;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    uint32_t v[4];
    chunk_words(bitmap, num_words, c * kDistinctRowsChunkWords + (int64_t)threadIdx.x * 4, v);
    const uint32_t n = wave_sum_u32((uint32_t)(__popc(v[0]) + __popc(v[1]) + __popc(v[2]) + __popc(v[3])));
    if (lane_id() == 0) wsum[wave] = n;
    __syncthreads();
    if (threadIdx.x == 0) {
      uint32_t s = 0;
      for (int k = 0; k < kDrWaves; k++) s += wsum[k];
      chunk_cnt[c] = s;
    }
    __syncthreads();  // (the sums are read before the next chunk's are written)
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) chunk_cnt[nchunks] = 0;
}

// chunk_off[c] = the rank of chunk c's first key. Ranks grow with c, so the first chunk at or past `keep` ends the
// workgroup's walk. keys holds min(keep, distinct keys) slots: every rank written is below both.
__global__ __launch_bounds__(kDrBlock) void distinct_rows_emit_kernel(const uint32_t *__restrict__ bitmap,
                                                                      int64_t num_words, int64_t nchunks,
                                                                      const int64_t *__restrict__ chunk_off,
                                                                      int64_t keep, uint64_t *__restrict__ keys) {
  __shared__ uint32_t wsum[kDrWaves];
  const int wave = threadIdx.x >> 6;
  for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int64_t base = chunk_off[c];  // (the same for every thread of the workgroup)
    if (base >= keep) return;
    if (chunk_off[c + 1] == base) continue;
    const int64_t w0 = c * kDistinctRowsChunkWords + (int64_t)threadIdx.x * 4;
    uint32_t v[4];
    chunk_words(bitmap, num_words, w0, v);
    const uint32_t n = (uint32_t)(__popc(v[0]) + __popc(v[1]) + __popc(v[2]) + __popc(v[3]));
    const uint32_t incl = wave_incl_scan(n);
    if (lane_id() == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t before = incl - n;
    for (int k = 0; k < wave; k++) before += wsum[k];
    int64_t rank = base + before;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      uint32_t x = v[k];
      while (x != 0u && rank < keep) {
        const int bit = __builtin_ctz(x);
        x &= x - 1u;
        keys[rank++] = (uint64_t)(w0 + k) * 32u + (uint32_t)bit;
      }
    }
    __syncthreads();  // (the waves' sums are read before the next chunk's are written)
  }
}

// blockIdx.y = the SELECT column; consecutive lanes, consecutive rows.
__global__ __launch_bounds__(kDrBlock) void distinct_rows_decode_kernel(const uint64_t *__restrict__ keys, int64_t rows,
                                                                        DistinctRowsDecode d,
                                                                        uint64_t *__restrict__ out) {
  const int k = blockIdx.y;
  const uint64_t stride = d.stride[k], card = (uint64_t)d.card[k];
  const uint64_t *values = d.values[k];
  for (int64_t r = (int64_t)blockIdx.x * kDrBlock + threadIdx.x; r < rows; r += (int64_t)gridDim.x * kDrBlock) {
    uint64_t digit = (keys[r] / stride) % card;
    if (d.desc[k]) digit = card - 1 - digit;
    out[(size_t)k * (size_t)rows + (size_t)r] = values != nullptr ? values[digit] : digit;
  }
}

// ---- launchers (runtime.cpp execute_select_distinct, through register_distinct_rows_launchers) ----------------------
static inline int64_t dr_chunks(int64_t num_words) {
  return (num_words + kDistinctRowsChunkWords - 1) / kDistinctRowsChunkWords;
}
static inline int dr_grid(int64_t n, int max_blocks = 4096) { return (int)(n < 1 ? 1 : (n > max_blocks ? max_blocks : n)); }

static hipError_t launch_distinct_rows_mark(const DevDistinctRows *q, int regime, int64_t total_work, size_t lds_bytes,
                                            int max_blocks, uint64_t *keys, int64_t num_keys, hipStream_t s) {
  if (total_work <= 0) return hipSuccess;
  int64_t blocks = (total_work + kDrWaves - 1) / kDrWaves;
  blocks = blocks < 1 ? 1 : (blocks > max_blocks ? max_blocks : blocks);
  if (regime == DR_LDS) distinct_rows_mark_kernel<DR_LDS><<<(int)blocks, kDrBlock, lds_bytes, s>>>(q, nullptr, 0);
  else if (regime == DR_GLOBAL) distinct_rows_mark_kernel<DR_GLOBAL><<<(int)blocks, kDrBlock, 0, s>>>(q, nullptr, 0);
  else if (regime == DR_SORTED) distinct_rows_mark_kernel<DR_SORTED><<<(int)blocks, kDrBlock, 0, s>>>(q, keys, num_keys);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

static hipError_t launch_distinct_rows_count(const uint32_t *bitmap, int64_t num_words, int max_blocks,
                                             int64_t *chunk_cnt, hipStream_t s) {
  const int64_t nchunks = dr_chunks(num_words);
  distinct_rows_count_kernel<<<dr_grid(nchunks, max_blocks), kDrBlock, 0, s>>>(bitmap, num_words, nchunks, chunk_cnt);
  return hipGetLastError();
}

static hipError_t launch_distinct_rows_emit(const uint32_t *bitmap, int64_t num_words, int max_blocks,
                                            const int64_t *chunk_off, int64_t keep, uint64_t *keys, hipStream_t s) {
  const int64_t nchunks = dr_chunks(num_words);
  if (keep <= 0 || nchunks <= 0) return hipSuccess;
  distinct_rows_emit_kernel<<<dr_grid(nchunks, max_blocks), kDrBlock, 0, s>>>(bitmap, num_words, nchunks, chunk_off, keep, keys);
  return hipGetLastError();
}

static hipError_t launch_distinct_rows_decode(const uint64_t *keys, int64_t rows, const DistinctRowsDecode &d,
                                              uint64_t *out, hipStream_t s) {
  if (rows <= 0 || d.num_cols <= 0) return hipSuccess;
  const dim3 grid((unsigned)dr_grid((rows + kDrBlock - 1) / kDrBlock), (unsigned)d.num_cols);
  distinct_rows_decode_kernel<<<grid, kDrBlock, 0, s>>>(keys, rows, d, out);
  return hipGetLastError();
}

namespace {
const DistinctRowsLaunchers kLaunchers = {launch_distinct_rows_mark, launch_distinct_rows_count,
                                          launch_distinct_rows_emit, launch_distinct_rows_decode};
struct Registrar {
  Registrar() { register_distinct_rows_launchers(&kLaunchers); }
} g_registrar;
}  // namespace

}  // namespace phip
