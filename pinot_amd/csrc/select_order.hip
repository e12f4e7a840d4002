// select_order.hip -- selection ORDER BY: a device top-K over the matched docs.
//
// SelectionOrderByOperator (pinot-core/.../operator/query/SelectionOrderByOperator.java:146-340) pushes every matched
// doc through a PriorityQueue of K = offset + limit rows; the combine (SelectionOrderByCombineOperator) keeps the best
// K of the segments' rows. Rows equal on every term are kept here in ascending (segment, doc) order, so the answer is
// the first K rows of a stable sort of the selection-only rows, and the device computes that directly. After the
// filter launch and select.hip's count + scan:
//   1. select_order_hist_kernel  one streaming pass over the matched docs: the primary term's value (sel_value) ->
//                                its 64-bit order image -> an 11-bit digit (image - imin) >> shift, counted in a
//                                2048-bin LDS table per workgroup, the non-zero bins flushed once into global bins;
//   2. select_order_pick_kernel  one wave: the first digit b at which the running count reaches K;
//   3. select_order_mask_kernel  the same walk writes candidate tile masks: matched and digit <= b. The candidates
//                                -- every doc before the boundary digit plus the whole boundary bucket -- hold the
//                                top K whatever the later terms say; select.hip's count / scan / bases / gather
//                                chain materialises them column-major in (segment, doc) order;
//   4. select_order_keys_kernel  per term, least significant first: the term's order image of every candidate, read
//                                through the permutation so far, then one stable radix pass (launch_sort_pairs). The
//                                first permutation is the identity = (segment, doc) order: the tie rule;
//   5. select_order_rows_kernel  the first min(K, candidates) rows of every column through the final permutation.
// The digit only has to be monotone in the image, so the host's bound (imin, shift) decides how well the pass prunes,
// never what it returns: an image outside the bound clamps to the first or the last bin.
#include "select_common.h"

namespace phip {

typedef const PHIP_CAS DevSelOrder cord_t;

// Order image of a gathered 8-byte slot: INT / LONG / ids by value (sign bit flipped), doubles in Double.compare
// order (double_order); DESC complements.
__device__ __forceinline__ uint64_t sel_order_image(uint64_t v, int32_t kind, int32_t desc) {
  const uint64_t u = kind == SEL_F64 ? double_order(as_f64(v)) : (v ^ 0x8000000000000000ull);
  return desc ? ~u : u;
}

__device__ __forceinline__ uint32_t sel_order_digit(uint64_t img, uint64_t imin, int32_t shift) {
  if (img <= imin) return 0u;
  const uint64_t d = (img - imin) >> shift;
  return d < (uint64_t)kSelOrderBins ? (uint32_t)d : (uint32_t)(kSelOrderBins - 1);
}

// The walk of select_count_kernel; f(t, seg, mask word) for every work tile of this wave that holds a matched doc
// (every tile when all_tiles).
template <bool all_tiles, typename F>
__device__ __forceinline__ void sel_order_walk(csel_t &q, F f) {
  cseg_t *segs = (cseg_t *)q.segs;
  const int64_t nw = (int64_t)gridDim.x * kSelWaves, w = (int64_t)blockIdx.x * kSelWaves + (threadIdx.x >> 6);
  const int b = (int)((int64_t)q.total_work * w / nw), e = (int)((int64_t)q.total_work * (w + 1) / nw);
  int si = 0;
  for (int t = b; t < e; t++) {
    while (si + 1 < q.num_segs && segs[si + 1].work_begin <= t) si++;
    const uint32_t m = sel_tile_mask(q, segs[si], t);
    if (!all_tiles && ballot(m != 0) == 0) continue;
    f(t, segs[si], m);
  }
}

__global__ __launch_bounds__(kSelBlock) void select_order_hist_kernel(const DevSelQuery *qp, const DevSelOrder *op) {
  __shared__ uint32_t bins[kSelOrderBins];
  csel_t &q = *(csel_t *)qp;
  cord_t &o = *(cord_t *)op;
  for (int i = threadIdx.x; i < kSelOrderBins; i += kSelBlock) bins[i] = 0u;
  __syncthreads();
  const PHIP_CAS DevSelect &term = q.sel[o.primary];
  const uint64_t imin = o.imin;
  const int32_t shift = o.shift, desc = o.desc, kind = term.kind;
  const int lane = lane_id();
  sel_order_walk<false>(q, [&](int t, cseg_t &seg, uint32_t m) {
    const int32_t doc0 = (seg.tile0 + (t - seg.work_begin)) * kTileDocs;
    for (int g = 0; g < kTileGroups; g++) {  // bit 31-g of lane l = doc 64g + l: consecutive lanes, consecutive docs
      const bool on = (m >> (31 - g)) & 1u;
      if (ballot(on) == 0) continue;
      if (on) {
        const uint64_t img = sel_order_image(sel_value(seg, term, doc0 + g * 64 + lane), kind, desc);
        atomicAdd(&bins[sel_order_digit(img, imin, shift)], 1u);
      }
    }
  });
  __syncthreads();
  unsigned long long *gbins = (unsigned long long *)o.bins;
  for (int i = threadIdx.x; i < kSelOrderBins; i += kSelBlock)
    if (bins[i] != 0u) atomicAdd(&gbins[i], (unsigned long long)bins[i]);
}

// One wave: lane l sums bins 32l .. 32l+31, an inclusive scan over the lanes finds the lane whose range holds the
// K-th doc, and that lane walks its bins to the boundary. Fewer than K matched docs: the last bin, every doc.
__global__ __launch_bounds__(kWave) void select_order_pick_kernel(const DevSelOrder *op) {
  cord_t &o = *(cord_t *)op;
  constexpr int kPer = kSelOrderBins / kWave;
  const int lane = lane_id();
  const uint64_t *bins = o.bins + lane * kPer;
  uint64_t sum = 0;
  for (int j = 0; j < kPer; j++) sum += bins[j];
  uint64_t incl = sum;
  for (int d = 1; d < kWave; d <<= 1) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)incl, d), hi = (uint32_t)__shfl_up((int)(uint32_t)(incl >> 32), d);
    if (lane >= d) incl += ((uint64_t)hi << 32) | lo;
  }
  const uint64_t total = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(incl >> 32), 63) << 32) |
                         (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)incl, 63);
  const uint64_t keep = (uint64_t)(o.keep < 0 ? 0 : o.keep);
  int64_t *bound = o.bound;
  if (!o.prune || total < keep || keep == 0) {
    if (lane == 0) {
      bound[0] = kSelOrderBins - 1;
      bound[1] = (int64_t)total;
    }
    return;
  }
  uint64_t run = incl - sum;
  if (run < keep && keep <= incl) {  // exactly one lane
    int j = 0;
    for (; j < kPer; j++) {
      run += bins[j];
      if (run >= keep) break;
    }
    bound[0] = lane * kPer + j;
    bound[1] = (int64_t)run;
  }
}

__global__ __launch_bounds__(kSelBlock) void select_order_mask_kernel(const DevSelQuery *qp, const DevSelOrder *op) {
  csel_t &q = *(csel_t *)qp;
  cord_t &o = *(cord_t *)op;
  const PHIP_CAS DevSelect &term = q.sel[o.primary];
  const uint64_t imin = o.imin;
  const int32_t shift = o.shift, desc = o.desc, kind = term.kind;
  const uint32_t last = (uint32_t)o.bound[0];
  PHIP_GLB uint32_t *out = (PHIP_GLB uint32_t *)o.cand_mask;
  const int lane = lane_id();
  sel_order_walk<true>(q, [&](int t, cseg_t &seg, uint32_t m) {
    const int32_t doc0 = (seg.tile0 + (t - seg.work_begin)) * kTileDocs;
    uint32_t c = 0u;
    if (last >= (uint32_t)(kSelOrderBins - 1)) {
      c = m;  // every digit is at or below the last bin
    } else {
      for (int g = 0; g < kTileGroups; g++) {
        const bool on = (m >> (31 - g)) & 1u;
        if (ballot(on) == 0) continue;
        if (on) {
          const uint64_t img = sel_order_image(sel_value(seg, term, doc0 + g * 64 + lane), kind, desc);
          if (sel_order_digit(img, imin, shift) <= last) c |= 0x80000000u >> g;
        }
      }
    }
    out[(size_t)t * 64 + lane] = c;
  });
}

// cols: the gathered candidates, column-major [num_select][n]. perm == nullptr: candidate order.
__global__ void select_order_keys_kernel(const uint64_t *__restrict__ cols, int64_t n, SelOrderTerm term,
                                         const int32_t *__restrict__ perm, uint64_t *__restrict__ ukeys,
                                         int32_t *__restrict__ idx) {
  const uint64_t *col = cols + (size_t)term.sel * (size_t)n;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = perm ? perm[i] : i;
    const uint64_t v = col[g];
    ukeys[i] = term.kind == SEL_ID ? (term.desc ? (uint64_t)(term.card - 1) - v : v)
                                   : sel_order_image(v, term.kind, term.desc);
    idx[i] = (int32_t)g;
  }
}

// Row r of the result = candidate perm[r]; consecutive lanes write consecutive rows of every column.
__global__ void select_order_rows_kernel(const uint64_t *__restrict__ cols, int64_t n, int32_t ncols,
                                         const int32_t *__restrict__ perm, int64_t rows, uint64_t *__restrict__ out) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < rows; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t g = perm[r];
    for (int k = 0; k < ncols; k++) out[(size_t)k * (size_t)rows + (size_t)r] = cols[(size_t)k * (size_t)n + (size_t)g];
  }
}

// ---- launchers (runtime.cpp execute_select_ordered, through register_select_order_launchers) ------------------------
static inline int order_grid(int64_t n) {
  const int64_t g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// The other walks' grid: a quarter and a half of it measured slower or equal, the flushes (up to 2048 bins per
// workgroup) notwithstanding.
static hipError_t launch_select_order_hist(const DevSelQuery *q, const DevSelOrder *o, int64_t total_work, int max_blocks,
                                           hipStream_t s) {
  if (total_work <= 0) return hipSuccess;
  select_order_hist_kernel<<<sel_blocks(total_work, max_blocks), kSelBlock, 0, s>>>(q, o);
  return hipGetLastError();
}

static hipError_t launch_select_order_pick(const DevSelOrder *o, hipStream_t s) {
  select_order_pick_kernel<<<1, kWave, 0, s>>>(o);
  return hipGetLastError();
}

static hipError_t launch_select_order_mask(const DevSelQuery *q, const DevSelOrder *o, int64_t total_work, int max_blocks,
                                           hipStream_t s) {
  if (total_work <= 0) return hipSuccess;
  select_order_mask_kernel<<<sel_blocks(total_work, max_blocks), kSelBlock, 0, s>>>(q, o);
  return hipGetLastError();
}

// One stable radix pass per term, least significant term first. Scratch: ukeys[2n] (u64), idx[2n] (i32), then the
// sort's temp storage; *scratch_bytes reports the total when scratch == nullptr.
static hipError_t launch_select_order_sort(const uint64_t *cols, int64_t n, const SelOrderTerm *terms, int32_t num_terms,
                                           void *scratch, size_t *scratch_bytes, const int32_t **order_out,
                                           hipStream_t s) {
  size_t sort_bytes = 0;
  hipError_t e = launch_sort_pairs(nullptr, &sort_bytes, nullptr, nullptr, nullptr, nullptr, false, n, 64, s);
  if (e != hipSuccess) return e;
  const size_t keys_bytes = ((size_t)n * 16 + 255) & ~(size_t)255, idx_bytes = ((size_t)n * 8 + 255) & ~(size_t)255;
  if (scratch == nullptr) {
    *scratch_bytes = keys_bytes + idx_bytes + sort_bytes;
    return hipSuccess;
  }
  uint64_t *k0 = (uint64_t *)scratch, *k1 = k0 + n;
  int32_t *i0 = (int32_t *)((uint8_t *)scratch + keys_bytes), *i1 = i0 + n;
  void *tmp = (uint8_t *)scratch + keys_bytes + idx_bytes;
  const int32_t *perm = nullptr;
  for (int j = num_terms - 1; j >= 0; j--) {
    select_order_keys_kernel<<<order_grid(n), 256, 0, s>>>(cols, n, terms[j], perm, k0, i0);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    size_t tb = sort_bytes;
    e = launch_sort_pairs(tmp, &tb, k0, k1, i0, i1, false, n, terms[j].bits, s);
    if (e != hipSuccess) return e;
    perm = i1;  // the next pass reads i1 and writes k0 / i0: no overlap
  }
  *order_out = i1;
  return hipSuccess;
}

static hipError_t launch_select_order_rows(const uint64_t *cols, int64_t n, int32_t ncols, const int32_t *perm,
                                           int64_t rows, uint64_t *out, hipStream_t s) {
  if (rows <= 0) return hipSuccess;
  select_order_rows_kernel<<<order_grid(rows), 256, 0, s>>>(cols, n, ncols, perm, rows, out);
  return hipGetLastError();
}

namespace {
const SelectOrderLaunchers kLaunchers = {launch_select_order_hist, launch_select_order_pick, launch_select_order_mask,
                                         launch_select_order_sort, launch_select_order_rows};
struct Registrar {
  Registrar() { register_select_order_launchers(&kLaunchers); }
} g_registrar;
}  // namespace

}  // namespace phip
