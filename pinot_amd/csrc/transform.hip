// transform.hip -- time transforms (dateTrunc, toEpoch*, timeConvert, the ISO-chronology fields) of one dictionary
// column, evaluated per dictionary entry, never per doc (device.h TransformTask; civil.h time_transform; runtime.cpp
// build_remap / phip_segment_match_transform; include/pinot_hip.h phip_time_transform).
//
// The reference evaluates a transform per projected doc (DateTruncTransformFunction.transformToLongValuesSV over a
// block, ExpressionFilterOperator per scanned doc). A dictionary column's docs hold ids, so f(dict[id]) per entry says
// everything: GROUP BY f(col) is the group-by walks' own remap gather with global ids numbering the distinct values of
// f, and WHERE f(col) <op> literal is a scan leaf over the ids whose entries match. No walk knows of transforms.
//
// dict_transform_kernel: one lane per entry, one 256-thread workgroup per 2048-entry tile, grid-strided over the
// dictionary's tiles. The task is read through the constant address space: the program's function, unit and scales
// are scalars and its branches are scalar branches. A wave takes 64-entry groups; its match word is the ballot of the
// lanes' predicate, stored once by one lane -- every word of every tile, zeros past card, no atomics.
// transform_remap_kernel: one lane per entry, a binary search of its image among the query's distinct images.
#include "civil.h"
#include "dev_common.h"
#include "launch.h"

#include <algorithm>

namespace phip {

constexpr int kTtBlock = 256;
constexpr int kTtWaves = kTtBlock / 64;

typedef const PHIP_CAS TransformTask ctt_t;

__global__ __launch_bounds__(kTtBlock) void dict_transform_kernel(const TransformTask *task, int32_t num_tiles) {
  ctt_t &t = *(ctt_t *)task;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  TimeProgram p;
  p.function = t.function;
  p.unit = t.unit;
  p.in_mul = t.in_mul;
  p.in_div = t.in_div;
  p.out_mul = t.out_mul;
  p.out_div = t.out_div;
  const int32_t card = t.card;
  const bool wide = t.type == PHIP_TYPE_LONG;
  uint64_t *values = t.values;
  uint64_t *match = t.match;
  const int32_t pred = t.pred;
  for (int32_t tile = blockIdx.x; tile < num_tiles; tile += gridDim.x) {
    for (int g = wave; g < kTileDocs / 64; g += kTtWaves) {
      const int64_t i = (int64_t)tile * kTileDocs + 64 * g + lane;
      bool ok = false;
      if (i < card) {
        const int64_t v = wide ? ((const int64_t *)t.dict)[i] : (int64_t)((const int32_t *)t.dict)[i];
        const int64_t r = time_transform(p, v);
        if (values) values[i] = (uint64_t)r ^ 0x8000000000000000ull;
        if (pred == kTtPredRange) {
          ok = (r > t.lo || (t.lo_inclusive && r == t.lo)) && (r < t.hi || (t.hi_inclusive && r == t.hi));
        } else if (pred == kTtPredSet) {
          int32_t a = 0, b = t.set_count;  // the first member >= r
          while (a < b) {
            const int32_t m = (a + b) >> 1;
            if (t.set[m] < r) a = m + 1;
            else b = m;
          }
          ok = a < t.set_count && t.set[a] == r;
        }
        if (t.invert) ok = !ok;
      }
      const uint64_t word = __ballot(ok);  // (lanes at and past card: 0)
      if (match && lane == 0) match[(int64_t)tile * (kTileDocs / 64) + g] = word;
    }
  }
}

__global__ void transform_remap_kernel(const uint64_t *__restrict__ images, int64_t n, const uint64_t *__restrict__ uniq,
                                       int64_t u, int32_t *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t x = images[i];
    int64_t a = 0, b = u;  // the first distinct image >= x: x itself, the images are among them
    while (a < b) {
      const int64_t m = (a + b) >> 1;
      if (uniq[m] < x) a = m + 1;
      else b = m;
    }
    out[i] = (int32_t)(a < u ? a : u - 1);
  }
}

static hipError_t launch_dict_transform(const TransformTask *task, int32_t card, int max_blocks, hipStream_t s) {
  if (card <= 0) return hipSuccess;
  const int32_t tiles = (int32_t)(((int64_t)card + kTileDocs - 1) / kTileDocs);
  const int blocks = std::max(1, std::min(tiles, max_blocks));
  dict_transform_kernel<<<blocks, kTtBlock, 0, s>>>(task, tiles);
  return hipGetLastError();
}

static hipError_t launch_transform_remap(const uint64_t *images, int64_t n, const uint64_t *uniq, int64_t u, int32_t *out,
                                         hipStream_t s) {
  if (n <= 0 || u <= 0) return hipSuccess;
  const int64_t g = (n + 255) / 256;
  transform_remap_kernel<<<(int)(g > 8192 ? 8192 : g), 256, 0, s>>>(images, n, uniq, u, out);
  return hipGetLastError();
}

namespace {
const TransformLaunchers g_transform_launchers = {&launch_dict_transform, &launch_transform_remap};
struct TransformRegistration {
  TransformRegistration() { register_transform_launchers(&g_transform_launchers); }
} g_transform_registration;
}  // namespace

}  // namespace phip
