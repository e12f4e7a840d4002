// strmatch.hip -- REGEXP_LIKE / LIKE: a byte-level DFA walked over STRING values (device.h StrMatchTask; runtime.cpp
// strmatch_image, PlanBuilder::make_leaf / stage_inverted_leaves, phip_segment_match_dictionary; include/pinot_hip.h
// "DFA blob").
//
// The reference runs java.util.regex's Matcher.reset(value).find() per scanned doc (RegexpLikePredicateEvaluator-
// Factory.java:74-76 for a dictionary column, after a dictionary lookup; :108-110 for a raw one) and always scans
// (FilterOperatorUtils.java:108-117). Here the host compiles the pattern once into a DFA with find() built in, and
// the predicate is a table walk: one lane per string, the table in LDS. Two string locators share the walk:
//   raw          doc d = bytes [offsets[d], offsets[d + 1]) of the column's resident bytes (load_varbyte)
//   dictionary   entry i = the `width` bytes at i * width, up to its first 0 pad byte
//                (FixedByteValueReaderWriter.readUnpaddedBytes)
// so a dictionary column costs `cardinality` walks, not num_docs, and a raw column one pre-pass that writes dense doc
// words the filter kernels read as an inverted leaf's (as mv_scan_kernel does): no filter kernel knows of patterns.
//
// Shape: one 256-thread workgroup per 2048-element tile, grid-strided over all tasks' tiles. The task's table image
// (256-byte class map, then the u16 transitions pre-multiplied by the class count: a byte costs the two dependent
// LDS reads trans[state + cmap[byte]]) is copied to LDS when the workgroup meets a new task. Each wave takes
// 64-element groups. A group's strings are one contiguous byte span: the wave stages it into its own LDS window with
// coalesced 16-byte loads and every lane walks its own string out of the window, a dword at a time. A span longer
// than the window is taken in windows, lanes carrying their state; the next window starts at the first live lane's
// position (positions ascend with the lane), so the bytes behind an early exit are never loaded. A lane is live until
// its string ends or its state is absorbing (the library numbers those states first: one compare); the group ends
// when __ballot says no lane is live. The group's result is the ballot of "final state accepting" -- exactly u64 word
// element / 64 -- stored once by one lane, zeros past the last element: no atomics, and every word of every tile
// written, so the words need no clearing pass.
#include "dev_common.h"
#include "launch.h"

#include <algorithm>
#include <mutex>

namespace phip {

constexpr int kSmBlock = 256;
constexpr int kSmWaves = kSmBlock / 64;
constexpr int kSmWinVecs = kStrMatchWindow / 16;  // uint4 per window
constexpr int kSmCmapWords = 64;

typedef const PHIP_CAS StrMatchTask csm_t;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

extern __shared__ u32x4 sm_lds[];  // [table image, padded to 16 bytes][kSmWaves windows]

__device__ __forceinline__ uint64_t shfl_u64(uint64_t v, int src) {
  const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src);
  const uint32_t hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
  return ((uint64_t)hi << 32) | lo;
}

// One 64-element group: -> the lanes' "accepted" ballot (bits at and past ng are 0).
template <bool kDict>
__device__ __forceinline__ uint64_t strmatch_group(csm_t &t, int64_t eb, int32_t ng, const uint8_t *cmap,
                                                   const uint16_t *trans, u32x4 *win, int lane) {
  const uint8_t *bytes = t.bytes;
  uint64_t lo, hi;
  if (kDict) {
    const uint64_t w = (uint64_t)t.width;
    lo = (uint64_t)(eb + min(lane, ng)) * w;
    hi = lane < ng ? lo + w : lo;
  } else {
    const int64_t e = eb + min(lane, ng);  // (<= num: offsets holds num + 1 entries)
    lo = t.offsets[e];
    hi = lane < ng ? t.offsets[e + 1] : lo;
  }
  const uint64_t span_end = (shfl_u64(hi, 63) + 15ull) & ~15ull;  // the buffers are padded by 16 bytes
  const uint32_t absorb_end = (uint32_t)t.absorb_end;
  uint32_t state = (uint32_t)t.start;
  uint64_t pos = lo;
  bool live = pos < hi && state >= absorb_end;
  uint64_t m = __ballot(live);
  const uint32_t *win32 = (const uint32_t *)win;
  while (m) {
    const int first = __ffsll((long long)m) - 1;
    const uint64_t w0 = shfl_u64(pos, first) & ~15ull;  // positions ascend with the lane: the first live one is lowest
    const uint64_t wend = min(w0 + (uint64_t)kStrMatchWindow, span_end);
    __builtin_amdgcn_wave_barrier();  // the previous window's reads are done
#pragma unroll
    for (int k = 0; k < kSmWinVecs / 64; k++) {
      const uint64_t a = w0 + 16ull * (uint32_t)(lane + 64 * k);
      if (a < wend) win[lane + 64 * k] = *(const u32x4 *)(bytes + a);
    }
    __builtin_amdgcn_wave_barrier();
    if (live && pos < w0 + (uint64_t)kStrMatchWindow) {
      uint32_t p = (uint32_t)(pos - w0);
      const uint32_t e = (uint32_t)(min(hi, w0 + (uint64_t)kStrMatchWindow) - w0);
      while (p < e) {
        uint32_t wv = win32[p >> 2] >> (8u * (p & 3u));
        const uint32_t n = min(4u - (p & 3u), e - p);
        bool ended = false;
        for (uint32_t k = 0; k < n; k++) {
          const uint32_t b = wv & 0xffu;
          wv >>= 8;
          if (kDict && b == 0u) {  // the entry's first pad byte: its value ends here
            ended = true;
            break;
          }
          state = trans[state + cmap[b]];
        }
        p += n;
        if (ended) {
          hi = 0;  // (pos >= hi from here on: not live)
          break;
        }
        if (state < absorb_end) break;
      }
      pos = w0 + p;
    }
    live = pos < hi && state >= absorb_end;
    m = __ballot(live);
  }
  const bool ok = lane < ng && state - (uint32_t)t.accept_begin < (uint32_t)(t.accept_end - t.accept_begin);
  return __ballot(ok);
}

__global__ __launch_bounds__(kSmBlock) void strmatch_kernel(const StrMatchTask *tasks, int32_t ntasks, int32_t total_tiles,
                                                            int32_t table_words) {
  uint32_t *s_table = (uint32_t *)sm_lds;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  u32x4 *win = sm_lds + ((table_words + 3) >> 2) + wave * kSmWinVecs;
  int staged_task = -1;
  for (int32_t w = blockIdx.x; w < total_tiles; w += gridDim.x) {
    int ti = 0;
    while (ti + 1 < ntasks && ((csm_t *)tasks)[ti + 1].tile_begin <= w) ti++;
    csm_t &t = ((csm_t *)tasks)[ti];
    if (staged_task != ti) {  // (uniform over the workgroup)
      __syncthreads();        // the previous task's table is no longer read
      const int32_t tw = min(table_words, kSmCmapWords + ((t.num_states * t.num_classes + 1) >> 1));
      for (int i = tid; i < tw; i += kSmBlock) s_table[i] = t.table[i];
      staged_task = ti;
      __syncthreads();
    }
    const uint8_t *cmap = (const uint8_t *)s_table;
    const uint16_t *trans = (const uint16_t *)(s_table + kSmCmapWords);
    const int32_t tile = w - t.tile_begin;
    const bool dict = t.offsets == nullptr;
    for (int g = wave; g < kTileDocs / 64; g += kSmWaves) {
      const int64_t eb = (int64_t)tile * kTileDocs + 64 * g;
      const int32_t ng = (int32_t)max((int64_t)0, min((int64_t)64, (int64_t)t.num - eb));  // (0: past the elements)
      uint64_t word = 0;
      if (ng > 0) {
        word = dict ? strmatch_group<true>(t, eb, ng, cmap, trans, win, lane)
                    : strmatch_group<false>(t, eb, ng, cmap, trans, win, lane);
        const uint64_t valid = ng >= 64 ? ~0ull : ((1ull << ng) - 1ull);
        if (t.invert) word = ~word;
        word &= valid;
      }
      if (lane == 0) t.out[(int64_t)tile * t.tile_words + g] = word;
    }
  }
}

static size_t strmatch_lds_bytes(int32_t table_words) {
  return (size_t)((table_words + 3) >> 2) * 16 + (size_t)kSmWaves * kStrMatchWindow;
}

static hipError_t launch_strmatch(const StrMatchTask *tasks, int32_t ntasks, int32_t total_tiles, int32_t table_words,
                                  int max_blocks, hipStream_t s) {
  if (ntasks <= 0 || total_tiles <= 0) return hipSuccess;
  constexpr int32_t kMaxWords = kSmCmapWords + kStrMatchMaxTableBytes / 4;
  if (table_words < kSmCmapWords || table_words > kMaxWords) return hipErrorInvalidValue;
  // the largest table image and the windows pass the 64 KiB a launch gets by default: raise the kernel's limit once
  static std::once_flag once;
  static hipError_t attr = hipSuccess;
  std::call_once(once, [] {
    attr = hipFuncSetAttribute((const void *)strmatch_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)strmatch_lds_bytes(kMaxWords));
  });
  const size_t lds = strmatch_lds_bytes(table_words);
  if (attr != hipSuccess && lds > 64 * 1024) return attr;
  const int blocks = std::max(1, std::min(total_tiles, max_blocks));
  strmatch_kernel<<<blocks, kSmBlock, lds, s>>>(tasks, ntasks, total_tiles, table_words);
  return hipGetLastError();
}

namespace {
const StrMatchLaunchers g_strmatch_launchers = {&launch_strmatch};
struct StrMatchRegistration {
  StrMatchRegistration() { register_strmatch_launchers(&g_strmatch_launchers); }
} g_strmatch_registration;
}  // namespace

}  // namespace phip
