// fused_shape.h -- the launch shape of a small fused aggregation scan (runtime.cpp, the filter kernel's configuration):
// the fewest tiles per wave at which every workgroup of the launch is resident at once, i.e. the whole scan is one
// generation of waves and no wave queues behind another. A pure host function (no HIP dependency), so that a
// stand-alone program can sweep it (tests/fused_shape).
//
// A plan has up to two candidate modes, which differ in the bytes of one LDS-DMA ring slot and of the matched-doc ring:
//   mode 0: the value columns stream with the tile (the density rule's choice, runtime.cpp kStreamValueMin);
//   mode 1: the matched docs are deferred and their values gathered (the slot holds the filter's sources alone).
// Per mode the function finds the smallest T (tiles per wave) such that blocks = ceil(tiles / (waves * T)) workgroups
// fit cus * bpc, where bpc = min(wave_cap, lds_cu / lds) workgroups share a CU's LDS at
//   lds = waves * nbuf * slot + doc_ring + static_lds   per workgroup.
// Ring depth: the deepest ring (<= kMaxRing) with which those workgroups are still all resident -- LDS the residency
// does not need goes to the ring. A wave with one tile can run in a single slot (issue the tile's DMA, wait for it,
// evaluate) and gets one when the residency asks for it; with spare LDS it keeps the deeper ring, whose prologue
// issues the tile's DMA ahead of the wave's set-up loads (sorted SSB Q1.3, 216 one-tile workgroups: 21.6 us in one
// slot against 20.4-20.9 us in two or eight). A wave with T >= 2 tiles wants the next tile in
// flight while it evaluates one, so T is the smallest that fits with at least two slots; a single slot under T >= 2
// only when two do not fit one workgroup at all, or when the depth is forced (force_nbuf, PHIP_FILTER_NBUF).
// The mode with the smaller T wins; on a tie mode 0, the density rule's own choice, stays.
#pragma once
#include <stdint.h>

namespace phip {

constexpr int kShapeLdsPerCu = 160 * 1024;  // gfx950: LDS bytes of one CU, and the most one workgroup may take
constexpr int kShapeMaxRing = 8;            // device.h kMaxRing (static_assert in runtime.cpp)

struct FusedShapeIn {
  int64_t tiles;        // work tiles of the launch (> 0)
  int32_t slot[2];      // bytes of one ring slot per mode (a multiple of 16); 0 = the plan has no such mode
  int32_t doc_ring[2];  // bytes of the workgroup's matched-doc rings per mode
  int32_t static_lds;   // the kernel's static LDS per workgroup
  int32_t waves;        // waves per workgroup
  int32_t cus;          // CUs the grid is sized from
  int32_t wave_cap;     // workgroups per CU the kernel is compiled for (its waves per SIMD)
  int32_t force_nbuf;   // 0 = by the rule, 1..kShapeMaxRing = this ring depth
};

struct FusedShape {
  int32_t mode;    // 0 / 1, -1 = no mode fits (a slot beyond a CU's LDS)
  int32_t blocks;  // workgroups, all resident at once: blocks <= cus * bpc (before any rounding of the grid)
  int32_t nbuf;    // ring slots per wave
  int32_t bpc;     // workgroups per CU the LDS and the wave cap admit at this depth
  int64_t T;       // tiles per wave at most: blocks * waves * T >= tiles
};

// workgroups per CU at ring depth nbuf, 0 = one workgroup does not fit
inline int32_t fused_shape_bpc(const FusedShapeIn &in, int mode, int nbuf) {
  const int64_t lds = (int64_t)in.waves * nbuf * in.slot[mode] + in.doc_ring[mode] + in.static_lds;
  if (lds > kShapeLdsPerCu) return 0;
  const int64_t by_lds = kShapeLdsPerCu / lds;
  return (int32_t)(by_lds < in.wave_cap ? by_lds : in.wave_cap);
}

// the smallest T in [t_lo, ..) of one mode with a ring depth in [lo, hi], deepest ring first; mode -1 when none fits
inline FusedShape fused_shape_mode(const FusedShapeIn &in, int mode, int64_t t_lo, int lo, int hi) {
  FusedShape s = {-1, 0, 0, 0, 0};
  if (in.slot[mode] <= 0 || in.tiles <= 0) return s;
  const int64_t per_block = in.waves;
  const int64_t t_max = (in.tiles + per_block - 1) / per_block;  // one workgroup walks everything
  // blocks(T) falls with T, so the first fit is the smallest T
  for (int64_t T = t_lo; T <= (t_max > t_lo ? t_max : t_lo); T++) {
    const int64_t blocks = (in.tiles + per_block * T - 1) / (per_block * T);
    for (int nbuf = hi; nbuf >= lo; nbuf--) {
      const int32_t bpc = fused_shape_bpc(in, mode, nbuf);
      if (bpc > 0 && blocks <= (int64_t)in.cus * bpc) {
        s.mode = mode;
        s.blocks = (int32_t)blocks;
        s.nbuf = nbuf;
        s.bpc = bpc;
        s.T = T;
        return s;
      }
    }
    // jump over the T that give the same block count (they cannot fit either)
    if (blocks > 1) {
      const int64_t next = (in.tiles + per_block * (blocks - 1) - 1) / (per_block * (blocks - 1));
      if (next > T + 1) T = next - 1;
    }
  }
  return s;
}

inline FusedShape fused_small_shape(const FusedShapeIn &in) {
  FusedShape best = {-1, 0, 0, 0, 0};
  for (int mode = 0; mode < 2; mode++) {
    FusedShape s;
    if (in.force_nbuf > 0) {
      s = fused_shape_mode(in, mode, 1, in.force_nbuf, in.force_nbuf);
    } else {
      // one-tile waves with any depth; else at least two slots; a single slot for long waves as the last resort
      s = fused_shape_mode(in, mode, 1, 1, kShapeMaxRing);
      if (s.mode < 0 || s.T > 1) s = fused_shape_mode(in, mode, 2, 2, kShapeMaxRing);
      if (s.mode < 0) s = fused_shape_mode(in, mode, 2, 1, 1);
    }
    if (s.mode >= 0 && (best.mode < 0 || s.T < best.T)) best = s;
  }
  return best;
}

}  // namespace phip
