// tile_range.h -- which tiles of the work list a filter wave, and so a filter workgroup, streams. One function for the
// kernel (filter_kernel.h) and for the host's per-block table of the record mode (host_final.h): the two cannot drift.
// No HIP dependency.
#pragma once
#include <stdint.h>

#include "device.h"  // PHIP_HD

namespace phip {

struct TileRange {
  int begin, end;  // tiles [begin, end) of the work list, walked one by one
};

// The contiguous range of wave `wave` of workgroup `block` (nwaves per workgroup, nblocks workgroups):
// xcd_walk == 0: the work list cut into one range per wave, in wave order;
// xcd_walk == 2: the work list cut into 8 XCD ranges (workgroup b runs on XCD b & 7; nblocks is a multiple of 8), each
//                cut into one range per wave of that XCD's workgroups.
// (xcd_walk == 1, the strided sweep, has no contiguous ranges and is not covered.) A workgroup's waves hold
// neighbouring ranges in wave order, so the workgroup's range is [its wave 0's begin, its last wave's end).
PHIP_HD inline TileRange wave_tile_range(int xcd_walk, int total_work, int nblocks, int block, int wave, int nwaves) {
  TileRange r;
  if (xcd_walk == 2) {
    const int x = block & 7, gx = nblocks >> 3;
    const int64_t xs = (int64_t)total_work * x / 8, xe = (int64_t)total_work * (x + 1) / 8;
    const int64_t nw = (int64_t)gx * nwaves, w = (int64_t)(block >> 3) * nwaves + wave;
    r.begin = (int)(xs + (xe - xs) * w / nw);
    r.end = (int)(xs + (xe - xs) * (w + 1) / nw);
  } else {
    const int64_t waves_total = (int64_t)nblocks * nwaves;
    const int64_t gw = (int64_t)block * nwaves + wave;
    r.begin = (int)((int64_t)total_work * gw / waves_total);
    r.end = (int)((int64_t)total_work * (gw + 1) / waves_total);
  }
  return r;
}

PHIP_HD inline TileRange block_tile_range(int xcd_walk, int total_work, int nblocks, int block, int nwaves) {
  TileRange r;
  r.begin = wave_tile_range(xcd_walk, total_work, nblocks, block, 0, nwaves).begin;
  r.end = wave_tile_range(xcd_walk, total_work, nblocks, block, nwaves - 1, nwaves).end;
  return r;
}

}  // namespace phip
