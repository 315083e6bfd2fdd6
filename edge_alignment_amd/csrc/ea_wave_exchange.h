// ea_wave_exchange.h — who owns which slot in the wave-exchange reduction of a 256-lane fp64 workgroup (fused_chunk,
// ea_kernels.hip), as pure functions the kernel and the host share: the host replays the two exchange rounds and the
// 8-value butterfly symbolically with them and tests them without a device (tests/wave_exchange_host_shim.cpp).
//
// Every lane of the four wavefronts holds 32 sums.  Instead of one 32-value butterfly per wavefront and a cross-wave sum of
// the four results, the wavefronts first add their sums LANE BY LANE through LDS -- a reduce-scatter in two rounds --
// so that wavefront w ends up with 8 of the 32 slots, in every lane already summed over the four wavefronts, and runs a
// butterfly over those 8 values only:
//
//   round 1, pairs w <-> w ^ 1: a wavefront keeps the half [16 (w & 1), +16) of the 32 slots and stores the other half into
//     region w; behind a barrier it adds what its partner stored (region w ^ 1) to the half it kept.
//   round 2, pairs w <-> w ^ 2: of its 16 it keeps [8 ((w >> 1) & 1), +8) and stores the other 8 into region w ^ 1 -- the region
//     its round-1 partner wrote, whose only reader it was, and which it has finished reading: no barrier against the round-1
//     reads, no second buffer.  Behind the second barrier it adds what w ^ 2 stored: region (w ^ 2) ^ 1 = w ^ 3.
//   butterfly: 8 -> 4 across half-waves (L ^ 32), 4 -> 2 across 16-lane rows (L ^ 16), 2 -> 1 inside a row (L ^ 15); then
//     three levels that add the partner's value (L ^ 7, L ^ 2, L ^ 1), after which the 8 lanes that agree in bits 5, 4, 3
//     hold the finished sum of slot first_slot(w) + 4 b5 + 2 b4 + b3.  The lane of the eight with L & 7 == 0 stores it.
//
// LDS: 4 regions of 16 cells x 64 lanes x 8 bytes = 32 KB.  Cell j of a lane lies at
// region * 8192 + (j / 2) * 1024 + lane * 16 + (j & 1) * 8: a lane moves two cells per 16-byte access, and the 64 lanes of
// an access are contiguous.
#pragma once

#include "ea_types.h"

namespace ea {

constexpr int kXchgWaves = 4, kXchgRegionCells = 16;
constexpr int kXchgRegionBytes = kXchgRegionCells * 64 * 8;      // 8 KB per wavefront
constexpr int kXchgBytes = kXchgWaves * kXchgRegionBytes;        // 32 KB per workgroup

// first of the 16 slots wavefront w keeps in round 1 / of the 16 it stores
EA_HD inline int xchg_keep16(int w) { return 16 * (w & 1); }
EA_HD inline int xchg_send16(int w) { return 16 * ((w & 1) ^ 1); }
// within its 16: first of the 8 it keeps in round 2 / of the 8 it stores
EA_HD inline int xchg_keep8(int w) { return 8 * ((w >> 1) & 1); }
EA_HD inline int xchg_send8(int w) { return 8 * (((w >> 1) & 1) ^ 1); }
// the regions a wavefront writes and reads in the two rounds
EA_HD inline int xchg_write_region1(int w) { return w; }
EA_HD inline int xchg_read_region1(int w) { return w ^ 1; }
EA_HD inline int xchg_write_region2(int w) { return w ^ 1; }
EA_HD inline int xchg_read_region2(int w) { return w ^ 3; }
// first of the 8 slots wavefront w owns behind round 2
EA_HD inline int xchg_first_slot(int w) { return xchg_keep16(w) + xchg_keep8(w); }
// byte offset of cell j (0..15) of `lane` in `region`
EA_HD inline int xchg_cell_offset(int region, int j, int lane) {
  return region * kXchgRegionBytes + (j >> 1) * 1024 + lane * 16 + (j & 1) * 8;
}
// which of its wavefront's 8 values a lane holds behind the butterfly
EA_HD inline int xchg_lane_value(int lane) { return ((lane >> 5) & 1) * 4 + ((lane >> 4) & 1) * 2 + ((lane >> 3) & 1); }
// the slot of the partial row lane `lane` of wavefront w stores, -1: the lane stores nothing
EA_HD inline int xchg_store_slot(int w, int lane) { return (lane & 7) == 0 ? xchg_first_slot(w) + xchg_lane_value(lane) : -1; }

}  // namespace ea
