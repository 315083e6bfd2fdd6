// ea_lanes_stream.h — the coordinate stream of a wavefront of ea_eval_poses_lanes_kernel, as pure functions the kernel and
// the host share (tests/poses_lanes_stream_host_shim.cpp plays them without a device).
//
// A wavefront walks its sub-run of n_sub points (1 .. 128) two per iteration: iteration k consumes the points
// (2 k, min(2 k + 1, last)), last = n_sub - 1 -- an odd sub-run ends on its last point taken twice, as it always has.  The
// coordinates of a pair are wave-uniform and arrive through scalar loads ONE pair ahead: the prologue (slot -1) loads pair 0,
// iteration k loads pair k + 1 while it sums pair k up, straight into the registers iteration k + 1 reads.
//
// What a slot loads from each of the three arrays:
//   a whole pair inside the sub-run (2 (k + 1) + 1 <= last): ONE 16-byte load of the two adjacent points;
//   otherwise two 8-byte loads of indices clamped to `last`: the odd sub-run's last pair (last, last), and behind the
//   sub-run's last pair a copy of the last point that nobody consumes -- the loop keeps one shape to its end.
// No index at or beyond n_sub is ever formed, so nothing is read behind the problem's last point.
#pragma once
#include "ea_types.h"

namespace ea {

struct LanesStreamLoad {
  int i0, i1;  // the indices that land in the pair's first and second register
  int wide;    // 1: i1 == i0 + 1 and both come with one 16-byte load at i0
};
// iterations of the loop
EA_HD inline int lanes_stream_iters(int n_sub) { return (n_sub + 1) >> 1; }
// the points iteration k consumes
EA_HD inline LanesStreamLoad lanes_stream_pair(int k, int n_sub) {
  const int last = n_sub - 1, i = 2 * k;
  if (i + 1 <= last) return LanesStreamLoad{i, i + 1, 1};
  return LanesStreamLoad{last, last, 0};  // (i >= last: min(i, last) = min(i + 1, last) = last)
}
// what is loaded in slot k (-1 = the prologue, 0 .. iters - 1 = iteration k): the pair iteration k + 1 consumes
EA_HD inline LanesStreamLoad lanes_stream_load(int k, int n_sub) { return lanes_stream_pair(k + 1, n_sub); }

}  // namespace ea
