// ea_poses_map.h — which piece of a pose-batched evaluation launch a workgroup takes (ea_eval_poses_kernel), as pure
// functions the kernel and the host share: the host sizes the grid with them and tests them without a device
// (tests/poses_map_host_shim.cpp).
//
// A launch evaluates g poses of a batch whose points are cut into `rows` chunks per pose (all terms together: one partial
// row per chunk), T = rows * g work items in all, and may carry `riders`: workgroups that fold the rows the PREVIOUS launch
// left behind, one per (pose, problem) of that launch.  The grid is one-dimensional:
//
//   workgroups [0, slots)            slots = riders rounded up to 8: rider L for L < riders, nothing otherwise.  They are
//                                    dispatched first, so the previous launch's results land early.
//   workgroups [slots, slots + 8 per) per = ceil(T / 8): workgroup slots + e takes item (e & 7) * per + (e >> 3).
//
// Workgroups are dealt round-robin over the 8 XCDs (observed, not promised): XCD x then owns the contiguous items
// [x per, x per + per) -- no XCD more than `per` of them, at most 7 workgroups of the launch without one -- and because
// `slots` is a multiple of 8 the riders do not shift the deal.  A per-pose partition cannot be even when `rows` does not
// divide by 8 (C2: 98 chunks = 7 XCDs x 13 + 1 x 7); a partition of the whole launch can.
//
// Item -> (row, pose), order 0: row = t / g, pose = t % g.  An XCD keeps a contiguous run of rows -- its points and image
// rows stay in its own L2 -- and walks all poses of a chunk back to back.  Order 1: pose = t / rows, row = t % rows.
// The partial row written is pose * rows + row in either order.
#pragma once
#include <stdint.h>

#include "ea_types.h"

namespace ea {

// one entry per row of a pose: the term that owns it, that term's first row, and the batch's problem count (the pose slot
// of (pose, term) is pose * count + group, and every entry carries `count` so that one 16-byte load answers everything)
struct PosesRow { int32_t term, row0, count, pad_; };

// the `shape` word of ea_eval_poses_kernel: bit 0 = XCD deal on, bit 1 = item order, bit 2 = a single term (no row table
// is read), bits 3.. = rider slots / 8
constexpr int kPosesXcd = 1, kPosesOrder1 = 2, kPosesSingle = 4;
EA_HD inline int poses_rider_slots(int riders) { return (riders + 7) & ~7; }
EA_HD inline int poses_shape(bool xcd, int order, bool single, int riders) {
  return (xcd ? kPosesXcd : 0) | (order ? kPosesOrder1 : 0) | (single ? kPosesSingle : 0) | poses_rider_slots(riders);
}
EA_HD inline int poses_shape_slots(int shape) { return shape & ~7; }
EA_HD inline int poses_per_xcd(int rows, int g) { return (rows * g + 7) >> 3; }
// workgroups of a launch
EA_HD inline unsigned poses_grid(int rows, int g, int riders) {
  return (unsigned)poses_rider_slots(riders) + 8u * (unsigned)poses_per_xcd(rows, g);
}

struct PosesWork {
  int kind;        // 0 = nothing, 1 = rider, 2 = evaluation item
  int rider;       // kind 1: which (pose, problem) of the previous launch
  int pose, row;   // kind 2: pose of this launch, row of that pose
};
EA_HD inline PosesWork poses_work(unsigned L, int shape, int rows, int g, int riders) {
  PosesWork w = {0, 0, 0, 0};
  const unsigned slots = (unsigned)poses_shape_slots(shape);
  if (L < slots) {
    if (L < (unsigned)riders) { w.kind = 1; w.rider = (int)L; }
    return w;
  }
  const unsigned e = L - slots;
  const int T = rows * g, per = poses_per_xcd(rows, g);
  const unsigned t = (shape & kPosesXcd) ? (e & 7u) * (unsigned)per + (e >> 3) : e;
  if ((e >> 3) >= (unsigned)per || t >= (unsigned)T) return w;
  w.kind = 2;
  if (shape & kPosesOrder1) { w.pose = (int)(t / (unsigned)rows); w.row = (int)(t % (unsigned)rows); }
  else { w.row = (int)(t / (unsigned)g); w.pose = (int)(t % (unsigned)g); }
  return w;
}
// kind 2 -> (term, chunk, pose slot, partial row); `table` is read unless the batch has a single term
struct PosesChunk { int term, chunk, slot, out_row; };
EA_HD inline PosesChunk poses_chunk(const PosesWork &w, int shape, int rows, const PosesRow *table) {
  PosesChunk c = {0, w.row, w.pose, w.pose * rows + w.row};
  if (!(shape & kPosesSingle)) {
    const PosesRow r = table[w.row];
    c.term = r.term; c.chunk = w.row - r.row0; c.slot = w.pose * r.count + r.term;
  }
  return c;
}
// rider r of a launch whose previous launch evaluated problems [0, count): pose r / count, problem r % count
EA_HD inline void poses_rider(int r, int count, int *pose, int *problem) { *pose = r / count; *problem = r % count; }

// K poses in launches of at most G: n = ceil(K / G) launches of ceil(K / n) poses, the last one takes the remainder
// (filling every launch to G can end on a launch of a few poses that costs a whole launch and fold of its own)
EA_HD inline int poses_launches(int K, int G) { return (K + G - 1) / G; }
EA_HD inline int poses_launch_size(int K, int G) { const int n = poses_launches(K, G); return (K + n - 1) / n; }

// ---- one pose per lane (ea_eval_poses_lanes_kernel) ---------------------------------------------------------------------
// The same launch with the mapping turned round: a work item is (row of a pose, GROUP of kPosesLanes consecutive poses of the
// launch), lane l of every wavefront of the workgroup holds pose 64 group + l, and the row's sums never leave the lane.  The
// list of items is the list above with `groups` in the place of g -- the XCD deal of contiguous rows and both item orders
// included; its launches carry no riders (riders = 0) -- so the functions above serve it unchanged; what is added is
// group -> (first pose, live lanes).  Its rows have a layout of their own and are folded inside the launch: further down.
constexpr int kPosesLanes = 64;
EA_HD inline int poses_lanes_groups(int g) { return (g + kPosesLanes - 1) / kPosesLanes; }
EA_HD inline unsigned poses_lanes_grid(int rows, int g, int riders) { return poses_grid(rows, poses_lanes_groups(g), riders); }
struct PosesLanesWork {
  int kind;         // 0 = nothing, 1 = rider, 2 = evaluation item
  int rider;        // kind 1
  int row;          // kind 2: row of a pose,
  int pose0, live;  //         first pose of the group and how many of its 64 lanes hold a pose of the launch (1..64)
};
EA_HD inline PosesLanesWork poses_lanes_work(unsigned L, int shape, int rows, int g, int riders) {
  const PosesWork w = poses_work(L, shape, rows, poses_lanes_groups(g), riders);
  PosesLanesWork o = {w.kind, w.rider, w.row, 0, 0};
  if (w.kind == 2) {
    o.pose0 = w.pose * kPosesLanes;
    o.live = g - o.pose0 < kPosesLanes ? g - o.pose0 : kPosesLanes;
  }
  return o;
}
// kind 2 -> (term, chunk of the term, problems in the batch); lane l's pose slot is (pose0 + l) * count + term
struct PosesLanesChunk { int term, chunk, count; };
EA_HD inline PosesLanesChunk poses_lanes_chunk(int row, int shape, const PosesRow *table) {
  PosesLanesChunk c = {0, row, 1};
  if (!(shape & kPosesSingle)) {
    const PosesRow r = table[row];
    c.term = r.term; c.chunk = row - r.row0; c.count = r.count;
  }
  return c;
}
// G of this path: the bound (rows memory, tuning cap) rounded down to whole groups -- a launch that is not the call's last
// leaves no lane idle -- and left alone below one group.  K poses then go in launches of G, the last takes the remainder:
// with few, long workgroups a launch costs about ceil(items / CUs) workgroup lifetimes, and full launches in front keep
// the sum of those at what one launch of K would cost (an even split can add a lifetime per launch).
EA_HD inline int poses_lanes_group_size(int bound) { return bound >= kPosesLanes ? bound - bound % kPosesLanes : (bound > 1 ? bound : 1); }
EA_HD inline int poses_lanes_launch_size(int K, int G) { return K < G ? K : G; }

// ---- the rows of the lanes path and their fold inside the launch (tests/poses_lanes_fold_host_shim.cpp) -----------------
// The lanes kernel keeps ONE row array, lane-minor: [group][row][slot][lane], kPosesLanesBlock doubles per (group, row) --
// slot s of the group's 64 poses is one 512-byte line, so the store of a row and every read of the fold are coalesced.
// The fold runs in the launch itself, in two levels of arrival counters ("tickets"); no workgroup waits for another.
//   level 1: the rows of problem i are cut into runs of kPosesRun consecutive rows, counted from the problem's first row.
//     An item adds one to the counter of its (group, problem, run); the workgroup whose add completes the run's row count
//     sums the run's rows in row order into one run partial (same lane-minor block) and adds one to the counter of
//     (group, problem).
//   level 2: the workgroup whose add completes the problem's run count sums the run partials in run order, writes the 64
//     results and raises the flag of (group of the call, problem).
// A pose's sums therefore depend on the pose and the problem's row count only.
// Run partials and level-1 counters are addressed by a run SLOT that needs no table: problem i's run r of a batch whose
// problem i starts at row row0 has slot row0 / kPosesRun + i + r.  Slots of different (problem, run) never collide
// (ceil(n / R) <= floor((a + n) / R) - floor(a / R) + 1) and stay below poses_lanes_run_slots(rows, count).
constexpr int kPosesRun = 16;
constexpr int kPosesLanesBlock = kAccSlots * kPosesLanes;  // doubles of one (group, row) or one run partial
EA_HD inline int poses_lanes_run(int chunk) { return chunk / kPosesRun; }                            // chunk = row - row0
EA_HD inline int poses_lanes_runs(int nrows) { return (nrows + kPosesRun - 1) / kPosesRun; }           // level-2 ticket target
EA_HD inline int poses_lanes_run_rows(int nrows, int run) {                                           // level-1 ticket target
  const int left = nrows - run * kPosesRun;
  return left < kPosesRun ? left : kPosesRun;
}
EA_HD inline int poses_lanes_run_slots(int rows, int count) { return rows / kPosesRun + count; }      // per group
EA_HD inline int poses_lanes_run_slot(int row0, int problem, int run) { return row0 / kPosesRun + problem + run; }
// offsets in doubles of a block's first word; word (slot s, lane l) of a block is at s * kPosesLanes + l
EA_HD inline size_t poses_lanes_row_off(int group, int row, int rows) { return ((size_t)group * (size_t)rows + (size_t)row) * kPosesLanesBlock; }
EA_HD inline size_t poses_lanes_partial_off(int group, int run_slot, int rows, int count) {
  return ((size_t)group * (size_t)poses_lanes_run_slots(rows, count) + (size_t)run_slot) * kPosesLanesBlock;
}
// counters of a launch of `groups` groups, one block of 32-bit words zeroed ahead of the launch:
// [level 1: groups x run slots | level 2: groups x count], padded to a multiple of 16 bytes
EA_HD inline size_t poses_lanes_counter1(int group, int run_slot, int rows, int count) {
  return (size_t)group * (size_t)poses_lanes_run_slots(rows, count) + (size_t)run_slot;
}
EA_HD inline size_t poses_lanes_counter2(int groups, int group, int problem, int rows, int count) {
  return (size_t)groups * (size_t)poses_lanes_run_slots(rows, count) + (size_t)group * (size_t)count + (size_t)problem;
}
EA_HD inline size_t poses_lanes_counters(int groups, int rows, int count) {
  return ((size_t)groups * (size_t)(poses_lanes_run_slots(rows, count) + count) + 3) & ~(size_t)3;
}
// flags in pinned memory, one per (group of the CALL, problem): launch j of a call in launches of G poses starts at group
// j * poses_lanes_groups(G)
EA_HD inline size_t poses_lanes_flag(int call_group, int problem, int count) { return (size_t)call_group * (size_t)count + (size_t)problem; }
EA_HD inline int poses_lanes_call_groups(int K, int G) {
  const int full = K / G, rest = K % G;
  return full * poses_lanes_groups(G) + poses_lanes_groups(rest);
}

}  // namespace ea
