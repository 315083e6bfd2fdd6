// ea_starts_map.h — the live list of a multi-start solve (ea_batch_solve_starts: K trust-region runs per problem in lock-step),
// as pure functions the kernels and the host share; the host sizes its grids with them and tests them without a device
// (tests/starts_map_host_shim.cpp).
//
// K starts of a batch of `count` problems; (start, problem) owns the slot start * count + problem of the pose / state / cold /
// trace arrays -- the layout of ea_batch_eval_poses.  The LIVE LIST holds, in ascending order, the starts that still have a
// running problem; n_live is its length.  An iteration walks the list in pieces of at most G positions, one (evaluate, step)
// launch pair per piece: the pair of piece [off, off + g) evaluates position off + pose of the list for pose < g into the
// partial rows pose * rows + row (ea_poses_map.h deals the (row, pose) items over the XCDs), and one step workgroup per
// (pose, problem) folds them.  The host sizes a piece from the last n_live it has SEEN, which is never smaller than the one
// the launch finds on the device: a position >= n_live has nothing to do.  The last workgroup of an iteration's last step
// launch rebuilds the list, order-preserving, into the other buffer of the pair (parity of the iteration) and posts
// {call tag, iterations complete, n_live} to the host as ONE 64-bit word.
#pragma once
#include <stdint.h>

#include "ea_poses_map.h"

namespace ea {

constexpr int kMaxStartSlots = 16384;  // K * count of one call

// evaluation item (pose of the piece, row) -> what it evaluates: `start` = live[off + pose], read by the caller once
// off + pose < n_live is known
EA_HD inline bool starts_position_live(int off, int pose, int n_live) { return off + pose < n_live; }
EA_HD inline PosesChunk starts_chunk(const PosesWork &w, int start, int shape, int rows, const PosesRow *table) {
  PosesChunk c = {0, w.row, start, w.pose * rows + w.row};
  if (!(shape & kPosesSingle)) {
    const PosesRow r = table[w.row];
    c.term = r.term; c.chunk = w.row - r.row0; c.slot = start * r.count + r.term;
  }
  return c;
}
// workgroup of a step launch -> (pose of the piece, problem); its slot is live[off + pose] * count + problem and its rows
// are pose * rows + the problem's range
EA_HD inline void starts_step_item(unsigned block, int count, int *pose, int *problem) {
  *pose = (int)(block / (unsigned)count); *problem = (int)(block % (unsigned)count);
}
EA_HD inline unsigned starts_step_grid(int g, int count) { return (unsigned)g * (unsigned)count; }

// the pieces of an iteration over n (possibly stale) live positions: ceil(n / G) pairs of ceil(n / pairs) positions, the
// last one takes the remainder (poses_launch_size)
EA_HD inline int starts_pairs(int n, int G) { return poses_launches(n, G); }
EA_HD inline int starts_piece(int n, int G) { return poses_launch_size(n, G); }

// Order-preserving compaction by a workgroup of 256 lanes = 4 wavefronts, a round per 256 positions: wavefront w publishes
// the 64-bit mask of its lanes whose start stays live; the entry of (wave, lane) lands behind the `before` entries kept in
// earlier rounds, those of the lower wavefronts and those of the lower lanes of its own.
EA_HD inline int starts_popc(uint64_t m) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __popcll(m);
#else
  return __builtin_popcountll(m);
#endif
}
EA_HD inline int starts_compact_slot(const uint64_t masks[4], int wave, int lane, int before) {
  int s = before;
  for (int w = 0; w < 4; ++w)
    if (w < wave) s += starts_popc(masks[w]);
  return s + starts_popc(masks[wave] & (((uint64_t)1 << lane) - 1));
}
EA_HD inline int starts_compact_kept(const uint64_t masks[4]) {
  return starts_popc(masks[0]) + starts_popc(masks[1]) + starts_popc(masks[2]) + starts_popc(masks[3]);
}

// the word the host polls: n_live in bits 0..14, iterations complete in bits 15..46, the call's tag in bits 47..63 (a
// launch the previous call left queued posts under the previous tag: the host does not take it for its own)
EA_HD inline uint64_t starts_word(unsigned tag, unsigned iteration, int n_live) {
  return ((uint64_t)(tag & 0x1ffffu) << 47) | ((uint64_t)iteration << 15) | (uint64_t)(unsigned)n_live;
}
EA_HD inline bool starts_word_read(uint64_t w, unsigned tag, int *iteration, int *n_live) {
  if ((unsigned)(w >> 47) != (tag & 0x1ffffu)) return false;
  *iteration = (int)((w >> 15) & 0xffffffffu); *n_live = (int)(w & 0x7fffu);
  return true;
}
static_assert(kMaxStartSlots < (1 << 15), "n_live field of starts_word");

}  // namespace ea
