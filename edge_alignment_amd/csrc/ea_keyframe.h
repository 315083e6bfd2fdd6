// ea_keyframe.h — the keyframe rule of the multi-stream tracker (ea_tracker_batch_set_keyframes) as a pure host function:
// what ea_frames.hip calls after the solves of a push, and what tests/keyframe_host_shim.cpp sweeps without a device.
#pragma once
#include <stdint.h>

#include "../../include/ea_hip.h"

namespace ea {

// NaN fields, a negative margin and a negative inlier_residual (which the statistics call would refuse) are refused
// (ea_tracker_batch_set_keyframes: EA_ERR_INVALID_ARG)
inline bool keyframe_params_ok(const ea_keyframe_params &p) {
  return p.min_visible_fraction == p.min_visible_fraction && p.min_inlier_fraction == p.min_inlier_fraction &&
         p.inlier_residual >= 0.0 && p.max_mean_flow == p.max_mean_flow && p.margin >= 0;
}

// The reason mask of one stream after a push; 0 = the keyframe is kept.  age: the frames solved against the keyframe, this
// one included.  The comparisons are the ones written beside ea_keyframe_params' fields, each with one IEEE multiplication.
inline int keyframe_decide(const ea_pose_stats &s, const ea_keyframe_params &p, int age, bool aligned, bool failed) {
  if (!aligned) return EA_KEY_FIRST;
  if (failed) return EA_KEY_SOLVE_FAILED;
  int why = 0;
  if (p.min_visible_fraction > 0.0 && (double)s.n_visible < p.min_visible_fraction * (double)s.n) why |= EA_KEY_VISIBLE;
  if (p.min_inlier_fraction > 0.0 && (double)s.n_inlier < p.min_inlier_fraction * (double)s.n) why |= EA_KEY_INLIERS;
  if (p.max_mean_flow > 0.0 && s.n_flow > 0 && s.sum_flow > p.max_mean_flow * (double)s.n_flow) why |= EA_KEY_FLOW;
  if (p.max_frames > 0 && age >= p.max_frames) why |= EA_KEY_AGE;
  return why;
}

}  // namespace ea
