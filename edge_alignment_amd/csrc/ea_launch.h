// ea_launch.h — what the library's translation units call in one another, each function declared once: the kernel
// launchers of ea_kernels.hip / ea_kernels_var.hip / ea_preprocess.hip and the functions ea_capi.hip keeps for ea_comm.hip.
// The defining files include it too: an extern "C" definition that drifts from its declaration here does not compile (a
// hand-copied prototype in the caller would have linked and passed garbage); a drifted launcher fails to link, as before.
// What a launcher takes is a struct filled by name plus what varies per call: no list of look-alike ints in which two swapped
// arguments would still compile.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/ea_hip.h"
#include "ea_depth_gate.h"
#include "ea_point_select.h"
#include "ea_point_merge.h"
#include "ea_lm.h"
#include "ea_reproject.h"
#include "ea_select.h"
#include "ea_types.h"

namespace ea {
// What is fixed about the launches of the fused evaluation family (ea_eval_fused / _poses / _fold / ea_lm_iter kernels) once
// a batch is built: the launch shape and the preloaded arguments.  Filled by name (ea_capi.hip: eval_launch); the launchers
// refuse a (dtype, ppt, nt, ...) combination no kernel is compiled for with hipErrorInvalidValue.
struct EvalLaunch {
  int dtype = 0;             // EA_F64 / EA_F32
  int ppt = 1, nt = 256;     // points per lane {1, 2, 4}, workgroup size {256, 1024}
  int variant = 0;           // distortion / second-camera / weighted terms (the kernels of ea_kernels_var.hip)
  int weighted = 0;          // some term carries per-point weights (variant bit 2): the weighted kernels of that file
  int chunk = 256;           // points per workgroup = nt * ppt
  int max_chunks = 0;        // workgroups of the widest term
  int xcd_remap = 1;
  int lds_bytes = 0;         // > 0: the DT footprint is staged through LDS (MODE 1)
  int wide = 0;              // fp32 sums in fp64 from the lane's sum on (MODE 2)
  int terms_are_groups = 1;  // one term per problem
  int buffer_loads = 0;      // raw-buffer addressing of image and points
  int img32 = 0;             // fp64 arithmetic over the fp32 mirror of the image
  const void *x0 = nullptr, *y0 = nullptr, *z0 = nullptr;  // problem 0's points and their count
  int n0 = 0;
};
// the fold that rides in an evaluation's launch: the previous step's rows into its result slots
struct RidingFold { const GroupDesc *groups; const double *prev_rows; EvalOut *prev_out; };
// a launch of ea_eval_poses_kernel: g poses x `rows` partial rows per pose; order: 0 = an XCD walks the poses of a row back to
// back, 1 = the rows of a pose; single: one term in the batch (no row table is read); exchange: the wave-exchange reduction
// (fp64 in 256-lane workgroups only; ea_wave_exchange.h)
struct PosesLaunch { int g = 0, rows = 0, order = 0, single = 0, exchange = 0; };
// What the folds of the pose-batched path work on: `n` results (pose-major: result r = pose r / count, problem r % count)
// whose rows lie in `rows` (pose p's at p * rows_per_pose + the problem's range in `groups`, the group table in the pose
// path's own chunking), folded into out[r]; counter / host_flag / seq: the completion signal of ea_reduce_done_kernel.
struct PosesFold {
  int n = 0, count = 1, rows_per_pose = 0, seq = 0;
  const GroupDesc *groups = nullptr;
  const double *rows = nullptr;
  EvalOut *out = nullptr;
  unsigned int *counter = nullptr;
  int *host_flag = nullptr;
};
// What the fold inside a launch of ea_eval_poses_lanes_kernel works on (ea_poses_map.h, "the rows of the lanes path"): the
// run partials and the counters of the launch's groups (zeroed ahead of the launch), the results out[pose * count + problem]
// of the launch's poses, and the pinned flags of the call -- the launch's first group is group0 of the call -- raised to seq.
// on = 0: evaluations only, the rows are stored and nothing is counted or folded.
struct PosesTickets {
  int on = 0, count = 1, group0 = 0, seq = 0;
  double *partials = nullptr;
  unsigned int *counters = nullptr;
  EvalOut *out = nullptr;
  int *flags = nullptr;
};
// the LM state an ea_lm_step_kernel / ea_lm_iter_kernel launch works on; `side`: the side table (PriorDesc records: NormalPriors and the constant-coordinate mask) sits behind the
// launch's `groups` (one per problem) -- some problem carries a NormalPrior or holds tangent coordinates constant
struct LMLaunch {
  PoseState *poses; LMState *states; LMCold *cold; LMTrace *traces;
  const LMOptions *opt;
  int *progress;
  LMState *host_states; LMTrace *host_traces;
  GroupDesc first;
  int post_done, side;
};
// what ea_lm_iter_kernel adds: launch j reads what launch j - 1 wrote and writes the other buffer of each pair (the `out`
// buffers take the place of LMLaunch::states / cold, which the launcher does not read)
struct LMIterPairs {
  const double *rows_in; double *rows_out;
  const LMState *st_in; LMState *st_out;
  const LMCold *cold_in; LMCold *cold_out;
};
// A multi-start solve (ea_batch_solve_starts, ea_starts_map.h): what the (evaluate, step) pair of one piece of the live list
// works on.  Every array is slot-major (slot = start * count + problem); live_in / n_in: the list of this iteration,
// live_out / n_out: the one the iteration's last step launch (`last`) rebuilds for the next; alive[start]: problems of the
// start still running; counter / host_word: the last arrival's count and the word it posts; traces / host_traces: nullable.
struct StartsStep {
  const GroupDesc *groups;  // row ranges in the pose path's chunking
  const GroupDesc *side;    // the batch's own group table, side table behind it (SIDE instantiations)
  const double *rows;
  PoseState *poses; LMState *states; LMCold *cold; LMTrace *traces;
  LMState *host_states; LMTrace *host_traces;
  const int *live_in, *n_in;
  int *live_out, *n_out, *alive;
  unsigned int *counter;
  unsigned long long *host_word;
  int count, rows_per_pose, off, last;
  unsigned iteration, tag;
};
// The device workspace of one quantile call (ea_select.h): nseg segments of the key array, nq quantiles each, max_n = the
// longest segment.  n_valid and hist are ONE range of clear_bytes bytes ([n_valid x nseg, padded | hist]) zeroed up front;
// prefix / rank: nseg x nq, written by the scans; out_values: nseg x nq, out_n_valid: nseg.
struct SelectWork {
  int nseg = 0, nq = 0, max_n = 0;
  const SelectSeg *segs = nullptr;
  const double *probs = nullptr;
  uint64_t *keys = nullptr;
  unsigned *n_valid = nullptr, *hist = nullptr;
  size_t clear_bytes = 0;
  uint64_t *prefix = nullptr;
  int64_t *rank = nullptr;
  double *out_values = nullptr;
  int64_t *out_n_valid = nullptr;
};
// The batched frame producers (ea_batch_set_frames): the frame is blockIdx.z of every launch.  What lies in the producers'
// workspace is addressed as `pointer for frame 0` + z * stride bytes (the batch owns n consecutive frame_ws(H, W) layouts,
// stride = frame_ws(H, W).total, a multiple of 256 -- or frame_stage(...).total where the ROS call's halving stage follows
// each frame's workspace); what the problems or the caller own comes out of a device table with one FrameSlot per frame.
struct FrameSlot {
  const uint8_t *bgr[2];  // the colour frame of the reference ([0]) / current ([1]) side: the workspace's copy of a host
                          // frame, or the caller's device frame read in place
  const uint16_t *depth;  // likewise (NULL in ea_batch_set_frames_ros, whose count keeps every edge pixel)
  const uint8_t *mask;    // likewise: the current side's mask of ea_batch_set_frames_canny (NULL without one)
  const float *depth_f32; // ea_batch_set_frames_ros: the reference side's depth in metres at the working resolution
  void *x, *y, *z, *w;    // the problem's point arrays and its weights (problem dtype), room for `capacity` points
  void *dt;               // the problem's padded DT image and, for an fp64 problem, its float32 mirror (else NULL)
  float *dt32;
  double fx, fy, cx, cy;  // the problem's camera
  double z_ref;           // ea_problem_set_depth_weighting
  int power;              // (0 = off)
  int capacity;           // = the frame's point count
  int pitch;              // of dt / dt32, in texels
  int ones;               // != 0: a frame without depth weighting (power 0) gets weights of exactly 1 (the gated tracker)
};
struct FramesLaunch {
  int n = 0, H = 0, W = 0;
  size_t stride = 0;
  const FrameSlot *slots = nullptr;  // device
};
// launch_halving_chain_*: where each step of one launch leaves its level (NULL: nowhere)
constexpr int kChainSteps = 3;
struct ChainLevels {
  void *dst[kChainSteps] = {nullptr, nullptr, nullptr};
};
struct RowsLaunch {
  int dtype = 0, variant = 0, buffer_loads = 0, img32 = 0;
  int layout = 0;   // 0 = J row-major [rows][6], 1 = column-major [6][rows]
  int staged = 0;   // (layout 0 only)
  int corrected = 0, nontemporal = 0;
  long long max_n = 0, total_rows = 0;
};

// ea_kernels.hip
hipError_t launch_eval_fused(const EvalLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses, double *partials,
                             hipStream_t stream);
// the same launch under the kernel name ea_eval_poses_grid_kernel: G poses x terms in grid y over tables replicated G times
// (the pose-batched launches of variant functors, LDS staging, wide_accumulate and terms that share a pose)
hipError_t launch_eval_poses_grid(const EvalLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses,
                                  double *partials, hipStream_t stream);
// ea_eval_poses_kernel: the flat, XCD-balanced launch of g poses with the previous launch's fold riding in front; `probs`
// has the batch's row table (PosesRow x rows, ea_poses_map.h) right in front of it
hipError_t launch_eval_poses(const EvalLaunch &s, const PosesLaunch &p, const ProblemDesc *probs, const PoseState *poses,
                             double *partials, const PosesFold &fold, hipStream_t stream);
// ea_eval_poses_lanes_kernel: that launch with one pose per lane (ea_poses_map.h: items are (row, 64 poses)); fp64 batches at
// the 256 x 2 pose shape, the same tables and items; its rows are lane-minor and folded in the launch itself (PosesTickets:
// the launcher zeroes the counters ahead of the kernel); p.exchange is not read
hipError_t launch_eval_poses_lanes(const EvalLaunch &s, const PosesLaunch &p, const ProblemDesc *probs, const PoseState *poses,
                                   double *rows, const PosesTickets &tickets, hipStream_t stream);
hipError_t launch_poses_fold(int nt, const PosesFold &fold, hipStream_t stream);
// ea_cost_poses_kernel: the cost-only form of launch_eval_poses' launch (256-lane workgroups; no riders) -- one narrow
// partial {cost, failed functors} of kCostPartialBytes per workgroup at pose * rows + row of `partials`.
// ea_cost_fold_kernel: fold.n results out of them (fold.rows = the narrow partials), {cost, n_invalid} into the cost and
// invalid slots of fold.out[r], the flag raised to fold.seq.
constexpr size_t kCostPartialBytes = 16;
hipError_t launch_cost_poses(const EvalLaunch &s, const PosesLaunch &p, const ProblemDesc *probs, const PoseState *poses,
                             void *partials, hipStream_t stream);
hipError_t launch_cost_fold(const PosesFold &fold, hipStream_t stream);
// ea_eval_starts_kernel: the poses live[off .. off + p.g) of a multi-start solve, as ea_eval_poses_kernel evaluates them,
// without riders; positions from *n_live on return at once.  ea_lm_step_starts_kernel: g x a.count workgroups.
hipError_t launch_eval_starts(const EvalLaunch &s, const PosesLaunch &p, const ProblemDesc *probs, const PoseState *poses,
                              double *partials, const int *live, const int *n_live, int off, hipStream_t stream);
hipError_t launch_lm_step_starts(int g, const StartsStep &a, const LMOptions &lo, int side, hipStream_t stream);
hipError_t launch_pixel_cost(int dtype, const ProblemDesc *probs, int problem, int n, const PoseState *poses, void *partials,
                             hipStream_t stream);
hipError_t launch_eval_rows(const RowsLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses, void *r_out,
                            void *J_out, unsigned int *n_invalid, hipStream_t stream);
hipError_t launch_eval_points(int dtype, const ProblemDesc *probs, int problem, int n, const PoseState *poses,
                              double *r_out, double *J_out, int corrected, hipStream_t stream);
hipError_t launch_reduce(const GroupDesc *groups, int count, const double *partials, EvalOut *out,
                         hipStream_t stream);
hipError_t launch_reduce_done(const GroupDesc *groups, int count, const double *partials, EvalOut *out, unsigned int *counter,
                              int *host_flag, int seq, hipStream_t stream);
hipError_t launch_eval_fold(const EvalLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses, double *partials,
                            const RidingFold &fold, hipStream_t stream);
hipError_t launch_reduce_nt(int nt, const GroupDesc *groups, int count, const double *partials, EvalOut *out,
                            hipStream_t stream);
hipError_t launch_lm_step(const GroupDesc *groups, int count, const double *partials, const LMLaunch &lm, hipStream_t stream);
hipError_t launch_lm_iter(const EvalLaunch &s, const ProblemDesc *probs, int count, const GroupDesc *groups, const LMLaunch &lm,
                          const LMIterPairs &io, hipStream_t stream);
hipError_t launch_pad_image(int dtype, const void *src, int H, int W, void *dst, int pitch, float *dst32, int *inexact,
                            hipStream_t stream);
hipError_t launch_make_poses(const double *qt, int n, int count, const ProblemDesc *probs, const GroupDesc *groups,
                             PoseState *out, hipStream_t stream);
hipError_t launch_grid_to_image(int dtype, const double *grid, int W, int H, void *dst, int pitch, float *dst32, int *inexact,
                                hipStream_t stream);
hipError_t launch_aos_to_soa(int dtype, const double *src, long long n, int stride, void *x, void *y, void *z, hipStream_t stream);
// ea_store_weights_kernel: dst[i] = src[order ? order[i] : i] in the problem dtype, src doubles or the problem dtype;
// ea_depth_weights_kernel: w[i] = min(1, (z_ref / z[i])^power), fp64 from the stored z, rounded once
hipError_t launch_store_weights(int dtype, int src_is_double, const void *src, const int32_t *order, long long n, void *dst,
                                hipStream_t stream);
hipError_t launch_depth_weights(int dtype, const void *z, long long n, double z_ref, int power, void *w, hipStream_t stream);
// ea_select_*_kernel (ea_select.h): launch_select_clear zeroes the counts, one of the two key passes fills w.keys,
// launch_select queues the six (histogram, scan) pairs; the first scan counts the valid blocks, the last writes out_values /
// out_n_valid
hipError_t launch_select_clear(const SelectWork &w, hipStream_t stream);
hipError_t launch_select_keys(int dtype, const SelectWork &w, const ProblemDesc *probs, const PoseState *poses, hipStream_t stream);
hipError_t launch_select_keys_values(const SelectWork &w, const double *values, hipStream_t stream);
hipError_t launch_select(const SelectWork &w, hipStream_t stream);
// ea_pose_stats_kernel + ea_pose_stats_fold_kernel: w.nseg segments (begin = first partial row, pose_stats_rows(n) of them),
// w.max_n the longest; one PoseStatsRow per segment into w.out
struct PoseStatsWork {
  int nseg = 0, max_n = 0;
  int margin = 0;
  double inlier_residual = 0.0;
  const SelectSeg *segs = nullptr;
  PoseStatsPartial *partials = nullptr;
  PoseStatsRow *out = nullptr;
};
hipError_t launch_pose_stats(int dtype, const PoseStatsWork &w, const ProblemDesc *probs, const PoseState *poses, hipStream_t stream);
// ea_reproject_kernel (ea_reproject.h): w.nseg segments, w.max_n the longest.  paint == 0: (u, v) of point i of a segment
// into uv[2 * (row + i)]; paint != 0: the segments' images painted with `color` (b | g << 8 | r << 16) and counts[2 * seg +
// {0, 1}] += {inside, outside} (zero before the launch)
struct ReprojectWork {
  int nseg = 0, max_n = 0, paint = 0;
  unsigned int color = 0;
  const ReprojectSeg *segs = nullptr;
  double *uv = nullptr;
  unsigned long long *counts = nullptr;
};
hipError_t launch_reproject(int dtype, const ReprojectWork &w, const ProblemDesc *probs, hipStream_t stream);
// ea_depth_gate_kernel (ea_depth_gate.h): w.nseg segments, w.max_n the longest, the depth images of one kind (EA_DEPTH_*) and
// the window radius 0..3; counts[6 * seg + class] += the segment's points of that class (zero before the launch)
struct DepthGateWork {
  int nseg = 0, max_n = 0, kind = 0, radius = 0;
  DepthGateRule rule = {};
  const DepthGateSeg *segs = nullptr;
  unsigned long long *counts = nullptr;
};
hipError_t launch_depth_gate(int dtype, const DepthGateWork &w, const ProblemDesc *probs, hipStream_t stream);
// ea_point_select_*_kernel (ea_point_select.h): w.nseg segments, w.max_n the longest.  cell_px > 0: `tables` (every segment's
// cell tables, table_bytes in all) is set to all ones, then the key pass(es); then count, scan and compaction.  out[seg]: zero
// before the launch; stride and target as the rule has them, clamped to 2^31 - 1 (target 0: off)
struct PointSelectWork {
  int nseg = 0, max_n = 0, cell_px = 0, nearest = 0, outside = 0;
  unsigned int stride = 1, target = 0;
  const PointSelectSeg *segs = nullptr;
  PointSelectOut *out = nullptr;
  void *tables = nullptr;
  size_t table_bytes = 0;
};
hipError_t launch_point_select(int dtype, const PointSelectWork &w, hipStream_t stream);
// ea_point_transform_kernel (ea_point_merge.h): nseg segments, max_n the longest; every segment's points rewritten in place
hipError_t launch_point_transform(int dtype, const PointTransformSeg *segs, int nseg, int max_n, hipStream_t stream);
// ea_point_merge_*_kernel (ea_point_merge.h): w.nseg segments, max_dst / max_src the longest dst and src (max_src >= 1).
// cell_px > 0: `tables` (every segment's occupancy bytes and cell tables, table_bytes in all) is set to all ones, then the
// occupancy pass over the dst points and the key pass(es) over the src points; then count, scan (ea_point_select_scan_kernel on
// scan_segs, whose n and block_counts are the segments' n_src and block_counts: its total is the survivors) and the copy.
// out[seg], scan_out[seg]: zero before the launch; cap: max_carried clamped to 2^31 - 1 (0: off)
struct PointMergeWork {
  int nseg = 0, max_dst = 0, max_src = 0, need_pixel = 0, margin = 0, cell_px = 0, nearest = 0;
  double max_dt = -1.0, weight_scale = 1.0;
  unsigned int cap = 0;
  const PointMergeSeg *segs = nullptr;
  PointMergeOut *out = nullptr;
  const PointSelectSeg *scan_segs = nullptr;
  PointSelectOut *scan_out = nullptr;
  void *tables = nullptr;
  size_t table_bytes = 0;
};
hipError_t launch_point_merge(int dtype, const PointMergeWork &w, hipStream_t stream);
hipError_t launch_selftest_reduce(const float *in, float *a, float *b, float *c, float *d, double *o32, double *o64,
                                  hipStream_t stream);
// ea_kernels_var.hip (the same file under -DEA_TU_VARIANT): what launch_eval_fused (tag 0) / launch_eval_poses_grid (tag 1) hand on
// when s.variant is set
hipError_t launch_eval_fused_var(int tag, const EvalLaunch &s, const ProblemDesc *probs, int nterms, const PoseState *poses,
                                 double *partials, hipStream_t stream);
hipError_t launch_empty(int grid, int block, hipStream_t stream);
#ifdef EA_STAMPS
hipError_t set_stamp_buffer(unsigned long long *buf);
hipError_t set_lm_stamp_buffer(unsigned long long *buf);
#endif
// ea_preprocess.hip
hipError_t launch_resize_half_bgr8(const uint8_t *src, int H, int W, uint8_t *dst, hipStream_t s);
hipError_t launch_resize_half_f32(const float *src, int H, int W, float *dst, int nan_to_zero, hipStream_t s);
hipError_t launch_nan_to_zero(float *img, size_t n, hipStream_t s);
hipError_t launch_edge_strength(const uint8_t *bgr, int H, int W, uint8_t *gray, uint8_t *lap, hipStream_t s);
hipError_t launch_threshold_median(const uint8_t *lap, int H, int W, int thr, int median, uint8_t *mask, hipStream_t s);
hipError_t launch_chamfer(const uint8_t *mask, int H, int W, int *G, int *scratch, int *dist_fix, float *dist_f32,
                          unsigned int *minmax, hipStream_t s);
hipError_t launch_canny(const uint8_t *bgr, int H, int W, int low, int high, int l2_bgr, const uint8_t *keep, uint8_t *gray,
                        int *mag, uint8_t *dir, uint8_t *label, uint8_t *edges, uint8_t *inv, int *changed, int *rounds_out,
                        hipStream_t s);
hipError_t launch_edge_scatter_ros(int dtype, const uint8_t *edges, const float *depth, int H, int W, const int *block_offsets,
                                   double fx, double fy, double cx, double cy, void *X, void *Y, void *Z, int capacity,
                                   hipStream_t s);
hipError_t launch_dt_store(int dtype, const int *dist_fix, const float *dist_f32, int H, int W, const unsigned int *minmax,
                           int normalize, double lo, double hi, void *dst, int pitch, float *plain, float *dst32, hipStream_t s);
hipError_t launch_gate_by_mask(uint8_t *grad, const uint8_t *mask, int H, int W, hipStream_t s);
hipError_t launch_edge_count_scan(const uint8_t *lap, const uint16_t *depth, int H, int W, int thr, int *block_counts,
                                  int *total, hipStream_t s);
hipError_t launch_edge_scatter(int dtype, const uint8_t *lap, const uint16_t *depth, int H, int W, int thr,
                               const int *block_offsets, double fx, double fy, double cx, double cy, double z_scaling,
                               void *X, void *Y, void *Z, int capacity, hipStream_t s);
// The same steps for f.n frames in one launch each (grid z = frame; the kernels run the per-frame kernels' bodies).  Workspace
// pointers are frame 0's; side: 0 = the reference frames' colour source, 1 = the current frames'.  The counts' layout is
// launch_edge_count_scan's per frame: the total behind the per-block counts, at f.stride bytes from its neighbour's.
hipError_t launch_edge_strength_frames(const FramesLaunch &f, int side, uint8_t *gray, uint8_t *lap, hipStream_t s);
hipError_t launch_threshold_median_frames(const FramesLaunch &f, const uint8_t *lap, int thr, int median, uint8_t *mask, hipStream_t s);
// (dist_f32 given: the exact Euclidean row pass into it, as in launch_chamfer, skipping the frames whose slot has no image)
hipError_t launch_chamfer_frames(const FramesLaunch &f, const uint8_t *mask, int *G, int *scratch, int *dist_fix, float *dist_f32,
                                 unsigned int *minmax, hipStream_t s);
hipError_t launch_dt_store_frames(int dtype, const FramesLaunch &f, const int *dist_fix, const unsigned int *minmax, int normalize,
                                  double lo, double hi, hipStream_t s);
hipError_t launch_edge_count_scan_frames(const FramesLaunch &f, const uint8_t *lap, int thr, int *block_counts, hipStream_t s);
hipError_t launch_edge_scatter_frames(int dtype, const FramesLaunch &f, const uint8_t *lap, int thr, const int *block_offsets,
                                      double z_scaling, hipStream_t s);
// launch_canny's chain (blur 3x3 -> gray -> Canny(low, high) [-> AND mask > 1, `masked`]) for f.n frames: every frame's edge
// map in its `edges`, the inverse in its `inv`.  changed: frame 0's 16 flag ints (kCannyFrameFlags of them travel per look);
// h_flags: f.n x kCannyFrameFlags ints of pinned memory, into which one strided copy brings every frame's flags per look.  The
// hysteresis converges per frame; the loop ends when every frame has had a quiet launch.  Waits for `s`; *looks: how many
// looks at the flags it took.
constexpr int kCannyFrameFlags = 8;
// l2_bgr != 0: launch_canny's ROS flavour (no blur / gray, (low, high) already squared).
hipError_t launch_canny_frames(const FramesLaunch &f, int side, int masked, int low, int high, int l2_bgr, uint8_t *gray, int *mag,
                               uint8_t *dir, uint8_t *label, uint8_t *edges, uint8_t *inv, int *changed, int *h_flags, int *looks,
                               hipStream_t s);
// The ROS chain's own steps for f.n frames (ea_batch_set_frames_ros; the ea_<step>_stack_kernel forms).  The store reads the
// float distance of the exact transform and skips the frames whose slot has no image; the scatter takes camera, point arrays,
// capacity and the float depth (depth_f32) from the slot.  The halving steps: H, W = the extent of the step's SOURCE; frame
// z's source is table[z] (device memory: f.n device pointers, the caller's frames read in place) where a table is given, else
// src + z * f.stride; its destination dst + z * f.stride.
hipError_t launch_dt_store_stack(int dtype, const FramesLaunch &f, const float *dist_f32, const unsigned int *minmax, int normalize,
                                 double lo, double hi, hipStream_t s);
hipError_t launch_edge_scatter_ros_stack(int dtype, const FramesLaunch &f, const uint8_t *edges, const int *block_offsets, hipStream_t s);
hipError_t launch_resize_half_bgr8_stack(const FramesLaunch &f, const uint8_t *const *table, const uint8_t *src, int H, int W,
                                         uint8_t *dst, hipStream_t s);
hipError_t launch_resize_half_f32_stack(const FramesLaunch &f, const float *const *table, const float *src, int H, int W, float *dst,
                                        int nan_to_zero, hipStream_t s);
// The halving chain (ea_batch_set_frames_ros_pyramid): `steps` (1..kChainSteps) successive halvings of f.n frames of H x W
// pixels (both multiples of 2^steps) from one read of the source, which is named as for the stack launchers above.  lv.dst[k]:
// frame 0's pointer for the level step k produces, (H >> (k + 1)) x (W >> (k + 1)), frame z's at z * f.stride bytes from it;
// NULL = the level is passed through in LDS and never written.  The last step's level is always written.  Every level is,
// bit for bit, what k + 1 launches of the stack launchers leave (NaN -> 0, where asked for, on the source only).  f: n and
// stride only.
hipError_t launch_halving_chain_bgr8(const FramesLaunch &f, const uint8_t *const *table, const uint8_t *src, int H, int W, int steps,
                                     const ChainLevels &lv, hipStream_t s);
hipError_t launch_halving_chain_f32(const FramesLaunch &f, const float *const *table, const float *src, int H, int W, int steps,
                                    const ChainLevels &lv, int nan_to_zero, hipStream_t s);
// ea_kernels.hip: ea_depth_weights_kernel's body for the frames whose slot has power > 0 (and ones for those with `ones`),
// max_n = the largest capacity among them
hipError_t launch_depth_weights_frames(int dtype, const FramesLaunch &f, long long max_n, hipStream_t s);
}  // namespace ea

// ea_capi.hip, for the library's other translation units (ea_comm.hip): the thread-local error message, a batch's stream,
// the point-sharded solve in the one-launch-per-iteration form
extern "C" int ea_internal_fail(int code, const char *msg);
extern "C" void *ea_internal_batch_stream(ea_batch *b, int *device);
extern "C" int ea_internal_solve_sharded_rows(ea_problem *p, const ea_options *opt, ea_device_allreduce_fn allreduce,
                                              int (*agree)(int vals[2], void *user), void *user, double q[4], double t[3],
                                              ea_summary *summary, int *used);
