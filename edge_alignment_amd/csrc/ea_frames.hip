// ea_frames.hip — the host side of everything that starts from raw frames: the frame producers behind
// ea_problem_set_{ref,now}_frame* (raw images -> edge points / DT image through the kernels of ea_preprocess.hip, in a
// workspace laid out by ea_frame_ws.h), their batched forms ea_batch_set_frames[_canny|_ros][_device] (N frame pairs, the
// frame a grid dimension of every launch) and the ROS chain's pyramid form ea_batch_set_frames_ros_pyramid (L levels from frames
// handed in once), ea_resize_half[_levels], the read-backs ea_problem_get_points / _get_dt, and the frame-to-frame
// tracker ea_tracker_* with its multi-stream form ea_tracker_batch_* (N streams through the batched producers, each frame
// processed once for both sides, one batch solve; with levels: coarse to fine).  Host code only: this file holds no kernel.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "../../include/ea_hip.h"
#include "ea_capi_internal.h"
#include "ea_frame_ws.h"
#include "ea_keyframe.h"
#include "ea_launch.h"
#include "ea_prior.h"
#include "ea_types.h"

using namespace ea;

// ---- the reference frame's edge points out of the frame producers' workspace (the producers themselves: further down) ----

// The edge points of a reference frame from the edge strength / edge map and the depth frame in the workspace, in two halves
// so that the tracker can put the first -- depth upload and per-block edge counts, both asynchronous on the null stream -- in
// front of the solve of the previous reference (which runs on the batch's own non-blocking stream and touches neither the
// workspace nor the depth) and the second -- count read-back, compaction -- behind it.  The full producers
// (ea_problem_set_ref_frame[_masked|_canny|_ros]) run the same two halves back to back (ref_points).
// What the first half left in flight on the null stream, and what the second needs to know
struct RefPointsJob {
  bool started = false;
  bool ros = false;                  // the ROS scatter: float depth in metres, every edge pixel a point
  int threshold = 0;                 // a pixel is an edge where its strength exceeds this
  const uint8_t *d_edges = nullptr;  // Laplacian strength or Canny edge map
  const void *d_depth = nullptr;     // uint16, float for the ROS scatter
  int *d_counts = nullptr, *d_total = nullptr;
};

// first half: per-block counts of the pixels of `edges` that become points, and their total.  The depth frame is in the
// workspace already (or on its way there on the null stream).
static int ref_points_count(ea_problem *p, const FrameWs &ws, const WsRegion<uint8_t> &edges, bool ros, int height, int width,
                            int threshold, RefPointsJob *job) {
  job->ros = ros;
  job->threshold = threshold;
  job->d_edges = edges.at(p->ws);
  job->d_depth = ws.depth.at(p->ws);
  job->d_counts = ws.counts.at(p->ws);
  job->d_total = job->d_counts + frame_ws_blocks(height, width);
  // (the ROS flavour keeps every edge pixel: no depth test)
  HIPCHK(launch_edge_count_scan(job->d_edges, ros ? nullptr : static_cast<const uint16_t *>(job->d_depth), height, width, threshold,
                                job->d_counts, job->d_total, nullptr));
  job->started = true;
  return EA_OK;
}

// a count the device has just produced (waits for the null stream)
static int read_count(const int *d_count, int *count) {
  HIPCHK(hipMemcpy(count, d_count, sizeof(int), hipMemcpyDeviceToHost));
  return EA_OK;
}

// The host bookkeeping of the producers, shared by the per-problem calls and ea_batch_set_frames.  Reference side: room for
// the frame's `total` points once the count is known (the problem is without points until ref_points_landed), then the
// point count and the depth weights' flags once scatter and weights have run.  Current side: the image alloc_dt made room
// for has been filled by launch_dt_store[_frames].
static int ref_points_room(ea_problem *p, int total) {
  p->version++;
  return reserve_points(p, total);
}
static void ref_points_landed(ea_problem *p, int total) {
  p->n = total;
  p->weighted = p->weights_from_depth = total > 0 && p->dw_power > 0;  // (reserve_points dropped the previous frame's)
}
static void dt_landed(ea_problem *p) {
  p->dt32_exact = p->d_dt32 != nullptr;  // the producers compute the distance transform in float32, as OpenCV does
  p->version++;
}

// second half: the points themselves, compacted in raster order and back-projected
static int ref_points_finish(ea_problem *p, const RefPointsJob &job, int height, int width, double z_scaling) {
  if (!job.started) return EA_ERR_STATE;
  int total = 0;
  int rc = read_count(job.d_total, &total);
  if (rc != EA_OK) return rc;
  rc = ref_points_room(p, total);
  if (rc != EA_OK) return rc;
  if (total > 0) {
    if (job.ros)
      HIPCHK(launch_edge_scatter_ros(p->dtype, job.d_edges, static_cast<const float *>(job.d_depth), height, width, job.d_counts,
                                     p->cam.fx, p->cam.fy, p->cam.cx, p->cam.cy, p->d_x, p->d_y, p->d_z, total, nullptr));
    else
      HIPCHK(launch_edge_scatter(p->dtype, job.d_edges, static_cast<const uint16_t *>(job.d_depth), height, width, job.threshold,
                                 job.d_counts, p->cam.fx, p->cam.fy, p->cam.cx, p->cam.cy, z_scaling, p->d_x, p->d_y, p->d_z, total,
                                 nullptr));
    // depth weighting (ea_problem_set_depth_weighting): the weights out of the z the scatter has just stored, behind it on
    // the same stream
    if (p->dw_power > 0)
      HIPCHK(launch_depth_weights(p->dtype, p->d_z, total, p->dw_z_ref, p->dw_power, weights_ptr(p), nullptr));
    HIPCHK(hipDeviceSynchronize());
  }
  ref_points_landed(p, total);
  return EA_OK;
}

// both halves: the tail of every full reference producer
static int ref_points(ea_problem *p, const FrameWs &ws, const WsRegion<uint8_t> &edges, bool ros, int height, int width,
                      int threshold, double z_scaling) {
  RefPointsJob job;
  const int rc = ref_points_count(p, ws, edges, ros, height, width, threshold, &job);
  return rc != EA_OK ? rc : ref_points_finish(p, job, height, width, z_scaling);
}

// The first half on what the last set_now_frame[_canny] call left in the workspace (kind 1: Laplacian strength in `lap`, 2:
// the edge map in `edges`): only the depth frame goes up.  EA_ERR_STATE when the workspace does not hold that frame.
static int ref_points_begin(ea_problem *p, int kind, const uint16_t *depth, int height, int width, int threshold, RefPointsJob *job) {
  job->started = false;
  if (p->ws_now_kind != kind || p->ws_now_h != height || p->ws_now_w != width) return EA_ERR_STATE;
  HIPCHK(hipSetDevice(p->device));
  const FrameWs ws = frame_ws(height, width);
  p->ws_now_kind = 0;
  HIPCHK(hipMemcpyAsync(ws.depth.at(p->ws), depth, (size_t)height * width * 2, hipMemcpyHostToDevice, nullptr));
  return ref_points_count(p, ws, kind == 1 ? ws.lap : ws.edges, false, height, width, threshold, job);
}

// Edge points of the frame the last set_now_frame[_canny] call processed, from what that call left in the workspace
// (Laplacian strength / Canny edge map): only the depth image goes up, no second upload or filtering of the colour
// frame.  Same thresholds, same compaction and back-projection as ea_problem_set_ref_frame[_canny] => the same points.
// Returns EA_ERR_STATE when the workspace does not hold that frame (the caller then takes the full path).
static int ref_points_from_last_now(ea_problem *p, int kind, const uint16_t *depth, int height, int width, double z_scaling,
                                    int threshold) {
  RefPointsJob job;
  int rc = ref_points_begin(p, kind, depth, height, width, threshold, &job);
  if (rc != EA_OK) return rc;
  return ref_points_finish(p, job, height, width, z_scaling);
}

// ---- frame-to-frame driver (the reference aligns one stored pair, src/ea.cpp:155-200) -------------
// Every pushed frame is aligned against the previous one: its DT image is produced, the previous frame's edge points
// are solved against it starting from the last relative pose (constant-velocity prior), then the new frame's edge
// points become the reference.  All of it stays on the device; one ea_problem is reused.
struct ea_tracker {
  ea_problem *p = nullptr;
  int flavour = 0;      // 0: get_aX / get_distance_transform, 1: Canny (get_aX_canny / get_distance_transform2)
  int frames = 0;
  double q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 0};
  // ea_tracker_set_covariance: the covariance of every aligned frame at the pose it returns
  bool cov_on = false, cov_valid = false;
  ea_covariance_options cov_opt{};
  ea_covariance cov_last{};
  // ea_tracker_set_motion_prior: NormalPriors centred on each solve's start pose, A = I / sigma (0 = that block off)
  double sigma_rot = 0.0, sigma_trans = 0.0;
  bool motion_set = false;  // the problem carries priors this tracker installed: `installed` (a caller's later prior differs)
  PriorDesc installed = {};
};

// The motion prior of the trackers (ea_tracker_set_motion_prior): NormalPriors centred on the constant-velocity prediction
// q, t the solve starts from, A = I / sigma (0 = that block off); they replace the caller's priors on the problem.
static int motion_prior_install(ea_problem *p, double sigma_rot, double sigma_trans, const double q[4], const double t[3]) {
  double Aq[16] = {0}, At[9] = {0};
  for (int i = 0; i < 4; ++i) Aq[5 * i] = sigma_rot > 0.0 ? 1.0 / sigma_rot : 0.0;
  for (int i = 0; i < 3; ++i) At[4 * i] = sigma_trans > 0.0 ? 1.0 / sigma_trans : 0.0;
  const int rc = ea_problem_set_normal_prior(p, 0, sigma_rot > 0.0 ? Aq : nullptr, 4, q);
  return rc != EA_OK ? rc : ea_problem_set_normal_prior(p, 1, sigma_trans > 0.0 ? At : nullptr, 3, t);
}
// off again: a block still holding the prior a tracker installed (`ins`) is cleared; one the caller has set since is kept
static void motion_prior_clear(ea_problem *p, const PriorDesc &ins) {
  const PriorDesc &cur = p->prior;
  if (cur.has_q && ins.has_q && std::memcmp(cur.Hq, ins.Hq, sizeof(cur.Hq)) == 0 && std::memcmp(cur.bq, ins.bq, sizeof(cur.bq)) == 0)
    (void)ea_problem_set_normal_prior(p, 0, nullptr, 0, nullptr);
  if (cur.has_t && ins.has_t && std::memcmp(cur.Ht, ins.Ht, sizeof(cur.Ht)) == 0 && std::memcmp(cur.bt, ins.bt, sizeof(cur.bt)) == 0)
    (void)ea_problem_set_normal_prior(p, 1, nullptr, 0, nullptr);
}
static bool sigmas_ok(double sigma_rot, double sigma_trans) {
  return sigma_rot >= 0.0 && sigma_rot <= DBL_MAX && sigma_trans >= 0.0 && sigma_trans <= DBL_MAX;
}

extern "C" int ea_tracker_create(ea_tracker **out, const ea_camera *cam, int dtype, int device, int flavour) {
  if (!out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (flavour != 0 && flavour != 1) return fail(EA_ERR_INVALID_ARG, "unknown pre-processing flavour");
  ea_tracker *tr = new (std::nothrow) ea_tracker;
  if (!tr) return fail(EA_ERR_ALLOC, "out of host memory");
  const int rc = ea_problem_create(&tr->p, cam, dtype, device);
  if (rc != EA_OK) { delete tr; return rc; }
  tr->flavour = flavour;
  *out = tr;
  return EA_OK;
}

extern "C" void ea_tracker_destroy(ea_tracker *tr) {
  if (!tr) return;
  ea_problem_destroy(tr->p);
  delete tr;
}

extern "C" ea_problem *ea_tracker_problem(ea_tracker *tr) { return tr ? tr->p : nullptr; }

// q_rel, t_rel: pose of the previous frame in the new frame's coordinates (b_T_a with a = previous, b = new); identity
// for the first frame.  aligned (nullable): 1 when a solve took place.  A failed solve keeps the prior for the next frame.
extern "C" int ea_tracker_push_frame(ea_tracker *tr, const uint8_t *bgr, const uint16_t *depth, int height, int width,
                                     double z_scaling, const ea_options *opt, double q_rel[4], double t_rel[3],
                                     ea_summary *summary, int *aligned) {
  if (!tr || !bgr || !depth || !q_rel || !t_rel) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  // every argument is checked before the tracker's problem is touched: a rejected call leaves the tracker as it was
  if (!(z_scaling > 0.0)) return fail(EA_ERR_INVALID_ARG, "z_scaling must be > 0");
  if (height < 1 || width < 1) return fail(EA_ERR_INVALID_ARG, "bad frame extent");
  int rc = EA_OK;
  if (aligned) *aligned = 0;
  if (summary) std::memset(summary, 0, sizeof(*summary));
  double q_new[4], t_new[3];
  std::memcpy(q_new, tr->q, sizeof(q_new));
  std::memcpy(t_new, tr->t, sizeof(t_new));
  RefPointsJob job;
  tr->cov_valid = false;
  if (tr->frames > 0 && ea_problem_num_points(tr->p) > 0) {
    rc = tr->flavour == 0 ? ea_problem_set_now_frame(tr->p, bgr, height, width, 35, 1, 1)
                          : ea_problem_set_now_frame_canny(tr->p, bgr, nullptr, height, width, 30, 90, 1, 0.0, 1.0);
    if (rc != EA_OK) return rc;
    // the new frame's depth goes up and its edge pixels are counted WHILE the previous reference is solved against the image
    // just produced (null stream beside the solve's non-blocking stream; neither touches what the other uses)
    (void)ref_points_begin(tr->p, tr->flavour == 0 ? 1 : 2, depth, height, width, tr->flavour == 0 ? 35 : 0, &job);
    double q[4], t[3];
    std::memcpy(q, tr->q, sizeof(q));
    std::memcpy(t, tr->t, sizeof(t));
    if (tr->sigma_rot > 0.0 || tr->sigma_trans > 0.0) {
      rc = motion_prior_install(tr->p, tr->sigma_rot, tr->sigma_trans, q, t);
      if (rc != EA_OK) {
        if (job.started) (void)hipDeviceSynchronize();
        return rc;
      }
      tr->motion_set = true;
      tr->installed = tr->p->prior;
    }
    ea_summary s;
    rc = ea_solve(tr->p, opt, q, t, &s);
    if (rc != EA_OK) {
      if (job.started) (void)hipDeviceSynchronize();  // (nothing of this frame may stay in flight behind a failed push)
      return rc;
    }
    if (s.termination != EA_FAILURE) {
      std::memcpy(q_new, q, sizeof(q));
      std::memcpy(t_new, t, sizeof(t));
    }
    if (tr->cov_on) {
      // The solve's points and DT image are still the problem's: ea_problem_covariance returns only once its results have
      // landed, i.e. once its evaluation on the batch's stream has read them, and ref_points_finish -- the only step that
      // overwrites the points -- is enqueued on the null stream after that.  ref_points_begin, already in flight on the null
      // stream, writes nothing but the workspace of the frame producers, which the evaluation does not read.
      std::memset(&tr->cov_last, 0, sizeof(tr->cov_last));
      if (s.termination != EA_FAILURE) {
        rc = ea_problem_covariance(tr->p, q, t, &tr->cov_opt, &tr->cov_last);
        if (rc != EA_OK) {
          if (job.started) (void)hipDeviceSynchronize();
          return rc;
        }
      } else {
        tr->cov_last.why = 4;  // no pose to take the covariance at
      }
      tr->cov_valid = true;
    }
    if (summary) *summary = s;
    if (aligned) *aligned = 1;
  }
  // the frame's edge strength / edge map is still in the workspace when it has just been the "now" frame
  rc = job.started ? ref_points_finish(tr->p, job, height, width, z_scaling)
                   : ref_points_from_last_now(tr->p, tr->flavour == 0 ? 1 : 2, depth, height, width, z_scaling, tr->flavour == 0 ? 35 : 0);
  if (rc == EA_ERR_STATE)
    rc = tr->flavour == 0 ? ea_problem_set_ref_frame(tr->p, bgr, depth, height, width, z_scaling, 35)
                          : ea_problem_set_ref_frame_canny(tr->p, bgr, depth, height, width, z_scaling, 30, 90);
  if (rc != EA_OK) {
    // the DT image is the new frame's but no reference came out of it: drop the stale reference so that the next push
    // starts a fresh chain instead of aligning frame k-1's points against frame k+2 from an advanced prior
    (void)reserve_points(tr->p, 0);
    tr->p->version++;
    tr->frames = 0;
    return rc;
  }
  // prior and frame count advance only with the new reference in place
  std::memcpy(tr->q, q_new, sizeof(q_new));
  std::memcpy(tr->t, t_new, sizeof(t_new));
  std::memcpy(q_rel, tr->q, sizeof(tr->q));
  std::memcpy(t_rel, tr->t, sizeof(tr->t));
  tr->frames += 1;
  return EA_OK;
}

extern "C" int ea_tracker_set_covariance(ea_tracker *tr, const ea_covariance_options *o) {
  if (!tr) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (o) {
    const int rc = check_cov_options(o);
    if (rc != EA_OK) return rc;
    tr->cov_opt = *o;
  }
  tr->cov_on = o != nullptr;
  tr->cov_valid = false;
  return EA_OK;
}

extern "C" int ea_tracker_set_motion_prior(ea_tracker *tr, double sigma_rot, double sigma_trans) {
  if (!tr) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!sigmas_ok(sigma_rot, sigma_trans)) return fail(EA_ERR_INVALID_ARG, "sigmas must be finite and >= 0");
  if (sigma_rot == 0.0 && sigma_trans == 0.0 && tr->motion_set) {
    motion_prior_clear(tr->p, tr->installed);
    tr->motion_set = false;
  }
  tr->sigma_rot = sigma_rot;
  tr->sigma_trans = sigma_trans;
  return EA_OK;
}

extern "C" int ea_tracker_last_covariance(ea_tracker *tr, ea_covariance *out) {
  if (!tr || !out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!tr->cov_on) return fail(EA_ERR_STATE, "covariance is off (ea_tracker_set_covariance)");
  if (!tr->cov_valid) return fail(EA_ERR_STATE, "the last push did not align a frame");
  *out = tr->cov_last;
  return EA_OK;
}

// ---- frame producers: raw images -> edge points / DT image, on the device -------

static int ensure_ws(ea_problem *p, size_t bytes) {
  p->ws_now_kind = 0;  // every producer starts by calling this: whatever the workspace held is about to be overwritten
  if (p->ws_bytes >= bytes) return EA_OK;
  if (p->ws) { cached_free(p->ws); p->ws = nullptr; p->ws_bytes = 0; }
  HIPCHK(cached_malloc(reinterpret_cast<void **>(&p->ws), bytes, p->device));
  p->ws_bytes = bytes;
  return EA_OK;
}

// What every producer starts with once its arguments are checked: the problem's device, a workspace large enough for a
// height x width frame laid out by name (ea_frame_ws.h), and the colour frame on its way into `bgr` (bgr == nullptr: the
// caller brings it there itself, stage_scaled)
static int frame_begin(ea_problem *p, const uint8_t *bgr, int height, int width, FrameWs *ws) {
  HIPCHK(hipSetDevice(p->device));
  *ws = frame_ws(height, width);
  const int rc = ensure_ws(p, ws->total);
  if (rc != EA_OK) return rc;
  if (bgr) HIPCHK(hipMemcpyAsync(ws->bgr.at(p->ws), bgr, (size_t)height * width * 3, hipMemcpyHostToDevice, nullptr));
  return EA_OK;
}

// a region of the workspace into a debug output of the caller's (nullable)
template <typename U>
static int read_region(ea_problem *p, const WsRegion<U> &r, size_t bytes, void *out) {
  if (out) HIPCHK(hipMemcpy(out, r.at(p->ws), bytes, hipMemcpyDeviceToHost));
  return EA_OK;
}

static int ref_frame_impl(ea_problem *p, const uint8_t *bgr, const uint8_t *mask, const uint16_t *depth, int height,
                          int width, double z_scaling, int threshold) {
  if (!p || !bgr || !depth) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (height < 3 || width < 3 || (int64_t)height * width > 0x3fffffff) return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  if (!(z_scaling > 0.0)) return fail(EA_ERR_INVALID_ARG, "z_scaling must be > 0");
  FrameWs ws;
  const int rc = frame_begin(p, bgr, height, width, &ws);
  if (rc != EA_OK) return rc;
  const size_t np = (size_t)height * width;
  HIPCHK(hipMemcpyAsync(ws.depth.at(p->ws), depth, np * 2, hipMemcpyHostToDevice, nullptr));
  HIPCHK(launch_edge_strength(ws.bgr.at(p->ws), height, width, ws.gray.at(p->ws), ws.lap.at(p->ws), nullptr));
  if (mask) {
    HIPCHK(hipMemcpyAsync(ws.keep.at(p->ws), mask, np, hipMemcpyHostToDevice, nullptr));
    HIPCHK(launch_gate_by_mask(ws.lap.at(p->ws), ws.keep.at(p->ws), height, width, nullptr));
  }
  return ref_points(p, ws, ws.lap, false, height, width, threshold, z_scaling);
}

extern "C" int ea_problem_set_ref_frame(ea_problem *p, const uint8_t *bgr, const uint16_t *depth, int height, int width,
                                        double z_scaling, int threshold) {
  return ref_frame_impl(p, bgr, nullptr, depth, height, width, z_scaling, threshold);
}

// get_aX_mask (ref: utils.cpp:283-369, call sites standalone_edge_align.cpp:1039, :1081): also requires mask > 0
extern "C" int ea_problem_set_ref_frame_masked(ea_problem *p, const uint8_t *bgr, const uint8_t *mask, const uint16_t *depth,
                                               int height, int width, double z_scaling, int threshold) {
  if (!mask) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  return ref_frame_impl(p, bgr, mask, depth, height, width, z_scaling, threshold);
}

// mask (0 = edge / DT source; the region `mask` or `inv`) -> chamfer DT in `dist` -> [normalise to [lo, hi]] -> the problem's
// padded DT image, and the plain float image in `plain`
static int dt_from_mask(ea_problem *p, const FrameWs &ws, const WsRegion<uint8_t> &mask, int height, int width, int normalize,
                        double lo, double hi, bool precise = false) {
  // the row pass stages one image row of column distances in LDS (4 bytes per pixel, 64 KB)
  if (width > 16384) return fail(EA_ERR_INVALID_ARG, "frames wider than 16384 pixels are not supported by the DT producers");
  int *d_dist = ws.dist.at(p->ws);  // doubles as the float32 distance when `precise`
  float *d_dist_f32 = precise ? ws.dist.at<float>(p->ws) : nullptr;
  unsigned int *d_minmax = ws.minmax.at(p->ws);
  HIPCHK(launch_chamfer(mask.at(p->ws), height, width, ws.G.at(p->ws), ws.scan.at(p->ws), d_dist, d_dist_f32, d_minmax, nullptr));
  {
    int rc = alloc_dt(p, width, height);
    if (rc != EA_OK) return rc;
  }
  HIPCHK(launch_dt_store(p->dtype, d_dist, d_dist_f32, height, width, d_minmax, normalize, lo, hi, p->d_dt, p->pitch,
                         ws.plain.at(p->ws), p->d_dt32, nullptr));
  HIPCHK(hipDeviceSynchronize());
  dt_landed(p);
  return EA_OK;
}

// `bgr` -> Laplacian strength in `lap` -> thresholded [median-filtered] `mask` -> dt_from_mask
static int run_dt(ea_problem *p, const FrameWs &ws, int height, int width, int threshold, int median, int normalize) {
  HIPCHK(launch_edge_strength(ws.bgr.at(p->ws), height, width, ws.gray.at(p->ws), ws.lap.at(p->ws), nullptr));
  HIPCHK(launch_threshold_median(ws.lap.at(p->ws), height, width, threshold, median, ws.mask.at(p->ws), nullptr));
  return dt_from_mask(p, ws, ws.mask, height, width, normalize, 0.0, 1.0);
}

// cv::Canny's integer thresholds (L1 magnitude): floor of the ordered pair.  NaN is refused; values beyond any magnitude an
// 8-bit image can produce (|dx| + |dy| <= 2040) are clamped before the conversion, which is undefined for them otherwise.
static int canny_thresholds(double t1, double t2, int *low, int *high) {
  if (t1 != t1 || t2 != t2) return fail(EA_ERR_INVALID_ARG, "Canny threshold is NaN");
  const double lo = std::min(t1, t2), hi = std::max(t1, t2);
  *low = (int)std::floor(std::min(std::max(lo, -1e9), 1e9));
  *high = (int)std::floor(std::min(std::max(hi, -1e9), 1e9));
  return EA_OK;
}

// blur 3x3 -> gray -> Canny(low, high) [-> AND (keep > 1), `masked`]: edge map in `edges`, its inverse in `inv`
static int run_canny(ea_problem *p, const FrameWs &ws, bool masked, int height, int width, int low, int high, int *rounds_out,
                     int l2_bgr = 0) {
  unsigned char *b = p->ws;
  HIPCHK(launch_canny(ws.bgr.at(b), height, width, low, high, l2_bgr, masked ? ws.keep.at(b) : nullptr, ws.gray.at(b), ws.mag.at(b),
                      ws.dir.at(b), ws.label.at(b), ws.edges.at(b), ws.inv.at(b), ws.changed.at(b), rounds_out, nullptr));
  return EA_OK;
}

static int check_frame_args(const ea_problem *p, const void *bgr, int height, int width) {
  if (!p || !bgr) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (height < 3 || width < 3 || height > 32768 || width > 32768 || (int64_t)height * width > 0x3fffffff)
    return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  return EA_OK;
}

// Canny flavour of the reference frame: get_aX_canny (ref: utils.cpp:371-462)
extern "C" int ea_problem_set_ref_frame_canny(ea_problem *p, const uint8_t *bgr, const uint16_t *depth, int height,
                                              int width, double z_scaling, double low_threshold, double high_threshold) {
  int rc = check_frame_args(p, bgr, height, width);
  if (rc != EA_OK) return rc;
  if (!depth) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!(z_scaling > 0.0) || !(z_scaling <= DBL_MAX)) return fail(EA_ERR_INVALID_ARG, "z_scaling must be > 0 and finite");
  int lo, hi;
  rc = canny_thresholds(low_threshold, high_threshold, &lo, &hi);
  if (rc != EA_OK) return rc;
  FrameWs ws;
  rc = frame_begin(p, bgr, height, width, &ws);
  if (rc != EA_OK) return rc;
  HIPCHK(hipMemcpyAsync(ws.depth.at(p->ws), depth, (size_t)height * width * 2, hipMemcpyHostToDevice, nullptr));
  rc = run_canny(p, ws, false, height, width, lo, hi, nullptr);
  if (rc != EA_OK) return rc;
  // ref: utils.cpp:441 -- all_grad(i) > 0 && Z > 0 on the 0/255 edge map
  return ref_points(p, ws, ws.edges, false, height, width, 0, z_scaling);
}

// Canny flavour of the current frame: get_distance_transform2 / _masked / _NoNormalize / _masked_NoNormalize
// (ref: utils.cpp:85-199).  mask (nullable): H x W bytes, edges survive where mask > 1.  normalize != 0: min-max to
// [norm_lo, norm_hi] ((0,1) at :103, (0,255) at :138).  The debug outputs may be NULL.
static int now_frame_canny(ea_problem *p, const uint8_t *bgr, const uint8_t *mask, int height, int width, double low_threshold,
                           double high_threshold, int normalize, double norm_lo, double norm_hi, uint8_t *edges_out,
                           int32_t *chamfer_fix_out, float *dt_out, int *rounds_out) {
  int rc = check_frame_args(p, bgr, height, width);
  if (rc != EA_OK) return rc;
  int lo, hi;
  rc = canny_thresholds(low_threshold, high_threshold, &lo, &hi);
  if (rc != EA_OK) return rc;
  if (normalize && (!(std::fabs(norm_lo) <= DBL_MAX) || !(std::fabs(norm_hi) <= DBL_MAX)))
    return fail(EA_ERR_INVALID_ARG, "normalisation range must be finite");
  FrameWs ws;
  rc = frame_begin(p, bgr, height, width, &ws);
  if (rc != EA_OK) return rc;
  const size_t np = (size_t)height * width;
  if (mask) HIPCHK(hipMemcpyAsync(ws.keep.at(p->ws), mask, np, hipMemcpyHostToDevice, nullptr));
  rc = run_canny(p, ws, mask != nullptr, height, width, lo, hi, rounds_out);
  if (rc == EA_OK) rc = dt_from_mask(p, ws, ws.inv, height, width, normalize, norm_lo, norm_hi);
  if (rc == EA_OK) rc = read_region(p, ws.edges, np, edges_out);
  if (rc == EA_OK) rc = read_region(p, ws.dist, np * 4, chamfer_fix_out);
  if (rc == EA_OK) rc = read_region(p, ws.plain, np * 4, dt_out);
  if (rc != EA_OK) return rc;
  // a masked edge map is not the one ea_problem_set_ref_frame_canny would produce from this frame: the tracker may not ride it
  if (!mask) { p->ws_now_kind = 2; p->ws_now_h = height; p->ws_now_w = width; }
  return EA_OK;
}

// ---- ROS flavour of the producers (ref: src/SolveEA.cpp:29-119): Canny(rgb, 150, 100, 3, true) on the 3-channel image
static int ros_thresholds(double t1, double t2, int *low, int *high) {
  // cv::Canny with L2gradient: min(t, 32767)^2, ordered
  if (t1 != t1 || t2 != t2) return fail(EA_ERR_INVALID_ARG, "Canny threshold is NaN");
  double lo = std::max(std::min(t1, t2), -1e4), hi = std::max(std::max(t1, t2), -1e4);
  lo = std::min(32767.0, lo); hi = std::min(32767.0, hi);
  if (lo > 0) lo *= lo;
  if (hi > 0) hi *= hi;
  *low = (int)std::floor(lo);
  *high = (int)std::floor(hi);
  return EA_OK;
}

namespace {
struct WsCarver {
  unsigned char *base;
  size_t off = 0;
  template <typename U> U *take(size_t n) {
    off = (off + 255) & ~(size_t)255;
    U *r = reinterpret_cast<U *>(base + off);
    off += n * sizeof(U);
    return r;
  }
};
}  // namespace

// Frames as the ROS callbacks receive them -> the resolution the node works at, on the device: `halvings` times
// (depth: NaN -> 0, then) cv::resize(..., 0.5, 0.5) (src/ea.cpp:38, :56-62).  bgr / depth: host, full_h x full_w; the
// results land in d_bgr / d_depth (device, full >> halvings).  halvings = 0: a plain upload.
static int stage_scaled(ea_problem *p, const uint8_t *bgr, const float *depth, int full_h, int full_w, int halvings,
                        uint8_t *d_bgr, float *d_depth) {
  const size_t np = (size_t)full_h * full_w;
  if (halvings == 0) {
    HIPCHK(hipMemcpyAsync(d_bgr, bgr, np * 3, hipMemcpyHostToDevice, nullptr));
    if (depth) HIPCHK(hipMemcpyAsync(d_depth, depth, np * 4, hipMemcpyHostToDevice, nullptr));
    return EA_OK;
  }
  // stage: [bgr full | depth full | bgr half | depth half] (the ping-pong partner of the full-size pair)
  const size_t need = np * 3 + np * 4 + np / 4 * 3 + np / 4 * 4 + 1024;
  if (p->stage_bytes < need) {
    if (p->stage) { cached_free(p->stage); p->stage = nullptr; p->stage_bytes = 0; }
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&p->stage), need, p->device));
    p->stage_bytes = need;
  }
  WsCarver st{p->stage};
  uint8_t *bgr_a = st.take<uint8_t>(np * 3), *bgr_b = nullptr;
  float *dep_a = st.take<float>(np), *dep_b = nullptr;
  bgr_b = st.take<uint8_t>(np / 4 * 3);
  dep_b = st.take<float>(np / 4);
  HIPCHK(hipMemcpyAsync(bgr_a, bgr, np * 3, hipMemcpyHostToDevice, nullptr));
  if (depth) HIPCHK(hipMemcpyAsync(dep_a, depth, np * 4, hipMemcpyHostToDevice, nullptr));
  int h = full_h, w = full_w;
  for (int k = 0; k < halvings; ++k) {
    const bool last = k == halvings - 1;
    uint8_t *bo = last ? d_bgr : bgr_b;
    float *dp = last ? d_depth : dep_b;
    HIPCHK(launch_resize_half_bgr8(bgr_a, h, w, bo, nullptr));
    if (depth) HIPCHK(launch_resize_half_f32(dep_a, h, w, dp, /*nan_to_zero=*/k == 0 ? 1 : 0, nullptr));
    std::swap(bgr_a, bgr_b); std::swap(dep_a, dep_b);
    h /= 2; w /= 2;
  }
  return EA_OK;
}

static int check_scaled_args(int height, int width, int halvings) {
  if (halvings < 0 || halvings > 8) return fail(EA_ERR_INVALID_ARG, "halvings out of range");
  if ((height % (1 << halvings)) != 0 || (width % (1 << halvings)) != 0)
    return fail(EA_ERR_INVALID_ARG, "frame extent must be divisible by 2^halvings");
  return EA_OK;
}

// SolveEA::setRefFrame (src/SolveEA.cpp:29-82): every edge pixel, depth CV_32F in metres, Z == 0 -> 1.0
extern "C" int ea_problem_set_ref_frame_ros_scaled(ea_problem *p, const uint8_t *bgr, const float *depth, int full_height,
                                                   int full_width, int halvings, double threshold1, double threshold2) {
  int rc = check_frame_args(p, bgr, full_height, full_width);
  if (rc != EA_OK) return rc;
  if (!depth) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  rc = check_scaled_args(full_height, full_width, halvings);
  if (rc != EA_OK) return rc;
  int lo, hi;
  rc = ros_thresholds(threshold1, threshold2, &lo, &hi);
  if (rc != EA_OK) return rc;
  const int height = full_height >> halvings, width = full_width >> halvings;
  if (height < 3 || width < 3) return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  FrameWs ws;
  rc = frame_begin(p, nullptr, height, width, &ws);
  if (rc == EA_OK) rc = stage_scaled(p, bgr, depth, full_height, full_width, halvings, ws.bgr.at(p->ws), ws.depth.at<float>(p->ws));
  if (rc == EA_OK) rc = run_canny(p, ws, false, height, width, lo, hi, nullptr, /*l2_bgr=*/1);
  if (rc != EA_OK) return rc;
  return ref_points(p, ws, ws.edges, /*ros=*/true, height, width, 0, /*z_scaling (metres already)=*/1.0);
}

extern "C" int ea_problem_set_ref_frame_ros(ea_problem *p, const uint8_t *bgr, const float *depth, int height, int width,
                                            double threshold1, double threshold2) {
  return ea_problem_set_ref_frame_ros_scaled(p, bgr, depth, height, width, 0, threshold1, threshold2);
}

// SolveEA::setNowFrame (src/SolveEA.cpp:86-119): Canny -> 255 - edges -> distanceTransform(L2, DIST_MASK_PRECISE) ->
// normalize to [0, 255].  An image without a single edge has no defined result upstream either: EA_ERR_STATE.
static int now_frame_ros_impl(ea_problem *p, const uint8_t *bgr, int full_height, int full_width, int halvings,
                              double threshold1, double threshold2, uint8_t *edges_out, float *dt_out) {
  int rc = check_frame_args(p, bgr, full_height, full_width);
  if (rc != EA_OK) return rc;
  rc = check_scaled_args(full_height, full_width, halvings);
  if (rc != EA_OK) return rc;
  int lo, hi;
  rc = ros_thresholds(threshold1, threshold2, &lo, &hi);
  if (rc != EA_OK) return rc;
  const int height = full_height >> halvings, width = full_width >> halvings;
  if (height < 3 || width < 3) return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  FrameWs ws;
  rc = frame_begin(p, nullptr, height, width, &ws);
  if (rc == EA_OK) rc = stage_scaled(p, bgr, nullptr, full_height, full_width, halvings, ws.bgr.at(p->ws), nullptr);
  if (rc == EA_OK) rc = run_canny(p, ws, false, height, width, lo, hi, nullptr, /*l2_bgr=*/1);
  if (rc != EA_OK) return rc;
  int *d_counts = ws.counts.at(p->ws), *d_total = d_counts + frame_ws_blocks(height, width), total = 0;
  HIPCHK(launch_edge_count_scan(ws.edges.at(p->ws), nullptr, height, width, 0, d_counts, d_total, nullptr));
  rc = read_count(d_total, &total);
  if (rc != EA_OK) return rc;
  if (total == 0) return fail(EA_ERR_STATE, "no edge in the frame: the exact distance transform is undefined");
  const size_t np = (size_t)height * width;
  rc = dt_from_mask(p, ws, ws.inv, height, width, 1, 0.0, 255.0, /*precise=*/true);
  if (rc == EA_OK) rc = read_region(p, ws.edges, np, edges_out);
  if (rc == EA_OK) rc = read_region(p, ws.plain, np * 4, dt_out);
  return rc;
}

extern "C" int ea_problem_debug_now_frame_ros(ea_problem *p, const uint8_t *bgr, int height, int width, double threshold1,
                                              double threshold2, uint8_t *edges_out, float *dt_out) {
  return now_frame_ros_impl(p, bgr, height, width, 0, threshold1, threshold2, edges_out, dt_out);
}

extern "C" int ea_problem_set_now_frame_ros(ea_problem *p, const uint8_t *bgr, int height, int width, double threshold1,
                                            double threshold2) {
  return now_frame_ros_impl(p, bgr, height, width, 0, threshold1, threshold2, nullptr, nullptr);
}

extern "C" int ea_problem_set_now_frame_ros_scaled(ea_problem *p, const uint8_t *bgr, int full_height, int full_width,
                                                   int halvings, double threshold1, double threshold2) {
  return now_frame_ros_impl(p, bgr, full_height, full_width, halvings, threshold1, threshold2, nullptr, nullptr);
}

// The half-resolution step by itself (host in, host out) for parity checks and for callers that build pyramid levels of
// their own: kind 0 = bgr8 (height x width x 3 bytes), 1 = float32 with NaN -> 0 first (the depth callback, src/ea.cpp:56-62),
// 2 = float32 as is.  dst: (height / 2) x (width / 2) of the same element type.
extern "C" int ea_resize_half(int device, int kind, const void *src, int height, int width, void *dst) {
  if (!src || !dst) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (kind < 0 || kind > 2) return fail(EA_ERR_INVALID_ARG, "kind must be 0 (bgr8), 1 (float32, NaN -> 0) or 2 (float32)");
  if (height < 2 || width < 2 || (height & 1) || (width & 1) || (int64_t)height * width > 0x3fffffff)
    return fail(EA_ERR_INVALID_ARG, "frame extent must be even and in range");
  int rc = check_device(device);
  if (rc != EA_OK) return rc;
  HIPCHK(hipSetDevice(device));
  const size_t np = (size_t)height * width, es = kind == 0 ? 3 : 4;
  DevBuf a, b;
  HIPCHK(cached_malloc(&a.p, np * es, device));
  HIPCHK(cached_malloc(&b.p, np / 4 * es, device));
  HIPCHK(hipMemcpy(a.p, src, np * es, hipMemcpyHostToDevice));
  if (kind == 0) HIPCHK(launch_resize_half_bgr8(a.as<uint8_t>(), height, width, b.as<uint8_t>(), nullptr));
  else HIPCHK(launch_resize_half_f32(a.as<float>(), height, width, b.as<float>(), kind == 1 ? 1 : 0, nullptr));
  HIPCHK(hipMemcpy(dst, b.p, np / 4 * es, hipMemcpyDeviceToHost));
  return EA_OK;
}

extern "C" int ea_problem_set_now_frame_canny(ea_problem *p, const uint8_t *bgr, const uint8_t *mask, int height, int width,
                                              double low_threshold, double high_threshold, int normalize, double norm_lo,
                                              double norm_hi) {
  return now_frame_canny(p, bgr, mask, height, width, low_threshold, high_threshold, normalize, norm_lo, norm_hi, nullptr,
                         nullptr, nullptr, nullptr);
}

extern "C" int ea_problem_debug_now_frame_canny(ea_problem *p, const uint8_t *bgr, const uint8_t *mask, int height,
                                                int width, double low_threshold, double high_threshold, int normalize,
                                                double norm_lo, double norm_hi, uint8_t *edges_out,
                                                int32_t *chamfer_fix_out, float *dt_out, int *hysteresis_launches) {
  return now_frame_canny(p, bgr, mask, height, width, low_threshold, high_threshold, normalize, norm_lo, norm_hi, edges_out,
                         chamfer_fix_out, dt_out, hysteresis_launches);
}

extern "C" int ea_problem_set_now_frame(ea_problem *p, const uint8_t *bgr, int height, int width, int threshold,
                                        int median, int normalize) {
  if (!p || !bgr) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (height < 3 || width < 3 || height > 32768 || width > 32768) return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  FrameWs ws;
  int rc = frame_begin(p, bgr, height, width, &ws);
  if (rc == EA_OK) rc = run_dt(p, ws, height, width, threshold, median, normalize);
  if (rc == EA_OK) { p->ws_now_kind = 1; p->ws_now_h = height; p->ws_now_w = width; }
  return rc;
}

// stages of the DT producer for parity checks: any output may be NULL
extern "C" int ea_problem_debug_now_frame(ea_problem *p, const uint8_t *bgr, int height, int width, int threshold,
                                          int median, int normalize, uint8_t *lap_out, uint8_t *mask_out,
                                          int32_t *chamfer_fix_out, float *dt_out) {
  if (!p || !bgr) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (height < 3 || width < 3 || height > 32768 || width > 32768) return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  FrameWs ws;
  int rc = frame_begin(p, bgr, height, width, &ws);
  if (rc == EA_OK) rc = run_dt(p, ws, height, width, threshold, median, normalize);
  const size_t np = (size_t)height * width;
  if (rc == EA_OK) rc = read_region(p, ws.lap, np, lap_out);
  if (rc == EA_OK) rc = read_region(p, ws.mask, np, mask_out);
  if (rc == EA_OK) rc = read_region(p, ws.dist, np * 4, chamfer_fix_out);
  if (rc == EA_OK) rc = read_region(p, ws.plain, np * 4, dt_out);
  return rc;
}

// ---- the batched producers: the Laplacian chain of ea_problem_set_ref_frame + ea_problem_set_now_frame for every problem of
// a batch, the frame a grid dimension of each step (ea_launch.h: FramesLaunch) ----------------------------------------------
//
// Memory, owned by the batch (batch_frames_reserve): a device block [count x frame_ws(H, W) | FrameSlot x count] -- 31.5
// bytes per pixel per frame; in the ROS call each frame's block is frame_stage(...), the workspace and the halving stage
// behind it, and the frame pointers of a device call follow the slots -- and a pinned block [table | table | int x count | int x 8 count]: two stagings of the table
// (FrameSlot x count, and behind them the ROS call's 3 x count frame pointers), because it goes up twice when reference frames
// are given (the point arrays exist only once the counts are back), the counts, and the hysteresis flags of the Canny and ROS
// flavours (further down).  Everything runs on the null stream, like the per-problem producers, with two waits: the counts,
// the end.

extern "C" void ea_default_frame_params(ea_frame_params *prm, int height, int width) {
  if (!prm) return;
  prm->height = height; prm->width = width;
  prm->z_scaling = 5000.0;
  prm->ref_threshold = 35;
  prm->now_threshold = 35; prm->now_median = 1; prm->now_normalize = 1;
}

// a frame the caller says is in device memory: of the batch's GPU, as far as the runtime can tell, and aligned for its elements
static int check_device_frame(const void *ptr, int device, size_t align, const char *what) {
  if (reinterpret_cast<uintptr_t>(ptr) % align != 0) return fail(EA_ERR_INVALID_ARG, std::string(what) + ": misaligned frame");
  hipPointerAttribute_t at;
  if (hipPointerGetAttributes(&at, ptr) != hipSuccess) {
    (void)hipGetLastError();
    return fail(EA_ERR_INVALID_ARG, std::string(what) + ": not memory of a HIP device known to this runtime");
  }
  if (at.type != hipMemoryTypeDevice) return fail(EA_ERR_INVALID_ARG, std::string(what) + ": device memory expected");
  if (at.device != device) return fail(EA_ERR_INVALID_ARG, std::string(what) + ": lives on another device than the batch");
  return EA_OK;
}

// What the two batched calls (ea_batch_set_frames, ea_batch_set_frames_canny) share: the argument checks, the batch's memory
// and the slot table, the reference side's counts and point arrays, the current side's images, and the tail.
struct BatchFrames {
  ea_problem *const *probs = nullptr;
  int count = 0, device = 0, H = 0, W = 0, dtype = 0;
  bool ref = false, now = false, on_device = false;
  // ea_batch_set_frames_ros: the frames as handed in are full_H x full_W and come down to H x W by `halvings` halving steps
  bool ros = false;
  int full_H = 0, full_W = 0, halvings = 0;
  FrameWs ws;
  FrameStage st;      // (ros) the halving stage behind each frame's workspace
  size_t stride = 0;  // from one frame's block to the next: ws.total, or st.total with a stage
  size_t n = 0, np = 0, table_bytes = 0;
  unsigned char *base = nullptr;  // frame 0's workspace; frame i's lies i * stride further on (frame(i))
  FrameSlot *h_slots[2] = {nullptr, nullptr};
  int *h_totals = nullptr, *h_flags = nullptr;
  FramesLaunch f;
  std::vector<FrameSlot> slots;
  // (ros, device frames, halvings > 0) the caller's full-size frames, which the first halving step reads in place: [ref_bgr x
  // n | ref_depth x n | now_bgr x n], travelling behind the slots in every upload of the table; d_ptrs: where they land
  std::vector<const void *> ptrs;
  const void *const *d_ptrs = nullptr;
  std::vector<unsigned char> no_image;  // (ros) current frames without any edge: no alloc_dt, no dt_landed
  int stage = 0;
  long long max_total = 0, max_weighted = 0;
  unsigned char *frame(size_t i) const { return base + i * stride; }
};

// every check that all three calls make, none of which touches a device or a problem.  now_mask: nullable (the Canny call's).
// ref_depth: uint16 or, for the ROS call, float frames -- depth_align is the element size a device frame must be aligned to.
// H, W: the extent the producers work at.
static int batch_frames_check(ea_batch *b, const uint8_t *const *ref_bgr, const void *const *ref_depth, size_t depth_align,
                              const uint8_t *const *now_bgr, const uint8_t *const *now_mask, int H, int W, double z_scaling,
                              bool on_device, BatchFrames *j) {
  const bool ref = ref_bgr || ref_depth, now = now_bgr != nullptr;
  if (ref && (!ref_bgr || !ref_depth)) return fail(EA_ERR_INVALID_ARG, "ref_bgr and ref_depth are given or NULL together");
  if (!ref && !now) return fail(EA_ERR_INVALID_ARG, "neither reference nor current frames given");
  if (H < 3 || W < 3 || H > 32768 || W > 32768 || (int64_t)H * W > 0x3fffffff)
    return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  if (now && W > 16384) return fail(EA_ERR_INVALID_ARG, "frames wider than 16384 pixels are not supported by the DT producers");
  if (!(z_scaling > 0.0)) return fail(EA_ERR_INVALID_ARG, "z_scaling must be > 0");
  const BatchView view = batch_view(b);
  ea_problem *const *probs = view.probs;
  const int count = view.count, device = view.device;
  if (count < 1 || count > 65535) return fail(EA_ERR_INVALID_ARG, "a batched producer call takes 1..65535 problems");
  for (int i = 0; i < count; ++i)
    if ((ref && (!ref_bgr[i] || !ref_depth[i])) || (now && !now_bgr[i]) || (now_mask && !now_mask[i]))
      return fail(EA_ERR_INVALID_ARG, "NULL frame in a given array");
  {
    std::vector<const ea_problem *> sorted(probs, probs + count);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
      return fail(EA_ERR_INVALID_ARG, "the same problem twice in the batch: each frame pair needs a problem of its own");
  }
  if (on_device)
    for (int i = 0; i < count; ++i) {
      int rc = EA_OK;
      if (ref) rc = check_device_frame(ref_bgr[i], device, 1, "ref_bgr");
      if (rc == EA_OK && ref) rc = check_device_frame(ref_depth[i], device, depth_align, "ref_depth");
      if (rc == EA_OK && now) rc = check_device_frame(now_bgr[i], device, 1, "now_bgr");
      if (rc == EA_OK && now_mask) rc = check_device_frame(now_mask[i], device, 1, "now_mask");
      if (rc != EA_OK) return rc;
    }
  j->probs = probs; j->count = count; j->device = device; j->H = H; j->W = W; j->dtype = probs[0]->dtype;
  j->ref = ref; j->now = now; j->on_device = on_device;
  return EA_OK;
}

// The batch's device block [count x frame_ws(H, W) | FrameSlot x count] and pinned block [FrameSlot x count | FrameSlot x
// count | int x count | int x count x kCannyFrameFlags] (two stagings of the table, the counts, the hysteresis flags of the
// Canny call), and the slots filled with what is known before the first launch: where each side's frames are read -- the
// workspace's copy of a host frame, the caller's device frame in place -- and the problem's camera and depth weighting.
// The ROS call (j->ros): each frame's block is its workspace and its halving stage (ea_frame_ws.h: frame_stage), the slots'
// colour and float depth pointers name the frame at the WORKING resolution -- the workspace's `bgr` / `depth`, or with
// halvings == 0 the caller's device frame in place -- and device frames to be halved travel as pointers behind the slots.
static void batch_frames_layout(BatchFrames *j);
static void batch_frames_place(BatchFrames *j, unsigned char *base, unsigned char *d_table, unsigned char *h_block,
                               const uint8_t *const *ref_bgr, const void *const *ref_depth, const uint8_t *const *now_bgr,
                               const uint8_t *const *now_mask);
static size_t batch_frames_pinned_bytes(const BatchFrames &j) {
  return (2 * j.table_bytes + j.n * (1 + kCannyFrameFlags) * sizeof(int) + 15) & ~(size_t)15;  // (several may lie in a row)
}
static int batch_frames_begin(ea_batch *b, const uint8_t *const *ref_bgr, const void *const *ref_depth,
                              const uint8_t *const *now_bgr, const uint8_t *const *now_mask, BatchFrames *j) {
  HIPCHK(hipSetDevice(j->device));
  batch_frames_layout(j);
  unsigned char *d_block = nullptr, *h_block = nullptr;
  const int rc = batch_frames_reserve(b, j->n * j->stride + j->table_bytes, batch_frames_pinned_bytes(*j), &d_block, &h_block);
  if (rc != EA_OK) return rc;
  batch_frames_set_without_edges(b, 0);
  batch_frames_place(j, d_block, d_block + j->n * j->stride, h_block, ref_bgr, ref_depth, now_bgr, now_mask);
  return EA_OK;
}

// the sizes: the frame's workspace, the stride between frames' blocks, the table (slots, and the frame pointers behind them)
static void batch_frames_layout(BatchFrames *j) {
  j->ws = frame_ws(j->H, j->W);
  const size_t n = j->n = (size_t)j->count;
  j->np = (size_t)j->H * j->W;
  j->stride = j->ws.total;
  if (j->ros) {
    j->st = frame_stage(j->full_H, j->full_W, j->halvings, !j->on_device);
    j->stride = j->st.total;
    if (j->on_device && j->halvings > 0) j->ptrs.assign(3 * n, nullptr);
  }
  j->table_bytes = n * sizeof(FrameSlot) + j->ptrs.size() * sizeof(void *);
  static_assert(sizeof(FrameSlot) % 8 == 0, "slots follow the 256-byte aligned workspaces, pointers follow the slots");
}

// base: frame 0's workspace (frame i's: j->stride bytes per frame further on); d_table: where the table lies on the device;
// h_block: batch_frames_pinned_bytes of pinned memory
static void batch_frames_place(BatchFrames *j, unsigned char *base, unsigned char *d_table, unsigned char *h_block,
                               const uint8_t *const *ref_bgr, const void *const *ref_depth, const uint8_t *const *now_bgr,
                               const uint8_t *const *now_mask) {
  const FrameWs &ws = j->ws;
  const size_t n = j->n, table_bytes = j->table_bytes;
  j->base = base;
  j->h_slots[0] = reinterpret_cast<FrameSlot *>(h_block);
  j->h_slots[1] = reinterpret_cast<FrameSlot *>(h_block + table_bytes);
  j->h_totals = reinterpret_cast<int *>(h_block + 2 * table_bytes);
  j->h_flags = j->h_totals + n;
  j->f.n = j->count; j->f.H = j->H; j->f.W = j->W; j->f.stride = j->stride;
  j->f.slots = reinterpret_cast<FrameSlot *>(d_table);
  j->d_ptrs = reinterpret_cast<const void *const *>(d_table + n * sizeof(FrameSlot));
  j->slots.resize(n);
  std::memset(j->slots.data(), 0, n * sizeof(FrameSlot));
  for (size_t i = 0; i < n; ++i) {
    ea_problem *p = j->probs[i];
    p->ws_now_kind = 0;  // (the problem's own workspace holds nothing of this frame pair)
    FrameSlot &sl = j->slots[i];
    unsigned char *wsi = j->frame(i);
    const bool in_place = j->on_device && j->halvings == 0;  // (halvings: 0 outside the ROS call)
    if (j->ref) sl.bgr[0] = in_place ? ref_bgr[i] : ws.bgr.at(wsi);
    if (j->ref && !j->ros) sl.depth = in_place ? static_cast<const uint16_t *>(ref_depth[i]) : ws.depth.at<uint16_t>(wsi);
    if (j->ref && j->ros) sl.depth_f32 = in_place ? static_cast<const float *>(ref_depth[i]) : ws.depth.at<float>(wsi);
    if (j->now) sl.bgr[1] = in_place ? now_bgr[i] : ws.bgr.at(wsi);
    if (!j->ptrs.empty()) {
      if (j->ref) { j->ptrs[i] = ref_bgr[i]; j->ptrs[n + i] = ref_depth[i]; }
      if (j->now) j->ptrs[2 * n + i] = now_bgr[i];
    }
    if (now_mask) sl.mask = j->on_device ? now_mask[i] : ws.keep.at(wsi);
    sl.fx = p->cam.fx; sl.fy = p->cam.fy; sl.cx = p->cam.cx; sl.cy = p->cam.cy;
    sl.z_ref = p->dw_z_ref; sl.power = p->dw_power;
  }
}

// The table on its way up: the slots and, behind them, the ROS call's frame pointers.  The rule: a staging block is not
// written again before a wait of the null stream has passed since it last went up.  The Laplacian and Canny calls upload at
// most twice, once from each staging.  The ROS call with both sides uploads three times -- before the reference side, with
// the point arrays, with the images -- and the third takes the first staging again: the counts of BOTH sides come back
// between the first and the third upload, each a blocking copy on the null stream, so the first upload has long landed.
static hipError_t upload_table(BatchFrames *j) {
  unsigned char *h = reinterpret_cast<unsigned char *>(j->h_slots[j->stage++ & 1]);
  const size_t slot_bytes = j->n * sizeof(FrameSlot);
  std::memcpy(h, j->slots.data(), slot_bytes);
  if (!j->ptrs.empty()) std::memcpy(h + slot_bytes, j->ptrs.data(), j->ptrs.size() * sizeof(void *));
  return hipMemcpyAsync(const_cast<FrameSlot *>(j->f.slots), h, j->table_bytes, hipMemcpyHostToDevice, nullptr);
}

// host frames into a region of every frame's workspace
template <typename U, typename V>
static int upload_frames(const BatchFrames &j, const WsRegion<U> &r, const V *const *frames, size_t bytes) {
  for (size_t i = 0; i < j.n; ++i) HIPCHK(hipMemcpyAsync(r.at(j.frame(i)), frames[i], bytes, hipMemcpyHostToDevice, nullptr));
  return EA_OK;
}

// count -> scan on every frame's `edges` region, the totals back into h_totals in one strided copy (a wait)
// (the two steps apart: the multi-stream tracker queues the first in front of its solve and fetches behind it)
static int batch_counts_queue(BatchFrames *j, const WsRegion<uint8_t> &edges, int threshold) {
  HIPCHK(launch_edge_count_scan_frames(j->f, edges.at(j->base), threshold, j->ws.counts.at(j->base), nullptr));
  return EA_OK;
}
static int batch_counts_fetch(BatchFrames *j) {
  HIPCHK(hipMemcpy2D(j->h_totals, sizeof(int), j->ws.counts.at(j->base) + frame_ws_blocks(j->H, j->W), j->stride, sizeof(int), j->n,
                     hipMemcpyDeviceToHost));
  return EA_OK;
}
static int batch_counts_back(BatchFrames *j, const WsRegion<uint8_t> &edges, int threshold) {
  const int rc = batch_counts_queue(j, edges, threshold);
  return rc != EA_OK ? rc : batch_counts_fetch(j);
}

// Reference side, first half: the counts, room for each problem's points and their arrays into its slot
static int batch_ref_room(BatchFrames *j, const unsigned char *take = nullptr);
static int batch_ref_counts(BatchFrames *j, const WsRegion<uint8_t> &edges, int threshold) {
  const int rc_counts = batch_counts_back(j, edges, threshold);
  return rc_counts != EA_OK ? rc_counts : batch_ref_room(j);
}
// (the counts are in h_totals; take: the multi-stream tracker's keyframe mode -- a problem with take[i] == 0 keeps the points
// it has: its slot stays at capacity 0 and nothing of it is touched)
static int batch_ref_room(BatchFrames *j, const unsigned char *take) {
  for (size_t i = 0; i < j->n; ++i) {
    if (take && !take[i]) continue;
    ea_problem *p = j->probs[i];
    const int total = j->h_totals[i];
    const int rc = ref_points_room(p, total);
    if (rc != EA_OK) return rc;  // (the problems so far are without points, as a failed per-problem call leaves one)
    FrameSlot &sl = j->slots[i];
    sl.capacity = total;
    if (total > 0) {
      sl.x = p->d_x; sl.y = p->d_y; sl.z = p->d_z; sl.w = weights_ptr(p);
      j->max_total = std::max<long long>(j->max_total, total);
      if (p->dw_power > 0) j->max_weighted = std::max<long long>(j->max_weighted, total);
    }
  }
  return EA_OK;
}

// Current side: every problem's image into its slot (a failure: the reference frames are put in place, no current frame is).
// A frame marked in no_image keeps the image it has: no alloc_dt, a slot without an image.
static int batch_alloc_dts(BatchFrames *j) {
  int rc_dt = EA_OK;
  for (size_t i = 0; i < j->n && rc_dt == EA_OK; ++i) {
    ea_problem *p = j->probs[i];
    if (!j->no_image.empty() && j->no_image[i]) continue;
    rc_dt = alloc_dt(p, j->W, j->H);
    j->slots[i].dt = p->d_dt; j->slots[i].dt32 = p->dtype == EA_F64 ? p->d_dt32 : nullptr; j->slots[i].pitch = p->pitch;
  }
  return rc_dt;
}

// Reference side, second half: the points and their depth weights.  A call whose frames have no point at all launches
// nothing that writes points; a frame without points among others has capacity 0 in its slot
static int batch_ref_scatter(const BatchFrames &j, const WsRegion<uint8_t> &edges, int threshold, double z_scaling) {
  if (j.max_total > 0)
    HIPCHK(launch_edge_scatter_frames(j.dtype, j.f, edges.at(j.base), threshold, j.ws.counts.at(j.base), z_scaling, nullptr));
  HIPCHK(launch_depth_weights_frames(j.dtype, j.f, j.max_weighted, nullptr));
  return EA_OK;
}

// The hysteresis pass of the Canny and ROS flavours on one side (0 reference, 1 current) of the job's frames: blur / gradient,
// non-maximum suppression, 8 hysteresis launches and one wait per look at the frames' flags, the finish -- into every frame's
// `edges` / `inv`.  *looks: the looks it took (0 when it failed); each caller posts its own batch_frames_set_rounds.
static int batch_canny(const BatchFrames &j, int side, bool masked, int lo, int hi, int l2_bgr, int *looks) {
  const FrameWs &ws = j.ws;
  unsigned char *base = j.base;
  int taken = 0;
  *looks = 0;
  HIPCHK(launch_canny_frames(j.f, side, masked, lo, hi, l2_bgr, ws.gray.at(base), ws.mag.at(base), ws.dir.at(base), ws.label.at(base),
                             ws.edges.at(base), ws.inv.at(base), ws.changed.at(base), j.h_flags, &taken, nullptr));
  *looks = taken;
  return EA_OK;
}

// The ROS chain's steps on one level's frames, behind the frames at the working resolution (batch_stage_ros,
// pyramid_stage_side): the two batched producers and the multi-stream tracker's push all run these.
// Current side: the hysteresis pass, count and scan on `edges` and the counts back (a wait) -- a frame without any edge has no
// exact distance transform and keeps the image it has (no_image), *bare counts them -- every other problem's image into its
// slot (*rc_dt: batch_alloc_dts's; a producer carries on to batch_frames_end with it, a push fails), and for the frames that
// have an edge the table up, the column passes and the exact row pass on `inv`, the store normalised to (0, 255).
static int batch_ros_now(BatchFrames *j, int lo, int hi, int *looks, int *bare, int *rc_dt) {
  const FrameWs &ws = j->ws;
  unsigned char *base = j->base;
  *bare = 0;
  *rc_dt = EA_OK;
  int rc = batch_canny(*j, 1, false, lo, hi, /*l2_bgr=*/1, looks);
  if (rc == EA_OK) rc = batch_counts_back(j, ws.edges, 0);
  if (rc != EA_OK) return rc;
  j->no_image.assign(j->n, 0);
  for (size_t i = 0; i < j->n; ++i)
    if (j->h_totals[i] == 0) { j->no_image[i] = 1; ++*bare; }
  *rc_dt = batch_alloc_dts(j);
  if (*rc_dt == EA_OK && (size_t)*bare < j->n) {
    HIPCHK(upload_table(j));  // the images
    HIPCHK(launch_chamfer_frames(j->f, ws.inv.at(base), ws.G.at(base), ws.scan.at(base), ws.dist.at(base), ws.dist.at<float>(base),
                                 ws.minmax.at(base), nullptr));
    HIPCHK(launch_dt_store_stack(j->dtype, j->f, ws.dist.at<float>(base), ws.minmax.at(base), 1, 0.0, 255.0, nullptr));
  }
  return EA_OK;
}
// Reference side, behind batch_ref_room: the table with the point arrays up, every edge pixel a point (no depth test,
// src/SolveEA.cpp:61-78) unless no frame has one, the depth weights.
static int batch_ros_scatter(BatchFrames *j) {
  HIPCHK(upload_table(j));
  if (j->max_total > 0) HIPCHK(launch_edge_scatter_ros_stack(j->dtype, j->f, j->ws.edges.at(j->base), j->ws.counts.at(j->base), nullptr));
  HIPCHK(launch_depth_weights_frames(j->dtype, j->f, j->max_weighted, nullptr));
  return EA_OK;
}

// the last wait, and the problems' bookkeeping
static int batch_frames_end(const BatchFrames &j, int rc_dt) {
  HIPCHK(hipDeviceSynchronize());
  for (size_t i = 0; i < j.n; ++i) {
    if (j.ref) ref_points_landed(j.probs[i], j.slots[i].capacity);
    if (j.now && rc_dt == EA_OK && (j.no_image.empty() || !j.no_image[i])) dt_landed(j.probs[i]);
  }
  return rc_dt;  // (a failed alloc_dt: the reference frames are in place, no current frame is)
}

static int batch_set_frames(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth,
                            const uint8_t *const *now_bgr, const ea_frame_params *prm, bool on_device) {
  // every check comes before a device or a problem is touched
  if (!b || !prm) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  BatchFrames j;
  const void *const *ref_depth_v = reinterpret_cast<const void *const *>(ref_depth);
  int rc = batch_frames_check(b, ref_bgr, ref_depth_v, 2, now_bgr, nullptr, prm->height, prm->width, prm->z_scaling, on_device, &j);
  if (rc == EA_OK) rc = batch_frames_begin(b, ref_bgr, ref_depth_v, now_bgr, nullptr, &j);
  if (rc != EA_OK) return rc;
  batch_frames_set_rounds(b, 0);  // (no hysteresis in this chain)
  const FrameWs &ws = j.ws;
  unsigned char *base = j.base;
  if (j.ref) {
    // strength -> count -> scan for every frame, the counts back in one strided copy: the first wait
    HIPCHK(upload_table(&j));
    if (!on_device) {
      rc = upload_frames(j, ws.bgr, ref_bgr, j.np * 3);
      if (rc == EA_OK) rc = upload_frames(j, ws.depth, ref_depth, j.np * 2);
      if (rc != EA_OK) return rc;
    }
    HIPCHK(launch_edge_strength_frames(j.f, 0, ws.gray.at(base), ws.lap.at(base), nullptr));
    rc = batch_ref_counts(&j, ws.lap, prm->ref_threshold);
    if (rc != EA_OK) return rc;
  }
  const int rc_dt = j.now ? batch_alloc_dts(&j) : EA_OK;
  HIPCHK(upload_table(&j));
  if (j.ref) {
    rc = batch_ref_scatter(j, ws.lap, prm->ref_threshold, prm->z_scaling);
    if (rc != EA_OK) return rc;
  }
  if (j.now && rc_dt == EA_OK) {
    if (!on_device) {
      rc = upload_frames(j, ws.bgr, now_bgr, j.np * 3);
      if (rc != EA_OK) return rc;
    }
    HIPCHK(launch_edge_strength_frames(j.f, 1, ws.gray.at(base), ws.lap.at(base), nullptr));
    HIPCHK(launch_threshold_median_frames(j.f, ws.lap.at(base), prm->now_threshold, prm->now_median, ws.mask.at(base), nullptr));
    HIPCHK(launch_chamfer_frames(j.f, ws.mask.at(base), ws.G.at(base), ws.scan.at(base), ws.dist.at(base), nullptr, ws.minmax.at(base), nullptr));
    HIPCHK(launch_dt_store_frames(j.dtype, j.f, ws.dist.at(base), ws.minmax.at(base), prm->now_normalize, 0.0, 1.0, nullptr));
  }
  return batch_frames_end(j, rc_dt);
}

extern "C" int ea_batch_set_frames(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth,
                                   const uint8_t *const *now_bgr, const ea_frame_params *prm) {
  return batch_set_frames(b, ref_bgr, ref_depth, now_bgr, prm, false);
}

extern "C" int ea_batch_set_frames_device(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth,
                                          const uint8_t *const *now_bgr, const ea_frame_params *prm) {
  return batch_set_frames(b, ref_bgr, ref_depth, now_bgr, prm, true);
}

// ---- the Canny flavour of the batched producers: ea_problem_set_ref_frame_canny + ea_problem_set_now_frame_canny for every
// problem of a batch.  Either side runs launch_canny_frames -- 3 launches, then 8 hysteresis launches and one wait per look at
// the frames' flags, then the finish -- into the frames' `edges` / `inv`; from there on the steps are the Laplacian call's,
// on other regions: count / scan / scatter on `edges` with threshold 0, chamfer on `inv`.  Waits: one per look, the counts,
// the end.

extern "C" void ea_default_canny_frame_params(ea_canny_frame_params *prm, int height, int width) {
  if (!prm) return;
  prm->height = height; prm->width = width;
  prm->z_scaling = 5000.0;
  prm->low_threshold = 30.0; prm->high_threshold = 90.0;
  prm->now_normalize = 1;
  prm->norm_lo = 0.0; prm->norm_hi = 1.0;
}

static int batch_set_frames_canny(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth,
                                  const uint8_t *const *now_bgr, const uint8_t *const *now_mask, const ea_canny_frame_params *prm,
                                  bool on_device) {
  // every check comes before a device or a problem is touched
  if (!b || !prm) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (now_mask && !now_bgr) return fail(EA_ERR_INVALID_ARG, "now_mask without now_bgr");
  int lo, hi;
  int rc = canny_thresholds(prm->low_threshold, prm->high_threshold, &lo, &hi);
  if (rc != EA_OK) return rc;
  if (prm->now_normalize && (!(std::fabs(prm->norm_lo) <= DBL_MAX) || !(std::fabs(prm->norm_hi) <= DBL_MAX)))
    return fail(EA_ERR_INVALID_ARG, "normalisation range must be finite");
  if (!(prm->z_scaling > 0.0) || !(prm->z_scaling <= DBL_MAX)) return fail(EA_ERR_INVALID_ARG, "z_scaling must be > 0 and finite");
  BatchFrames j;
  const void *const *ref_depth_v = reinterpret_cast<const void *const *>(ref_depth);
  rc = batch_frames_check(b, ref_bgr, ref_depth_v, 2, now_bgr, now_mask, prm->height, prm->width, prm->z_scaling, on_device, &j);
  if (rc == EA_OK) rc = batch_frames_begin(b, ref_bgr, ref_depth_v, now_bgr, now_mask, &j);
  if (rc != EA_OK) return rc;
  const FrameWs &ws = j.ws;
  unsigned char *base = j.base;
  int looks = 0, total_looks = 0;
  batch_frames_set_rounds(b, 0);
  if (j.ref) {
    HIPCHK(upload_table(&j));
    if (!on_device) {
      rc = upload_frames(j, ws.bgr, ref_bgr, j.np * 3);
      if (rc == EA_OK) rc = upload_frames(j, ws.depth, ref_depth, j.np * 2);
      if (rc != EA_OK) return rc;
    }
    rc = batch_canny(j, 0, false, lo, hi, /*l2_bgr=*/0, &looks);
    batch_frames_set_rounds(b, total_looks += looks);
    if (rc != EA_OK) return rc;
    // ref: utils.cpp:441 -- all_grad(i) > 0 && Z > 0 on the 0/255 edge map
    rc = batch_ref_counts(&j, ws.edges, 0);
    if (rc != EA_OK) return rc;
  }
  const int rc_dt = j.now ? batch_alloc_dts(&j) : EA_OK;
  HIPCHK(upload_table(&j));
  if (j.ref) {
    rc = batch_ref_scatter(j, ws.edges, 0, prm->z_scaling);
    if (rc != EA_OK) return rc;
  }
  if (j.now && rc_dt == EA_OK) {
    if (!on_device) {
      rc = upload_frames(j, ws.bgr, now_bgr, j.np * 3);
      if (rc == EA_OK && now_mask) rc = upload_frames(j, ws.keep, now_mask, j.np);
      if (rc != EA_OK) return rc;
    }
    // (the scatter above reads the reference side's `edges` and is in front of this on the same stream)
    rc = batch_canny(j, 1, now_mask != nullptr, lo, hi, /*l2_bgr=*/0, &looks);
    batch_frames_set_rounds(b, total_looks += looks);
    if (rc != EA_OK) return rc;
    HIPCHK(launch_chamfer_frames(j.f, ws.inv.at(base), ws.G.at(base), ws.scan.at(base), ws.dist.at(base), nullptr, ws.minmax.at(base), nullptr));
    HIPCHK(launch_dt_store_frames(j.dtype, j.f, ws.dist.at(base), ws.minmax.at(base), prm->now_normalize, prm->norm_lo, prm->norm_hi,
                                  nullptr));
  }
  return batch_frames_end(j, rc_dt);
}

extern "C" int ea_batch_set_frames_canny(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth,
                                         const uint8_t *const *now_bgr, const uint8_t *const *now_mask,
                                         const ea_canny_frame_params *prm) {
  return batch_set_frames_canny(b, ref_bgr, ref_depth, now_bgr, now_mask, prm, false);
}

extern "C" int ea_batch_set_frames_canny_device(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth,
                                                const uint8_t *const *now_bgr, const uint8_t *const *now_mask,
                                                const ea_canny_frame_params *prm) {
  return batch_set_frames_canny(b, ref_bgr, ref_depth, now_bgr, now_mask, prm, true);
}

// ---- the ROS flavour of the batched producers: ea_problem_set_ref_frame_ros_scaled + ea_problem_set_now_frame_ros_scaled for
// every problem of a batch.  Either side: the frames come down to the working resolution (batch_stage_ros: 2 launches per
// halving for the reference side, 1 for the current side), then launch_canny_frames in its l2_bgr form -- 2 launches, 8
// hysteresis launches and one wait per look, the finish -- then count and scan on `edges` without a depth test and the counts
// back (a wait).  Reference side: the ROS scatter and the depth weights.  Current side: the column passes and the exact row
// pass on `inv`, the store normalised to (0, 255), for the frames that have an edge.  Waits: one per look, the counts of each
// side, the end -- five for a call with both sides and one look each, where the per-problem calls wait six times per PAIR.

extern "C" void ea_default_ros_frame_params(ea_ros_frame_params *prm, int full_height, int full_width) {
  if (!prm) return;
  prm->full_height = full_height; prm->full_width = full_width;
  prm->halvings = 0;
  prm->threshold1 = 150.0; prm->threshold2 = 100.0;
}

// One side's frames at the working resolution: in every frame's `bgr` (and float `depth`: the reference side, depth given)
// -- or, for device frames without halvings, nowhere: the slots name the caller's frames.  Host frames go up into the
// workspace (halvings == 0: as they are, no NaN -> 0, like stage_scaled) or into the stage's full-size regions; the halving
// steps then walk full -> a -> b -> a ... with the last one landing in the workspace (ea_frame_ws.h: frame_stage), the
// first reading device frames in place through the pointer table behind the slots, NaN -> 0 on the first step only.
static int batch_stage_ros(const BatchFrames &j, int side, const uint8_t *const *bgr, const float *const *depth) {
  const FrameWs &ws = j.ws;
  const FrameStage &st = j.st;
  unsigned char *base = j.base;
  const size_t npf = (size_t)j.full_H * j.full_W;
  const bool has_depth = side == 0;
  if (j.halvings == 0) {
    if (j.on_device) return EA_OK;
    int rc = upload_frames(j, ws.bgr, bgr, npf * 3);
    if (rc == EA_OK && has_depth) rc = upload_frames(j, ws.depth, depth, npf * 4);
    return rc;
  }
  const uint8_t *const *bgr_table = nullptr;
  const float *const *depth_table = nullptr;
  const uint8_t *bsrc = nullptr;
  const float *dsrc = nullptr;
  if (j.on_device) {
    bgr_table = reinterpret_cast<const uint8_t *const *>(j.d_ptrs + (side == 0 ? 0 : 2 * j.n));
    depth_table = reinterpret_cast<const float *const *>(j.d_ptrs + j.n);
  } else {
    int rc = upload_frames(j, st.bgr_full, bgr, npf * 3);
    if (rc == EA_OK && has_depth) rc = upload_frames(j, st.depth_full, depth, npf * 4);
    if (rc != EA_OK) return rc;
    bsrc = st.bgr_full.at(base);
    dsrc = st.depth_full.at(base);
  }
  int h = j.full_H, w = j.full_W;
  for (int k = 0; k < j.halvings; ++k) {
    const bool last = k == j.halvings - 1;
    uint8_t *bdst = last ? ws.bgr.at(base) : (k & 1) ? st.bgr_b.at(base) : st.bgr_a.at(base);
    float *ddst = last ? ws.depth.at<float>(base) : (k & 1) ? st.depth_b.at(base) : st.depth_a.at(base);
    HIPCHK(launch_resize_half_bgr8_stack(j.f, k == 0 ? bgr_table : nullptr, bsrc, h, w, bdst, nullptr));
    if (has_depth)
      HIPCHK(launch_resize_half_f32_stack(j.f, k == 0 ? depth_table : nullptr, dsrc, h, w, ddst, /*nan_to_zero=*/k == 0 ? 1 : 0, nullptr));
    bsrc = bdst; dsrc = ddst;
    h /= 2; w /= 2;
  }
  return EA_OK;
}

static int batch_set_frames_ros(ea_batch *b, const uint8_t *const *ref_bgr, const float *const *ref_depth,
                                const uint8_t *const *now_bgr, const ea_ros_frame_params *prm, bool on_device) {
  // every check comes before a device or a problem is touched; the extents are checked as the per-problem _scaled calls do
  if (!b || !prm) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  const int full_h = prm->full_height, full_w = prm->full_width;
  if (full_h < 3 || full_w < 3 || full_h > 32768 || full_w > 32768 || (int64_t)full_h * full_w > 0x3fffffff)
    return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  int rc = check_scaled_args(full_h, full_w, prm->halvings);
  if (rc != EA_OK) return rc;
  int lo, hi;
  rc = ros_thresholds(prm->threshold1, prm->threshold2, &lo, &hi);
  if (rc != EA_OK) return rc;
  const int H = full_h >> prm->halvings, W = full_w >> prm->halvings;
  if (H < 3 || W < 3) return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  BatchFrames j;
  j.ros = true; j.full_H = full_h; j.full_W = full_w; j.halvings = prm->halvings;
  const void *const *ref_depth_v = reinterpret_cast<const void *const *>(ref_depth);
  rc = batch_frames_check(b, ref_bgr, ref_depth_v, sizeof(float), now_bgr, nullptr, H, W, /*z_scaling (metres already)=*/1.0, on_device, &j);
  if (rc == EA_OK) rc = batch_frames_begin(b, ref_bgr, ref_depth_v, now_bgr, nullptr, &j);
  if (rc != EA_OK) return rc;
  int looks = 0, total_looks = 0;
  batch_frames_set_rounds(b, 0);
  HIPCHK(upload_table(&j));  // where the frames are read, the cameras, the depth weighting
  if (j.ref) {
    rc = batch_stage_ros(j, 0, ref_bgr, ref_depth);
    if (rc != EA_OK) return rc;
    rc = batch_canny(j, 0, false, lo, hi, /*l2_bgr=*/1, &looks);
    batch_frames_set_rounds(b, total_looks += looks);
    if (rc == EA_OK) rc = batch_ref_counts(&j, j.ws.edges, 0);
    if (rc == EA_OK) rc = batch_ros_scatter(&j);
    if (rc != EA_OK) return rc;
  }
  int rc_dt = EA_OK, bare = 0;
  if (j.now) {
    // (the scatter above reads the reference side's `edges` and `depth` and is in front of this on the same stream; the
    // current side writes no depth; its third upload of the table takes the first staging again, two waits after it last went up)
    rc = batch_stage_ros(j, 1, now_bgr, nullptr);
    if (rc != EA_OK) return rc;
    rc = batch_ros_now(&j, lo, hi, &looks, &bare, &rc_dt);
    batch_frames_set_rounds(b, total_looks += looks);
    if (rc != EA_OK) return rc;
  }
  batch_frames_set_without_edges(b, bare);
  rc = batch_frames_end(j, rc_dt);
  if (rc == EA_OK && bare > 0)
    return fail(EA_ERR_STATE, "no edge in " + std::to_string(bare) + " of the current frames, the first at index " +
                                  std::to_string(std::find(j.no_image.begin(), j.no_image.end(), 1) - j.no_image.begin()) +
                                  ": the exact distance transform is undefined");
  return rc;
}

extern "C" int ea_batch_set_frames_ros(ea_batch *b, const uint8_t *const *ref_bgr, const float *const *ref_depth,
                                       const uint8_t *const *now_bgr, const ea_ros_frame_params *prm) {
  return batch_set_frames_ros(b, ref_bgr, ref_depth, now_bgr, prm, false);
}

extern "C" int ea_batch_set_frames_ros_device(ea_batch *b, const uint8_t *const *ref_bgr, const float *const *ref_depth,
                                              const uint8_t *const *now_bgr, const ea_ros_frame_params *prm) {
  return batch_set_frames_ros(b, ref_bgr, ref_depth, now_bgr, prm, true);
}

// ---- the pyramid form of the ROS producers: ea_batch_set_frames_ros with halvings, halvings + 1, ... on the batches of the
// levels, from frames handed in ONCE.  The frames' blocks are laid out by frame_pyramid (ea_frame_ws.h) in the block of
// levels[0]: every level's workspace, then the stage; each level has a BatchFrames of its own whose base is its workspace in
// frame 0's block and whose stride is the pyramid's, a slot table of its own behind the frames, and its part of the pinned
// block -- so every step behind the halvings is the single-level call's, launched per level.  Per side: the frames go up (host
// frames: once, into the stage's full-size regions, or without halvings into level 0's own `bgr` / `depth` as they are), ONE
// halving chain per kind (launch_halving_chain_*: three steps per launch) leaves every level's frame in that level's `bgr` /
// `depth`, then per level the sequence of batch_set_frames_ros.  The reference side of all levels is queued before the
// current side overwrites the stage and the levels' `bgr`; everything is on the null stream.

// `T` halving steps of every frame from one read per launch.  dst_of(k), k = 1..T: where the frames after k steps go (frame
// 0's pointer), NULL = nowhere; the frames after 3 and 6 steps (where a launch ends) and after T must go somewhere.
template <typename E, typename DstOf>
static int halving_chain(const FramesLaunch &f, const E *const *table, const E *src, int H, int W, int T, DstOf dst_of, int nan_to_zero) {
  for (int k0 = 0; k0 < T; k0 += kChainSteps) {
    const int steps = std::min(kChainSteps, T - k0);
    ChainLevels lv;
    for (int s = 0; s < steps; ++s) lv.dst[s] = dst_of(k0 + s + 1);
    if constexpr (sizeof(E) == 1)
      HIPCHK(launch_halving_chain_bgr8(f, k0 == 0 ? table : nullptr, src, H >> k0, W >> k0, steps, lv, nullptr));
    else
      HIPCHK(launch_halving_chain_f32(f, k0 == 0 ? table : nullptr, src, H >> k0, W >> k0, steps, lv, k0 == 0 ? nan_to_zero : 0, nullptr));
    src = static_cast<const E *>(lv.dst[steps - 1]);
  }
  return EA_OK;
}

// One side's frames on every level.  J: the levels' jobs (J[0].base is frame 0's block); *uploads counts the frame copies.
static int pyramid_stage_side(const std::vector<BatchFrames> &J, const FramePyramid &py, int halvings, int side,
                              const uint8_t *const *bgr, const float *const *depth, int64_t *uploads) {
  const BatchFrames &j0 = J[0];
  const int T = halvings + (int)J.size() - 1;
  const size_t npf = (size_t)j0.full_H * j0.full_W;
  const bool has_depth = side == 0;
  unsigned char *block = j0.base;
  const uint8_t *bsrc = nullptr;
  const float *dsrc = nullptr;
  if (!j0.on_device) {
    const WsRegion<uint8_t> &rb = halvings > 0 ? py.bgr_full : j0.ws.bgr;
    int rc = upload_frames(j0, rb, bgr, npf * 3);
    *uploads += (int64_t)j0.n;
    bsrc = rb.at(block);
    if (rc == EA_OK && has_depth) {
      if (halvings > 0) { rc = upload_frames(j0, py.depth_full, depth, npf * 4); dsrc = py.depth_full.at(block); }
      else { rc = upload_frames(j0, j0.ws.depth, depth, npf * 4); dsrc = j0.ws.depth.at<float>(block); }
      *uploads += (int64_t)j0.n;
    }
    if (rc != EA_OK) return rc;
  }
  if (T == 0) return EA_OK;
  const uint8_t *const *bgr_table = nullptr;
  const float *const *depth_table = nullptr;
  if (j0.on_device) {
    bgr_table = reinterpret_cast<const uint8_t *const *>(j0.d_ptrs + (side == 0 ? 0 : 2 * j0.n));
    depth_table = reinterpret_cast<const float *const *>(j0.d_ptrs + j0.n);
  }
  FramesLaunch f;
  f.n = j0.count; f.stride = j0.stride;
  int rc = halving_chain<uint8_t>(f, bgr_table, bsrc, j0.full_H, j0.full_W, T, [&](int k) -> void * {
    if (k >= halvings) return J[(size_t)(k - halvings)].ws.bgr.at(J[(size_t)(k - halvings)].base);
    return k == 3 ? py.bgr_a.at(block) : k == 6 ? py.bgr_b.at(block) : nullptr;
  }, 0);
  if (rc == EA_OK && has_depth)
    rc = halving_chain<float>(f, depth_table, dsrc, j0.full_H, j0.full_W, T, [&](int k) -> void * {
      if (k >= halvings) return J[(size_t)(k - halvings)].ws.depth.at<float>(J[(size_t)(k - halvings)].base);
      return k == 3 ? py.depth_a.at(block) : k == 6 ? py.depth_b.at(block) : nullptr;
    }, /*nan_to_zero=*/1);
  return rc;
}

// The memory of a pyramid call, after its checks: the frames' blocks (frame_pyramid) and every level's slot table in the
// device block of levels[0], every level's staging in its pinned block, and each level's job placed on its part.
static int pyramid_frames_begin(ea_batch *const *levels, std::vector<BatchFrames> *jobs, int halvings, const uint8_t *const *ref_bgr,
                                const void *const *ref_depth, const uint8_t *const *now_bgr, FramePyramid *py_out) {
  std::vector<BatchFrames> &J = *jobs;
  const int nlevels = (int)J.size(), T = halvings + nlevels - 1;
  const bool on_device = J[0].on_device;
  HIPCHK(hipSetDevice(J[0].device));
  const FramePyramid py = *py_out = frame_pyramid(J[0].full_H, J[0].full_W, halvings, nlevels, !on_device);
  const size_t n = (size_t)J[0].count;
  size_t table_total = 0, pinned_total = 0;
  for (int l = 0; l < nlevels; ++l) {
    BatchFrames &j = J[(size_t)l];
    batch_frames_layout(&j);
    j.stride = py.total;
    // the caller's device frames travel once, behind level 0's slots, for the chain's first launch
    j.ptrs.clear();
    if (l == 0 && on_device && T > 0) j.ptrs.assign(3 * n, nullptr);
    j.table_bytes = n * sizeof(FrameSlot) + j.ptrs.size() * sizeof(void *);
    table_total += j.table_bytes;
    pinned_total += batch_frames_pinned_bytes(j);
  }
  unsigned char *d_block = nullptr, *h_block = nullptr;
  const int rc = batch_frames_reserve(levels[0], n * py.total + table_total, pinned_total, &d_block, &h_block);
  if (rc != EA_OK) return rc;
  unsigned char *d_table = d_block + n * py.total, *h = h_block;
  for (int l = 0; l < nlevels; ++l) {
    BatchFrames &j = J[(size_t)l];
    batch_frames_set_without_edges(levels[l], 0);
    batch_frames_set_rounds(levels[l], 0);
    batch_frames_place(&j, d_block + py.level_off[l], d_table, h, ref_bgr, ref_depth, now_bgr, nullptr);
    d_table += j.table_bytes;
    h += batch_frames_pinned_bytes(j);
  }
  return EA_OK;
}

static int batch_set_frames_ros_pyramid(ea_batch *const *levels, int nlevels, const uint8_t *const *ref_bgr,
                                        const float *const *ref_depth, const uint8_t *const *now_bgr, const ea_ros_frame_params *prm,
                                        bool on_device) {
  // every check comes before a device or a problem is touched
  if (!levels || !prm) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (nlevels < 1 || nlevels > kPyramidMaxLevels) return fail(EA_ERR_INVALID_ARG, "a pyramid has 1..9 levels");
  for (int l = 0; l < nlevels; ++l)
    if (!levels[l]) return fail(EA_ERR_INVALID_ARG, "NULL level");
  const int full_h = prm->full_height, full_w = prm->full_width, halvings = prm->halvings;
  if (full_h < 3 || full_w < 3 || full_h > 32768 || full_w > 32768 || (int64_t)full_h * full_w > 0x3fffffff)
    return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  if (halvings < 0 || halvings + nlevels - 1 > 8) return fail(EA_ERR_INVALID_ARG, "halvings + levels - 1 must be within 0..8");
  const int T = halvings + nlevels - 1;
  int rc = check_scaled_args(full_h, full_w, T);
  if (rc != EA_OK) return rc;
  int lo, hi;
  rc = ros_thresholds(prm->threshold1, prm->threshold2, &lo, &hi);
  if (rc != EA_OK) return rc;
  if ((full_h >> T) < 3 || (full_w >> T) < 3) return fail(EA_ERR_INVALID_ARG, "image extent out of range: the coarsest level is below 3 x 3");
  std::vector<BatchFrames> J((size_t)nlevels);
  const void *const *ref_depth_v = reinterpret_cast<const void *const *>(ref_depth);
  std::vector<const ea_problem *> all;
  for (int l = 0; l < nlevels; ++l) {
    BatchFrames &j = J[(size_t)l];
    j.ros = true; j.full_H = full_h; j.full_W = full_w; j.halvings = halvings + l;
    // (the caller's device frames are looked at once, with level 0)
    rc = batch_frames_check(levels[l], ref_bgr, ref_depth_v, sizeof(float), now_bgr, nullptr, full_h >> j.halvings, full_w >> j.halvings,
                            /*z_scaling (metres already)=*/1.0, on_device && l == 0, &j);
    if (rc != EA_OK) return rc;
    j.on_device = on_device;
    if (j.count != J[0].count) return fail(EA_ERR_INVALID_ARG, "the levels' batches differ in count");
    if (j.device != J[0].device) return fail(EA_ERR_INVALID_ARG, "the levels' batches are on different devices");
    for (int i = 0; i < j.count; ++i) {
      if (j.probs[i]->dtype != J[0].dtype) return fail(EA_ERR_INVALID_ARG, "the levels' problems differ in dtype");
      all.push_back(j.probs[i]);
    }
  }
  std::sort(all.begin(), all.end());
  if (std::adjacent_find(all.begin(), all.end()) != all.end())
    return fail(EA_ERR_INVALID_ARG, "the same problem on two levels: each level of each frame pair needs a problem of its own");

  FramePyramid py;
  rc = pyramid_frames_begin(levels, &J, halvings, ref_bgr, ref_depth_v, now_bgr, &py);
  if (rc != EA_OK) return rc;
  batch_frames_set_uploaded(levels[0], 0);
  std::vector<int> total_looks((size_t)nlevels, 0);
  int looks = 0;
  int64_t uploads = 0;
  for (BatchFrames &j : J) HIPCHK(upload_table(&j));  // where the frames are read, the cameras, the depth weighting
  if (J[0].ref) {
    rc = pyramid_stage_side(J, py, halvings, 0, ref_bgr, ref_depth, &uploads);
    batch_frames_set_uploaded(levels[0], uploads);
    if (rc != EA_OK) return rc;
    for (int l = 0; l < nlevels; ++l) {
      BatchFrames &j = J[(size_t)l];
      rc = batch_canny(j, 0, false, lo, hi, /*l2_bgr=*/1, &looks);
      batch_frames_set_rounds(levels[l], total_looks[(size_t)l] += looks);
      if (rc == EA_OK) rc = batch_ref_counts(&j, j.ws.edges, 0);
      if (rc == EA_OK) rc = batch_ros_scatter(&j);
      if (rc != EA_OK) return rc;
    }
  }
  std::vector<int> rc_dt((size_t)nlevels, EA_OK);
  int first_bare_level = -1, bare_all = 0;
  if (J[0].now) {
    // (every level's scatter reads that level's `edges` and `depth` and is in front of this on the same stream)
    rc = pyramid_stage_side(J, py, halvings, 1, now_bgr, nullptr, &uploads);
    batch_frames_set_uploaded(levels[0], uploads);
    if (rc != EA_OK) return rc;
    for (int l = 0; l < nlevels; ++l) {
      int bare = 0;
      rc = batch_ros_now(&J[(size_t)l], lo, hi, &looks, &bare, &rc_dt[(size_t)l]);
      batch_frames_set_rounds(levels[l], total_looks[(size_t)l] += looks);
      batch_frames_set_without_edges(levels[l], bare);
      if (rc != EA_OK) return rc;
      if (bare > 0 && bare_all == 0) first_bare_level = l;
      bare_all += bare;
    }
  }
  rc = EA_OK;
  for (int l = 0; l < nlevels; ++l) {
    const int rc_l = batch_frames_end(J[(size_t)l], rc_dt[(size_t)l]);  // (the first waits, the others find the device idle)
    if (rc == EA_OK) rc = rc_l;
  }
  if (rc == EA_OK && bare_all > 0) {
    const std::vector<unsigned char> &none = J[(size_t)first_bare_level].no_image;
    return fail(EA_ERR_STATE, "no edge in " + std::to_string(bare_all) + " of the current frames' levels, the first at level " +
                                  std::to_string(first_bare_level) + ", index " +
                                  std::to_string(std::find(none.begin(), none.end(), 1) - none.begin()) +
                                  ": the exact distance transform is undefined");
  }
  return rc;
}

extern "C" int ea_batch_set_frames_ros_pyramid(ea_batch *const *levels, int nlevels, const uint8_t *const *ref_bgr,
                                               const float *const *ref_depth, const uint8_t *const *now_bgr,
                                               const ea_ros_frame_params *prm) {
  return batch_set_frames_ros_pyramid(levels, nlevels, ref_bgr, ref_depth, now_bgr, prm, false);
}

extern "C" int ea_batch_set_frames_ros_pyramid_device(ea_batch *const *levels, int nlevels, const uint8_t *const *ref_bgr,
                                                      const float *const *ref_depth, const uint8_t *const *now_bgr,
                                                      const ea_ros_frame_params *prm) {
  return batch_set_frames_ros_pyramid(levels, nlevels, ref_bgr, ref_depth, now_bgr, prm, true);
}

// The halving chain by itself (host in, host out), the sibling of ea_resize_half: levels skip .. skip + keep - 1 of one
// frame, level k = k halvings, from one upload.  Level 0 (skip == 0) is the frame as handed in; kind 1 replaces NaN on the
// chain's first step only, so from level 1 on.
extern "C" int ea_resize_half_levels(int device, int kind, const void *src, int height, int width, int skip, int keep,
                                     void *const *dst) {
  if (!src || !dst) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (kind < 0 || kind > 2) return fail(EA_ERR_INVALID_ARG, "kind must be 0 (bgr8), 1 (float32, NaN -> 0) or 2 (float32)");
  if (skip < 0 || keep < 1 || skip + keep - 1 > 8) return fail(EA_ERR_INVALID_ARG, "skip >= 0, keep >= 1, skip + keep - 1 <= 8");
  const int T = skip + keep - 1;
  if (height < 1 || width < 1 || height > 32768 || width > 32768 || (int64_t)height * width > 0x3fffffff || (height >> T) < 1 ||
      (width >> T) < 1 || (height % (1 << T)) != 0 || (width % (1 << T)) != 0)
    return fail(EA_ERR_INVALID_ARG, "frame extent must be divisible by 2^(skip + keep - 1) and in range");
  for (int k = 0; k < keep; ++k)
    if (!dst[k]) return fail(EA_ERR_INVALID_ARG, "NULL level");
  const size_t np = (size_t)height * width, es = kind == 0 ? 3 : 4;
  if (skip == 0) std::memcpy(dst[0], src, np * es);
  if (T == 0) return EA_OK;
  int rc = check_device(device);
  if (rc != EA_OK) return rc;
  HIPCHK(hipSetDevice(device));
  // the frame, and behind it room for every level 1..T at 256-aligned offsets (levels that are passed through stay unused)
  std::vector<size_t> off((size_t)T + 1, 0);
  size_t bytes = (np * es + 255) & ~(size_t)255;
  for (int k = 1; k <= T; ++k) {
    off[(size_t)k] = bytes;
    bytes += ((np >> (2 * k)) * es + 255) & ~(size_t)255;
  }
  DevBuf a;
  HIPCHK(cached_malloc(&a.p, bytes, device));
  HIPCHK(hipMemcpy(a.p, src, np * es, hipMemcpyHostToDevice));
  FramesLaunch f;
  f.n = 1;
  auto dst_of = [&](int k) -> void * { return k >= skip || k == 3 || k == 6 ? a.as<unsigned char>() + off[(size_t)k] : nullptr; };
  if (kind == 0) rc = halving_chain<uint8_t>(f, nullptr, a.as<uint8_t>(), height, width, T, dst_of, 0);
  else rc = halving_chain<float>(f, nullptr, a.as<float>(), height, width, T, dst_of, kind == 1 ? 1 : 0);
  if (rc != EA_OK) return rc;
  for (int k = std::max(skip, 1); k <= T; ++k)
    HIPCHK(hipMemcpy(dst[k - skip], a.as<unsigned char>() + off[(size_t)k], (np >> (2 * k)) * es, hipMemcpyDeviceToHost));
  return EA_OK;
}

// ---- the multi-stream tracker: ea_tracker for N streams pushed in lock-step, on the batched producers and ONE batch solve ----
//
// Every pushed frame passes the edge detection once (launch_edge_strength_frames / launch_canny_frames, the frame a grid
// dimension) and what that leaves in its workspace serves both sides: the current-side tail (threshold + chamfer, or the exact
// transform, then the store into the stream's image) and, behind the solve, the reference-side tail (count, scan, scatter,
// depth weights).  Both sides of a slot name the same frame, so every step is a kernel the batched producers have already.
// A tracker has L >= 1 levels (ea_tracker_batch_create_pyramid, the ROS flavour: level l works at halvings + l), each with
// problems, a batch and sub-batches of its own; ONE push (tracker_batch_push) serves every flavour and every L, as phases over
// one TrackerPush, all on the null stream but the solves:
//   checks            tracker_push_check: nothing is touched before they have passed
//   frames in place   tracker_push_frames: table and frames up (device frames: read in place) [-> ROS: halvings; L > 1: the
//                     frames go up once and one halving chain per kind leaves every level's frame in its workspace]
//   images, per level tracker_push_images: edge pass -> [ROS: count + scan, the counts back (wait): a frame without an edge
//                     has no image] -> chamfer / exact transform -> store; then ONE wait (the images are complete)
//                     -> [Laplacian, Canny: count + scan queued, it runs beside the solves]
//   priors            tracker_push_priors: the aligned streams (level 0's rule), their motion priors on every usable level
//   descent           tracker_push_descent: for l = L - 1 .. 0 ea_batch_solve of the streams still descending that can use l,
//                     on the batches' own streams, the pose carried down; a single level is this loop run once.  With a
//                     depth gate set (ea_tracker_batch_set_depth_gate) each solve is preceded by the gate of its streams at
//                     the pose they carry in, on the same batch and stream: one launch and one wait per solved (level, group)
//   covariance        tracker_push_covariance: [ea_batch_covariance] [keyframe mode: ea_batch_pose_stats] at level 0
//   references, per level   tracker_push_references: [Laplacian, Canny: the counts back (wait)] -> room for the points ->
//                     table up -> scatter -> depth weights; then the last wait
//   bookkeeping       tracker_push_book
// (The ROS chain needs its counts before the transform, and its count has no depth test: the same counts serve the scatter.)
// Waits per push outside the solves: the hysteresis looks (Canny, ROS), the images, the counts, the end.

namespace {
struct TrackerStream {
  int frames = 0;
  double q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 0};
  bool cov_valid = false;
  ea_covariance cov_last{};
  bool motion_set = false;
  PriorDesc installed = {};
  ea_keyframe_state key{};  // ea_tracker_batch_set_keyframes
};
}  // namespace

struct ea_tracker_batch {
  // One level of every stream (ea_tracker_batch_create: one; _create_pyramid: levels, lv[0] the finest): its problems, the
  // batch over them -- the solve when all are aligned; lv[0]'s also owns the frame workspace of every level -- and the
  // sub-batches (streams, their batch) that solve fewer than all streams
  struct Level {
    std::vector<ea_problem *> probs;
    ea_batch *b = nullptr;
    std::vector<std::pair<std::vector<int>, ea_batch *>> subs;
  };
  std::vector<Level> lv;
  std::vector<TrackerStream> st;
  int flavour = 0, halvings = 0, device = 0, levels = 1;
  std::vector<ea_summary> last_sums;  // levels x streams, level-major: ea_tracker_batch_last_summaries
  bool cov_on = false;
  ea_covariance_options cov_opt{};
  double sigma_rot = 0.0, sigma_trans = 0.0;
  // ea_tracker_batch_get_info
  int last_aligned = 0, last_bare = 0, last_rounds = 0, last_edge_passes = 0;
  int64_t pushes = 0;
  // keyframe mode (ea_tracker_batch_set_keyframes): off = every pushed frame becomes every stream's reference
  bool key_on = false;
  ea_keyframe_params key_prm{};
  int last_taken = 0;
  // depth gate (ea_tracker_batch_set_depth_gate): off = no launch of it
  bool gate_on = false;
  ea_depth_gate_params gate_prm{};
  std::vector<ea_depth_gate_stats> last_gate;  // levels x streams, level-major: ea_tracker_batch_last_depth_gate
  int last_gated = 0;
  bool gate_applies() const { return gate_on && gate_prm.apply != 0; }
  // point selection (ea_tracker_batch_set_point_selection): off = no launch of it
  bool sel_on = false;
  ea_point_selection sel_prm{};
  std::vector<ea_point_selection_stats> last_sel;  // levels x streams, level-major: the push that selected each reference
  int last_selected = 0;
  // points carried across a keyframe replacement (ea_tracker_batch_set_point_carry): off = no launch of it
  bool carry_on = false;
  ea_point_merge carry_prm{};
  std::vector<ea_point_merge_stats> last_carry;  // per stream: the merge of the last push (zeros: it did not carry)
  int last_carried = 0;
};

static int tracker_batch_create(ea_tracker_batch **out, const ea_camera *cams, int count, int levels, int dtype, int device,
                                int flavour, int halvings) {
  if (!out || !cams) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (count < 1 || count > 65535) return fail(EA_ERR_INVALID_ARG, "a multi-stream tracker takes 1..65535 streams");
  if (flavour < 0 || flavour > 2) return fail(EA_ERR_INVALID_ARG, "unknown pre-processing flavour");
  if (halvings < 0 || halvings > 8) return fail(EA_ERR_INVALID_ARG, "halvings out of range");
  if (flavour != 2 && halvings != 0) return fail(EA_ERR_INVALID_ARG, "halvings belong to the ROS flavour (2) only");
  if (levels < 1 || halvings + levels - 1 > 8) return fail(EA_ERR_INVALID_ARG, "levels >= 1 and halvings + levels - 1 <= 8");
  ea_tracker_batch *tb = new (std::nothrow) ea_tracker_batch;
  if (!tb) return fail(EA_ERR_ALLOC, "out of host memory");
  tb->flavour = flavour; tb->halvings = halvings; tb->device = device; tb->levels = levels;
  tb->lv.resize((size_t)levels);
  int rc = EA_OK;
  for (int l = 0; l < levels && rc == EA_OK; ++l) {
    ea_tracker_batch::Level &lv = tb->lv[(size_t)l];
    for (int i = 0; i < count && rc == EA_OK; ++i) {
      ea_problem *p = nullptr;
      rc = ea_problem_create(&p, cams + (size_t)l * count + i, dtype, device);
      if (rc == EA_OK) lv.probs.push_back(p);
    }
    if (rc == EA_OK) rc = ea_batch_create(&lv.b, lv.probs.data(), count);
  }
  if (rc != EA_OK) { ea_tracker_batch_destroy(tb); return rc; }
  tb->st.resize((size_t)count);
  tb->last_sums.resize((size_t)levels * count);
  std::memset(tb->last_sums.data(), 0, tb->last_sums.size() * sizeof(ea_summary));
  tb->last_gate.assign((size_t)levels * count, ea_depth_gate_stats{});
  tb->last_sel.assign((size_t)levels * count, ea_point_selection_stats{});
  tb->last_carry.assign((size_t)count, ea_point_merge_stats{});
  *out = tb;
  return EA_OK;
}

extern "C" int ea_tracker_batch_create(ea_tracker_batch **out, const ea_camera *cams, int count, int dtype, int device, int flavour,
                                       int halvings) {
  return tracker_batch_create(out, cams, count, 1, dtype, device, flavour, halvings);
}

extern "C" int ea_tracker_batch_create_pyramid(ea_tracker_batch **out, const ea_camera *cams, int count, int levels, int dtype,
                                               int device, int halvings) {
  return tracker_batch_create(out, cams, count, levels, dtype, device, /*flavour=*/2, halvings);
}

extern "C" void ea_tracker_batch_destroy(ea_tracker_batch *tb) {
  if (!tb) return;
  for (ea_tracker_batch::Level &lv : tb->lv) {
    for (auto &s : lv.subs) ea_batch_destroy(s.second);
    ea_batch_destroy(lv.b);
    for (ea_problem *p : lv.probs) ea_problem_destroy(p);
  }
  delete tb;
}

extern "C" int ea_tracker_batch_count(const ea_tracker_batch *tb) { return tb ? (int)tb->st.size() : 0; }

extern "C" ea_problem *ea_tracker_batch_level_problem(ea_tracker_batch *tb, int level, int i) {
  return tb && level >= 0 && level < tb->levels && i >= 0 && (size_t)i < tb->st.size() ? tb->lv[(size_t)level].probs[(size_t)i] : nullptr;
}

extern "C" ea_problem *ea_tracker_batch_problem(ea_tracker_batch *tb, int i) { return ea_tracker_batch_level_problem(tb, 0, i); }

extern "C" int ea_tracker_batch_last_summaries(ea_tracker_batch *tb, int i, ea_summary *out) {
  if (!tb || !out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (i < 0 || (size_t)i >= tb->st.size()) return fail(EA_ERR_INVALID_ARG, "no such stream");
  for (int l = 0; l < tb->levels; ++l) out[l] = tb->last_sums[(size_t)l * tb->st.size() + (size_t)i];
  return EA_OK;
}

// a stream without a reference: the next push starts a fresh chain for it
static void tracker_stream_drop(ea_tracker_batch *tb, size_t i) {
  for (const ea_tracker_batch::Level &lv : tb->lv) {
    (void)reserve_points(lv.probs[i], 0);
    lv.probs[i]->version++;
  }
  for (int l = 0; l < tb->levels; ++l) tb->last_sel[(size_t)l * tb->st.size() + i] = ea_point_selection_stats{};
  tb->last_carry[i] = ea_point_merge_stats{};
  tb->st[i].frames = 0;
  tb->st[i].cov_valid = false;
  tb->st[i].key = ea_keyframe_state{};
}

// A push that failed past its checks: some streams' images are the new frame's, some references may be, nothing says which.
// Nothing of the push stays in flight, and every stream starts a fresh chain.
static int tracker_batch_fail(ea_tracker_batch *tb, int rc) {
  const std::string why = ea_last_error();  // (the clean-up below may not overwrite what failed)
  (void)hipDeviceSynchronize();
  (void)hipGetLastError();
  for (size_t i = 0; i < tb->st.size(); ++i) tracker_stream_drop(tb, i);
  tb->last_aligned = 0;
  return fail(rc, why);
}
// a step of a push (its tracker: `tb`) that fails takes the push with it: tracker_batch_fail, and its code is returned
#define TBCHK(expr)                                                                                                            \
  do {                                                                                                                         \
    const hipError_t e_ = (expr);                                                                                              \
    if (e_ != hipSuccess) { (void)fail(EA_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); return tracker_batch_fail(tb, EA_ERR_HIP); } \
  } while (0)
#define TBRC(expr)                                          \
  do {                                                      \
    const int rc_ = (expr);                                 \
    if (rc_ != EA_OK) return tracker_batch_fail(tb, rc_);   \
  } while (0)

// the batch that solves exactly the streams in `members`: the level's own when that is all of them, else one of the few
// sub-batches it keeps (the same streams tend to be aligned push after push; the oldest makes room)
static int tracker_batch_solver(ea_tracker_batch *tb, const std::vector<int> &members, ea_batch **out, int level) {
  ea_tracker_batch::Level &lv = tb->lv[(size_t)level];
  if (members.size() == lv.probs.size()) { *out = lv.b; return EA_OK; }
  std::vector<std::pair<std::vector<int>, ea_batch *>> &subs = lv.subs;
  for (size_t k = 0; k < subs.size(); ++k)
    if (subs[k].first == members) { *out = subs[k].second; return EA_OK; }
  constexpr size_t kKeptSubBatches = 4;
  if (subs.size() >= kKeptSubBatches) {
    ea_batch_destroy(subs.front().second);
    subs.erase(subs.begin());
  }
  std::vector<ea_problem *> probs;
  for (int i : members) probs.push_back(lv.probs[(size_t)i]);
  ea_batch *sub = nullptr;
  const int rc = ea_batch_create(&sub, probs.data(), (int)probs.size());
  if (rc != EA_OK) return rc;
  subs.emplace_back(members, sub);
  *out = sub;
  return EA_OK;
}

// The aligned streams in the groups that are solved together.  A batch runs ONE kernel family for all its problems: a problem
// with per-point weights, distortion or a second camera puts its neighbours on the variant kernels, whose sums agree with the
// plain kernels' to rounding only.  Streams are therefore grouped by what their own problem needs (term_variant), so that each
// is solved by the kernels, and to the bits, of a tracker of its own; a problem with further terms is a group by itself.
// Streams with the same settings -- the usual case -- are one group: one solve.
static std::vector<std::vector<int>> tracker_batch_groups(const ea_tracker_batch *tb, const std::vector<int> &al, int level) {
  std::vector<std::vector<int>> groups;
  std::vector<int> keys;
  for (int i : al) {
    const ea_problem *p = tb->lv[(size_t)level].probs[(size_t)i];
    const int key = p->terms.empty() ? term_variant(p) : -1 - i;
    size_t g = 0;
    while (g < keys.size() && keys[g] != key) ++g;
    if (g == keys.size()) { keys.push_back(key); groups.emplace_back(); }
    groups[g].push_back(i);
  }
  return groups;
}

// What a push carries from phase to phase (tracker_batch_push; the block comment above names the phases)
namespace {
struct TrackerPush {
  ea_tracker_batch *tb = nullptr;
  const uint8_t *const *bgr = nullptr;  // the pushed frames: the reference side's and the current side's of every slot
  const void *const *depth = nullptr;
  double z_scaling = 0.0;
  const ea_options *opt = nullptr;
  ea_summary *summaries = nullptr;  // the caller's (nullable)
  bool on_device = false;
  int lo = 0, hi = 0;               // the flavour's hysteresis thresholds
  std::vector<BatchFrames> J;       // the levels' jobs
  std::vector<int> al;              // the aligned streams
  // per stream: the pose its solve started from, the one it carries down the levels, and the one it returned
  std::vector<double> q0, t0, qc, tc, qs, ts;
  std::vector<unsigned char> stopped, is_al;  // its descent ended in a failed solve; it was aligned
  std::vector<ea_pose_stats> kstats;          // keyframe mode: the statistics at the pose its solve returned
  std::vector<unsigned char> take;            // the pushed frame becomes its reference: every stream's, but in keyframe mode
  std::vector<int> why;                       // keyframe mode: why (keyframe_decide)
  WsRegion<float> depth_full;                 // (ROS, host frames, halvings >= 1) the stage's full-size depth in a frame's block
  bool ros() const { return tb->flavour == 2; }
  // The depth gate's image of stream i: the pushed depth frame at full resolution where the push has put it -- the caller's
  // device frame in place; of a host frame the `depth` region of level 0's workspace (uint16, or the ROS flavour's float
  // frame without halvings) or the stage's depth_full.  Written by the upload alone and read-only to every kernel behind it
  // (the halving steps and chains read it through const pointers and write other regions; no region of a frame's block
  // shares bytes with another), so it is what was pushed until the next push.
  const void *gate_depth(size_t i) const {
    if (on_device) return depth[i];
    const BatchFrames &j0 = J[0];
    return ros() && tb->halvings > 0 ? depth_full.at<unsigned char>(j0.frame(i)) : j0.ws.depth.at<unsigned char>(j0.frame(i));
  }
  // what the reference side counts and scatters
  const WsRegion<uint8_t> &ref_edges(const BatchFrames &j) const { return tb->flavour == 0 ? j.ws.lap : j.ws.edges; }
  int ref_threshold() const { return tb->flavour == 0 ? 35 : 0; }
  // a level takes part in a stream's solve when its reference has points and its frame has an edge
  bool usable(int l, size_t i) const {
    const std::vector<unsigned char> &none = J[(size_t)l].no_image;
    return tb->lv[(size_t)l].probs[i]->n > 0 && (none.empty() || !none[i]);
  }
};
}  // namespace

// Checks: every one comes before a device or a stream is touched -- a rejected call leaves the tracker as it was.
static int tracker_push_check(TrackerPush *s, int height, int width) {
  const ea_tracker_batch *tb = s->tb;
  if (height < 3 || width < 3 || height > 32768 || width > 32768 || (int64_t)height * width > 0x3fffffff)
    return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  const int L = tb->levels, T = tb->halvings + L - 1;
  int rc = check_scaled_args(height, width, T);
  if (rc != EA_OK) return rc;
  // (a coarsest level that is too small: with levels the pyramid producer's words, here; on a single level batch_frames_check's, below)
  if (L > 1 && ((height >> T) < 3 || (width >> T) < 3))
    return fail(EA_ERR_INVALID_ARG, "image extent out of range: the coarsest level is below 3 x 3");
  const bool ros = s->ros();
  rc = tb->flavour == 0 ? EA_OK : ros ? ros_thresholds(150.0, 100.0, &s->lo, &s->hi) : canny_thresholds(30.0, 90.0, &s->lo, &s->hi);
  if (rc != EA_OK) return rc;
  // (as the producers of ea_tracker's flavours: the Canny reference refuses an infinite z_scaling, the Laplacian one takes it)
  if (tb->flavour == 1 && !(s->z_scaling <= DBL_MAX)) return fail(EA_ERR_INVALID_ARG, "z_scaling must be > 0 and finite");
  if (s->opt) {
    rc = check_options(*s->opt);
    if (rc != EA_OK) return rc;
  }
  s->J.resize((size_t)L);
  for (int l = 0; l < L; ++l) {
    BatchFrames &j = s->J[(size_t)l];
    j.ros = ros; j.full_H = height; j.full_W = width; j.halvings = tb->halvings + l;
    // (both sides of every slot are the pushed frame; the caller's device frames are looked at once, with level 0)
    rc = batch_frames_check(tb->lv[(size_t)l].b, s->bgr, s->depth, ros ? sizeof(float) : 2, s->bgr, nullptr, height >> j.halvings,
                            width >> j.halvings, ros ? 1.0 : s->z_scaling, s->on_device && l == 0, &j);
    if (rc != EA_OK) return rc;
    j.on_device = s->on_device;
  }
  return EA_OK;
}

// Frames in place: the jobs' memory, the table up, and every level's frame at its working resolution in that level's
// workspace.  The one phase in which the level count selects a path: a single level is laid out by frame_stage and halved
// one step per launch (batch_stage_ros), several by frame_pyramid and one halving chain per kind (pyramid_stage_side).
static int tracker_push_frames(TrackerPush *s) {
  ea_tracker_batch *tb = s->tb;
  const float *const *depth_f32 = reinterpret_cast<const float *const *>(s->depth);
  if (tb->levels > 1) {
    std::vector<ea_batch *> batches;
    for (const ea_tracker_batch::Level &lv : tb->lv) batches.push_back(lv.b);
    FramePyramid py;
    int64_t uploads = 0;
    TBRC(pyramid_frames_begin(batches.data(), &s->J, tb->halvings, s->bgr, s->depth, s->bgr, &py));
    for (BatchFrames &j : s->J) TBCHK(upload_table(&j));
    TBRC(pyramid_stage_side(s->J, py, tb->halvings, 0, s->bgr, depth_f32, &uploads));
    s->depth_full = py.depth_full;
    return EA_OK;
  }
  BatchFrames &j = s->J[0];
  TBRC(batch_frames_begin(tb->lv[0].b, s->bgr, s->depth, s->bgr, nullptr, &j));
  if (s->ros()) {
    TBCHK(upload_table(&j));
    TBRC(batch_stage_ros(j, 0, s->bgr, depth_f32));
    s->depth_full = j.st.depth_full;
    return EA_OK;
  }
  // (Laplacian, Canny: no count comes before the transform, so the table goes up with the images in it)
  TBRC(batch_alloc_dts(&j));
  TBCHK(upload_table(&j));
  if (!s->on_device) {
    TBRC(upload_frames(j, j.ws.bgr, s->bgr, j.np * 3));
    TBRC(upload_frames(j, j.ws.depth, s->depth, j.np * 2));
  }
  return EA_OK;
}

// Images: on every level the frame passes the edge detection once and the current-side tail stores every stream's image; one
// wait, because the solves run on the batches' streams, which do not wait for the null stream.  Laplacian, Canny: the frame's
// edge pixels are then counted WHILE the previous references are solved against the images just produced (null stream beside
// the solve's non-blocking streams; neither touches what the other uses).
static int tracker_push_images(TrackerPush *s) {
  ea_tracker_batch *tb = s->tb;
  for (int l = 0; l < tb->levels; ++l) {
    BatchFrames &j = s->J[(size_t)l];
    ea_batch *b = tb->lv[(size_t)l].b;
    const FrameWs &ws = j.ws;
    unsigned char *base = j.base;
    int looks = 0;
    tb->last_edge_passes++;
    if (s->ros()) {
      int bare = 0, rc_dt = EA_OK;
      const int rc = batch_ros_now(&j, s->lo, s->hi, &looks, &bare, &rc_dt);
      tb->last_rounds += looks;
      batch_frames_set_rounds(b, looks);
      if (l == 0) tb->last_bare = bare;
      batch_frames_set_without_edges(b, bare);
      TBRC(rc);
      TBRC(rc_dt);
      continue;
    }
    if (tb->flavour == 0) {
      TBCHK(launch_edge_strength_frames(j.f, 1, ws.gray.at(base), ws.lap.at(base), nullptr));
      TBCHK(launch_threshold_median_frames(j.f, ws.lap.at(base), 35, 1, ws.mask.at(base), nullptr));
    } else {
      const int rc = batch_canny(j, 1, false, s->lo, s->hi, /*l2_bgr=*/0, &looks);
      tb->last_rounds += looks;
      batch_frames_set_rounds(b, looks);
      TBRC(rc);
    }
    TBCHK(launch_chamfer_frames(j.f, (tb->flavour == 0 ? ws.mask : ws.inv).at(base), ws.G.at(base), ws.scan.at(base), ws.dist.at(base),
                                nullptr, ws.minmax.at(base), nullptr));
    TBCHK(launch_dt_store_frames(j.dtype, j.f, ws.dist.at(base), ws.minmax.at(base), 1, 0.0, 1.0, nullptr));
  }
  TBCHK(hipStreamSynchronize(nullptr));
  for (int l = 0; l < tb->levels; ++l) {
    const std::vector<unsigned char> &none = s->J[(size_t)l].no_image;
    for (size_t i = 0; i < tb->st.size(); ++i)
      if (none.empty() || !none[i]) dt_landed(tb->lv[(size_t)l].probs[i]);
  }
  if (!s->ros()) TBRC(batch_counts_queue(&s->J[0], s->ref_edges(s->J[0]), s->ref_threshold()));
  return EA_OK;
}

// Priors: a stream is aligned by level 0's rule and starts from its last relative pose; with a motion prior on, every
// usable level of every aligned stream carries it, centred on that pose.
static int tracker_push_priors(TrackerPush *s) {
  ea_tracker_batch *tb = s->tb;
  const size_t n = tb->st.size();
  for (size_t i = 0; i < n; ++i)
    if (tb->st[i].frames > 0 && s->usable(0, i)) s->al.push_back((int)i);
  s->q0.resize(4 * n); s->t0.resize(3 * n); s->qs.resize(4 * n); s->ts.resize(3 * n);
  s->stopped.assign(n, 0); s->is_al.assign(n, 0);
  if (tb->key_on) s->kstats.assign(n, ea_pose_stats{});
  for (int a : s->al) {
    const size_t i = (size_t)a;
    TrackerStream &st = tb->st[i];
    s->is_al[i] = 1;
    std::memcpy(&s->q0[4 * i], st.q, sizeof(st.q));
    std::memcpy(&s->t0[3 * i], st.t, sizeof(st.t));
    if (tb->sigma_rot > 0.0 || tb->sigma_trans > 0.0) {
      for (int l = 0; l < tb->levels; ++l)
        if (s->usable(l, i)) TBRC(motion_prior_install(tb->lv[(size_t)l].probs[i], tb->sigma_rot, tb->sigma_trans, st.q, st.t));
      st.motion_set = true;
      st.installed = tb->lv[0].probs[i]->prior;
    }
  }
  s->qc = s->q0; s->tc = s->t0;
  return EA_OK;
}

// the poses of a group's streams, in the group's order, as a batch call takes them
static void tracker_group_poses(const std::vector<int> &grp, const std::vector<double> &q, const std::vector<double> &t,
                                std::vector<double> *qg, std::vector<double> *tg) {
  qg->resize(4 * grp.size()); tg->resize(3 * grp.size());
  for (size_t k = 0; k < grp.size(); ++k) {
    std::memcpy(&(*qg)[4 * k], &q[4 * (size_t)grp[k]], 4 * sizeof(double));
    std::memcpy(&(*tg)[3 * k], &t[3 * (size_t)grp[k]], 3 * sizeof(double));
  }
}

// The depth gate of one group in front of its solve on level l: ea_batch_depth_gate's kernel on the batch that solves the group,
// at the poses the streams carry into the level, against the pushed depth at full resolution (the ROS flavour: 2^(halvings + l)
// times the level's extent -- the level's own depth is the reference's reduction, NaN -> 0 and the plain mean, which a hole
// pulls towards the camera).  apply: the weights of the group's level problems are written before the solve reads them.
static int tracker_gate_group(TrackerPush *s, int l, const std::vector<int> &grp, ea_batch *solver, const std::vector<double> &qg,
                              const std::vector<double> &tg) {
  ea_tracker_batch *tb = s->tb;
  const size_t ng = grp.size(), n = tb->st.size();
  std::vector<double> M(16 * ng);
  std::vector<const void *> depth(ng);
  std::vector<ea_depth_gate_stats> stats(ng);
  for (size_t k = 0; k < ng; ++k) {
    (void)ea_pose_to_matrix(&qg[4 * k], &tg[3 * k], &M[16 * k]);
    depth[k] = s->gate_depth((size_t)grp[k]);
  }
  GateImages img;
  img.kind = s->ros() ? EA_DEPTH_F32 : EA_DEPTH_U16;
  img.shift = s->ros() ? tb->halvings + l : 0;
  img.z_scaling = s->ros() ? 1.0 : s->z_scaling;
  img.depth = depth.data();
  TBRC(batch_depth_gate_images(solver, M.data(), &tb->gate_prm, img, stats.data()));
  for (size_t k = 0; k < ng; ++k) tb->last_gate[(size_t)l * n + (size_t)grp[k]] = stats[k];
  tb->last_gated += (int)ng;
  return EA_OK;
}

// Descent: ea_solve_pyramid per stream, run as batch solves -- the coarsest level first, on each level the streams still
// descending that can use it, grouped by kernel family, the pose carried down.  A failed solve stops its stream's descent: it
// keeps its prior.  A single level is this loop run once.
static int tracker_push_descent(TrackerPush *s) {
  ea_tracker_batch *tb = s->tb;
  const size_t n = tb->st.size();
  std::vector<double> qg, tg;
  for (int l = tb->levels - 1; l >= 0; --l) {
    std::vector<int> members;
    for (int i : s->al)
      if (!s->stopped[(size_t)i] && s->usable(l, (size_t)i)) members.push_back(i);
    for (const std::vector<int> &grp : tracker_batch_groups(tb, members, l)) {
      ea_batch *solver = nullptr;
      TBRC(tracker_batch_solver(tb, grp, &solver, l));
      std::vector<ea_summary> sg(grp.size());
      tracker_group_poses(grp, s->qc, s->tc, &qg, &tg);
      if (tb->gate_on) {
        const int rc_gate = tracker_gate_group(s, l, grp, solver, qg, tg);
        if (rc_gate != EA_OK) return rc_gate;
      }
      TBRC(ea_batch_solve(solver, s->opt, qg.data(), tg.data(), sg.data()));
      for (size_t k = 0; k < grp.size(); ++k) {
        const size_t i = (size_t)grp[k];
        tb->last_sums[(size_t)l * n + i] = sg[k];
        if (s->summaries) s->summaries[i] = sg[k];  // (the finest level the descent reaches comes last)
        if (sg[k].termination == EA_FAILURE) { s->stopped[i] = 1; continue; }
        std::memcpy(&s->qc[4 * i], &qg[4 * k], 4 * sizeof(double));
        std::memcpy(&s->tc[3 * i], &tg[3 * k], 3 * sizeof(double));
      }
    }
  }
  for (int a : s->al) {
    const size_t i = (size_t)a;
    std::memcpy(&s->qs[4 * i], s->stopped[i] ? &s->q0[4 * i] : &s->qc[4 * i], 4 * sizeof(double));
    std::memcpy(&s->ts[3 * i], s->stopped[i] ? &s->t0[3 * i] : &s->tc[3 * i], 3 * sizeof(double));
  }
  return EA_OK;
}

// Covariance and (keyframe mode) pose statistics: at level 0, at the returned poses, per kernel family as the solves, from the
// points and images the solves used -- both calls return once their results have landed, and the scatter that overwrites the
// points is queued behind that.  A stopped descent has no pose to take either at: its covariance reports why = 4, its
// statistics stay zero, and a group without a surviving stream makes no call.
static int tracker_push_covariance(TrackerPush *s) {
  ea_tracker_batch *tb = s->tb;
  if (!tb->cov_on && !tb->key_on) return EA_OK;
  std::vector<double> qg, tg;
  for (const std::vector<int> &grp : tracker_batch_groups(tb, s->al, 0)) {
    const size_t ng = grp.size();
    ea_batch *solver = nullptr;
    TBRC(tracker_batch_solver(tb, grp, &solver, 0));
    tracker_group_poses(grp, s->qs, s->ts, &qg, &tg);
    size_t ok = 0;
    for (int i : grp) ok += s->stopped[(size_t)i] ? 0 : 1;
    if (tb->cov_on) {
      std::vector<ea_covariance> covs(ng);
      std::memset(covs.data(), 0, ng * sizeof(ea_covariance));
      if (ok > 0) TBRC(ea_batch_covariance(solver, qg.data(), tg.data(), &tb->cov_opt, covs.data()));
      for (size_t k = 0; k < ng; ++k) {
        TrackerStream &st = tb->st[(size_t)grp[k]];
        st.cov_last = covs[k];
        if (s->stopped[(size_t)grp[k]]) {
          std::memset(&st.cov_last, 0, sizeof(st.cov_last));
          st.cov_last.why = 4;
        }
        st.cov_valid = true;
      }
    }
    if (tb->key_on && ok > 0) {
      // how much of each reference is still seen at the returned pose: one call for the group, on the batch that solved it
      std::vector<ea_pose_stats> stg(ng);
      TBRC(ea_batch_pose_stats(solver, qg.data(), tg.data(), tb->key_prm.margin, tb->key_prm.inlier_residual, stg.data()));
      for (size_t k = 0; k < ng; ++k)
        if (!s->stopped[(size_t)grp[k]]) s->kstats[(size_t)grp[k]] = stg[k];
    }
  }
  return EA_OK;
}

// References: on every level the frame's edge points become the reference of every stream -- in keyframe mode (a single level:
// ea_tracker_batch_set_keyframes) of the streams whose rule says so (keyframe_decide); a ROS stream whose frame has no edge
// keeps what it holds.  Laplacian, Canny: the counts queued beside the solve come back first (a wait).  Then the last wait.
namespace {
// the point arrays of the keyframes a push replaces, detached from their problems until the merge has read them; they go back
// to the cache with the push, however it ends
struct DetachedReferences {
  std::vector<int> streams;
  std::vector<MergeSource> src;
  ~DetachedReferences() {
    for (const MergeSource &m : src) {
      cached_free(const_cast<void *>(m.x)); cached_free(const_cast<void *>(m.y)); cached_free(const_cast<void *>(m.z));
    }
  }
  // moved, not copied: the problem is left without points and without arrays, as reserve_points(p, 0) leaves one
  void take(ea_problem *p, int stream) {
    streams.push_back(stream);
    src.push_back(MergeSource{p->d_x, p->d_y, p->d_z, p->n, p->weighted ? p->w_off : 0, p->weighted});
    p->d_x = p->d_y = p->d_z = nullptr;
    p->own_points = false;
    p->pts_cap = 0;
    p->n = 0;
    p->w_off = 0;
    p->weighted = p->weights_from_depth = false;
    p->version++;
  }
};
}  // namespace

static int tracker_push_references(TrackerPush *s) {
  ea_tracker_batch *tb = s->tb;
  DetachedReferences old;
  const size_t n = tb->st.size();
  s->take.assign(n, 1);
  s->why.assign(n, 0);
  bool any_take = true;
  if (tb->key_on) {
    const std::vector<unsigned char> &none = s->J[0].no_image;
    any_take = false;
    for (size_t i = 0; i < n; ++i) {
      const bool bare = !none.empty() && none[i];
      s->why[i] = bare ? 0 : keyframe_decide(s->kstats[i], tb->key_prm, tb->st[i].key.age + 1, s->is_al[i] != 0, s->stopped[i] != 0);
      s->take[i] = s->why[i] != 0;
      any_take = any_take || s->take[i];
    }
  }
  if (tb->carry_on && tb->key_on)
    for (size_t i = 0; i < n; ++i) {
      // a stream that replaces a keyframe it solved against keeps that keyframe's arrays for the merge below
      ea_problem *p = tb->lv[0].probs[i];
      if (s->take[i] && !(s->why[i] & (EA_KEY_FIRST | EA_KEY_SOLVE_FAILED)) && p->n > 0 && p->own_points && p->order.empty())
        old.take(p, (int)i);
    }
  for (BatchFrames &j : s->J) {
    if (!s->ros() && any_take) TBRC(batch_counts_fetch(&j));
    TBRC(batch_ref_room(&j, tb->key_on ? s->take.data() : nullptr));
    if (tb->gate_applies()) {
      // a gated stream is a weighted problem from its first reference on: the new reference's weights are dd, or exactly 1
      for (FrameSlot &sl : j.slots) sl.ones = 1;
      j.max_weighted = j.max_total;
    }
    if (!any_take) continue;
    if (s->ros()) {
      TBRC(batch_ros_scatter(&j));
    } else {
      TBCHK(upload_table(&j));
      TBRC(batch_ref_scatter(j, s->ref_edges(j), s->ref_threshold(), s->z_scaling));
    }
  }
  TBCHK(hipDeviceSynchronize());
  for (int l = 0; l < tb->levels; ++l)
    for (size_t i = 0; i < n; ++i)
      if (s->take[i]) {
        ea_problem *p = tb->lv[(size_t)l].probs[i];
        ref_points_landed(p, s->J[(size_t)l].slots[i].capacity);
        if (tb->gate_applies()) p->weighted = p->n > 0;  // (weights_from_depth: as landed -- they are dd alone, or ones)
      }
  if (!old.streams.empty()) {
    // the replaced keyframes' points into the new references, by the pose this push solved: ONE ea_batch_merge_points-equivalent
    // call over the streams that carry, before point selection
    const size_t m = old.streams.size();
    std::vector<double> T(16 * m);
    std::vector<ea_point_merge_stats> stats(m);
    for (size_t k = 0; k < m; ++k) {
      const size_t i = (size_t)old.streams[k];
      pose_to_matrix(&s->qs[4 * i], &s->ts[3 * i], &T[16 * k]);
    }
    TBRC(batch_merge_arrays(tb->lv[0].b, old.streams.data(), (int)m, old.src.data(), T.data(), &tb->carry_prm, stats.data()));
    for (size_t k = 0; k < m; ++k) tb->last_carry[(size_t)old.streams[k]] = stats[k];
    tb->last_carried = (int)m;
  }
  if (tb->sel_on && any_take) {
    // the new references are thinned where they landed: per level one ea_batch_select_points over the streams that took one
    std::vector<int> sel;
    for (size_t i = 0; i < n; ++i)
      if (s->take[i]) sel.push_back((int)i);
    std::vector<ea_point_selection_stats> stats(sel.size());
    for (int l = 0; l < tb->levels; ++l) {
      TBRC(ea_batch_select_points(tb->lv[(size_t)l].b, sel.data(), (int)sel.size(), &tb->sel_prm, stats.data()));
      for (size_t k = 0; k < sel.size(); ++k) tb->last_sel[(size_t)l * n + (size_t)sel[k]] = stats[k];
    }
    tb->last_selected = (int)sel.size();
  }
  return EA_OK;
}

// Bookkeeping: priors and frame counts advance only with the new references in place
static void tracker_push_book(const TrackerPush &s, double *q_rel, double *t_rel, int *aligned) {
  ea_tracker_batch *tb = s.tb;
  for (size_t i = 0; i < tb->st.size(); ++i) {
    TrackerStream &st = tb->st[i];
    if (s.is_al[i]) {
      std::memcpy(st.q, &s.qs[4 * i], sizeof(st.q));
      std::memcpy(st.t, &s.ts[3 * i], sizeof(st.t));
      if (aligned) aligned[i] = 1;
    }
    if (tb->key_on) {
      // the pose solved in this push against the keyframe in use during it (an unaligned stream: the identity); a stream that
      // took the frame starts its next solve at the identity, a kept one at the pose just stored
      const double q_id[4] = {1, 0, 0, 0}, t_id[3] = {0, 0, 0};
      std::memcpy(q_rel + 4 * i, s.is_al[i] ? st.q : q_id, sizeof(st.q));
      std::memcpy(t_rel + 3 * i, s.is_al[i] ? st.t : t_id, sizeof(st.t));
      st.key.replaced = s.why[i];
      st.key.stats = s.kstats[i];
      if (s.take[i]) {
        std::memcpy(st.q, q_id, sizeof(st.q));
        std::memcpy(st.t, t_id, sizeof(st.t));
        st.key.age = 0;
        st.key.keyframe_push = tb->pushes;
        tb->last_taken++;
      } else if (s.is_al[i]) {
        st.key.age += 1;
      }
    } else {
      std::memcpy(q_rel + 4 * i, st.q, sizeof(st.q));
      std::memcpy(t_rel + 3 * i, st.t, sizeof(st.t));
    }
    st.frames += 1;
  }
  tb->last_aligned = (int)s.al.size();
}

// The push of every flavour and level count: the phases above, in order.  q_rel, t_rel, summaries, aligned: as ea_hip.h says.
static int tracker_batch_push(ea_tracker_batch *tb, const uint8_t *const *bgr, const void *const *depth, int height, int width,
                              double z_scaling, const ea_options *opt, double *q_rel, double *t_rel, ea_summary *summaries,
                              int *aligned, bool on_device) {
  if (!tb || !bgr || !depth || !q_rel || !t_rel) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  TrackerPush s;
  s.tb = tb; s.bgr = bgr; s.depth = depth; s.z_scaling = z_scaling; s.opt = opt; s.summaries = summaries; s.on_device = on_device;
  int rc = tracker_push_check(&s, height, width);
  if (rc != EA_OK) return rc;
  const size_t n = tb->st.size();
  tb->pushes++;
  tb->last_aligned = tb->last_bare = tb->last_rounds = tb->last_edge_passes = tb->last_taken = 0;
  for (size_t i = 0; i < n; ++i) tb->st[i].cov_valid = false;
  if (aligned) std::fill(aligned, aligned + n, 0);
  if (summaries) std::memset(summaries, 0, n * sizeof(*summaries));
  std::memset(tb->last_sums.data(), 0, tb->last_sums.size() * sizeof(ea_summary));
  std::fill(tb->last_gate.begin(), tb->last_gate.end(), ea_depth_gate_stats{});
  tb->last_gated = 0;
  tb->last_selected = 0;
  std::fill(tb->last_carry.begin(), tb->last_carry.end(), ea_point_merge_stats{});
  tb->last_carried = 0;
  // (a phase that fails has dropped every stream: tracker_batch_fail)
  for (int (*phase)(TrackerPush *) : {tracker_push_frames, tracker_push_images, tracker_push_priors, tracker_push_descent,
                                      tracker_push_covariance, tracker_push_references})
    if ((rc = phase(&s)) != EA_OK) return rc;
  tracker_push_book(s, q_rel, t_rel, aligned);
  return EA_OK;
}

extern "C" int ea_tracker_batch_push_frames(ea_tracker_batch *tb, const uint8_t *const *bgr, const void *const *depth, int height,
                                            int width, double z_scaling, const ea_options *opt, double *q_rel, double *t_rel,
                                            ea_summary *summaries, int *aligned) {
  return tracker_batch_push(tb, bgr, depth, height, width, z_scaling, opt, q_rel, t_rel, summaries, aligned, false);
}

extern "C" int ea_tracker_batch_push_frames_device(ea_tracker_batch *tb, const uint8_t *const *bgr, const void *const *depth,
                                                   int height, int width, double z_scaling, const ea_options *opt, double *q_rel,
                                                   double *t_rel, ea_summary *summaries, int *aligned) {
  return tracker_batch_push(tb, bgr, depth, height, width, z_scaling, opt, q_rel, t_rel, summaries, aligned, true);
}

extern "C" int ea_tracker_batch_reset(ea_tracker_batch *tb, int i) {
  if (!tb) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (i >= (int)tb->st.size()) return fail(EA_ERR_INVALID_ARG, "no such stream");
  HIPCHK(hipSetDevice(tb->device));
  for (size_t s = 0; s < tb->st.size(); ++s) {
    if (i >= 0 && s != (size_t)i) continue;
    tracker_stream_drop(tb, s);  // (its keyframe state too)
    const double q[4] = {1, 0, 0, 0};
    std::memcpy(tb->st[s].q, q, sizeof(q));
    std::memset(tb->st[s].t, 0, sizeof(tb->st[s].t));
  }
  return EA_OK;
}

extern "C" int ea_tracker_batch_set_covariance(ea_tracker_batch *tb, const ea_covariance_options *o) {
  if (!tb) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (o) {
    const int rc = check_cov_options(o);
    if (rc != EA_OK) return rc;
    tb->cov_opt = *o;
  }
  tb->cov_on = o != nullptr;
  for (TrackerStream &s : tb->st) s.cov_valid = false;
  return EA_OK;
}

extern "C" int ea_tracker_batch_last_covariance(ea_tracker_batch *tb, int i, ea_covariance *out) {
  if (!tb || !out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (i < 0 || (size_t)i >= tb->st.size()) return fail(EA_ERR_INVALID_ARG, "no such stream");
  if (!tb->cov_on) return fail(EA_ERR_STATE, "covariance is off (ea_tracker_batch_set_covariance)");
  if (!tb->st[(size_t)i].cov_valid) return fail(EA_ERR_STATE, "the last push did not align this stream");
  *out = tb->st[(size_t)i].cov_last;
  return EA_OK;
}

extern "C" int ea_tracker_batch_set_motion_prior(ea_tracker_batch *tb, double sigma_rot, double sigma_trans) {
  if (!tb) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!sigmas_ok(sigma_rot, sigma_trans)) return fail(EA_ERR_INVALID_ARG, "sigmas must be finite and >= 0");
  if (sigma_rot == 0.0 && sigma_trans == 0.0)
    for (size_t i = 0; i < tb->st.size(); ++i)
      if (tb->st[i].motion_set) {
        for (const ea_tracker_batch::Level &lv : tb->lv) motion_prior_clear(lv.probs[i], tb->st[i].installed);
        tb->st[i].motion_set = false;
      }
  tb->sigma_rot = sigma_rot;
  tb->sigma_trans = sigma_trans;
  return EA_OK;
}

extern "C" void ea_default_keyframe_params(ea_keyframe_params *p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->min_visible_fraction = 0.75;  // (an untuned starting value)
}

extern "C" int ea_tracker_batch_set_keyframes(ea_tracker_batch *tb, const ea_keyframe_params *p) {
  if (!tb) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (p && !keyframe_params_ok(*p))
    return fail(EA_ERR_INVALID_ARG, "keyframe parameters: no NaN field, margin >= 0, inlier_residual >= 0");
  if (p && tb->levels > 1) return fail(EA_ERR_STATE, "keyframe mode is not available with pyramid levels (levels > 1)");
  for (const TrackerStream &s : tb->st)
    if (s.frames > 0)
      return fail(EA_ERR_STATE, "a stream holds a reference: set the mode before the first push or after ea_tracker_batch_reset(-1)");
  tb->key_on = p != nullptr;
  if (p) tb->key_prm = *p;
  for (TrackerStream &s : tb->st) s.key = ea_keyframe_state{};
  return EA_OK;
}

extern "C" int ea_tracker_batch_set_depth_gate(ea_tracker_batch *tb, const ea_depth_gate_params *prm) {
  if (prm)
    if (const char *why = depth_gate_params_error(prm)) return fail(EA_ERR_INVALID_ARG, why);
  if (!tb) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (prm && !depth_gate_factors_fit(prm, tb->lv[0].probs[0]->dtype == EA_F32 ? (double)FLT_MAX : DBL_MAX))
    return fail(EA_ERR_INVALID_ARG, "a weight factor overflows the float of an fp32 tracker");
  for (const TrackerStream &s : tb->st)
    if (s.frames > 0)
      return fail(EA_ERR_STATE, "a stream holds a reference: set the gate before the first push or after ea_tracker_batch_reset(-1)");
  tb->gate_on = prm != nullptr;
  if (prm) tb->gate_prm = *prm;
  std::fill(tb->last_gate.begin(), tb->last_gate.end(), ea_depth_gate_stats{});
  tb->last_gated = 0;
  return EA_OK;
}

extern "C" int ea_tracker_batch_last_depth_gate(ea_tracker_batch *tb, int level, int i, ea_depth_gate_stats *out) {
  if (!tb || !out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (level < 0) return fail(EA_ERR_INVALID_ARG, "no such level");  // (a negative index: before the handle is looked at)
  if (i < 0) return fail(EA_ERR_INVALID_ARG, "no such stream");
  if (level >= tb->levels) return fail(EA_ERR_INVALID_ARG, "no such level");
  if ((size_t)i >= tb->st.size()) return fail(EA_ERR_INVALID_ARG, "no such stream");
  *out = tb->last_gate[(size_t)level * tb->st.size() + (size_t)i];
  return EA_OK;
}

extern "C" int ea_tracker_batch_set_point_selection(ea_tracker_batch *tb, const ea_point_selection *prm) {
  if (prm) {
    if (const char *why = point_selection_error(prm)) return fail(EA_ERR_INVALID_ARG, why);
    if (prm->height != 0 || prm->width != 0)
      return fail(EA_ERR_INVALID_ARG, "height and width must be 0: every level uses the extent of its own DT image");
  }
  if (!tb) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  tb->sel_on = prm != nullptr;
  if (prm) tb->sel_prm = *prm;
  return EA_OK;
}

extern "C" int ea_tracker_batch_last_point_selection(const ea_tracker_batch *tb, ea_point_selection_stats *stats, int capacity) {
  if (!tb || !stats) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (capacity < 0 || (size_t)capacity < tb->last_sel.size()) return fail(EA_ERR_INVALID_ARG, "capacity is smaller than levels x streams");
  std::copy(tb->last_sel.begin(), tb->last_sel.end(), stats);
  return EA_OK;
}

extern "C" int ea_tracker_batch_set_point_carry(ea_tracker_batch *tb, const ea_point_merge *prm) {
  if (prm) {
    if (const char *why = point_merge_error(prm)) return fail(EA_ERR_INVALID_ARG, why);
    if (prm->height != 0 || prm->width != 0)
      return fail(EA_ERR_INVALID_ARG, "height and width must be 0: a stream uses the extent of its own DT image");
  }
  if (!tb) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (prm && !tb->key_on) return fail(EA_ERR_STATE, "keyframe mode is off (ea_tracker_batch_set_keyframes)");
  for (const TrackerStream &s : tb->st)
    if (s.frames > 0)
      return fail(EA_ERR_STATE, "a stream holds a reference: set the carry before the first push or after ea_tracker_batch_reset(-1)");
  tb->carry_on = prm != nullptr;
  if (prm) tb->carry_prm = *prm;
  return EA_OK;
}

extern "C" int ea_tracker_batch_last_point_carry(const ea_tracker_batch *tb, ea_point_merge_stats *stats, int capacity) {
  if (!tb || !stats) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (capacity < 0 || (size_t)capacity < tb->last_carry.size()) return fail(EA_ERR_INVALID_ARG, "capacity is smaller than the number of streams");
  std::copy(tb->last_carry.begin(), tb->last_carry.end(), stats);
  return EA_OK;
}

extern "C" int ea_tracker_batch_keyframe_state(ea_tracker_batch *tb, int i, ea_keyframe_state *out) {
  if (!tb || !out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (i < 0 || (size_t)i >= tb->st.size()) return fail(EA_ERR_INVALID_ARG, "no such stream");
  if (!tb->key_on) return fail(EA_ERR_STATE, "keyframe mode is off (ea_tracker_batch_set_keyframes)");
  *out = tb->st[(size_t)i].key;
  return EA_OK;
}

extern "C" int ea_tracker_batch_get_info(const ea_tracker_batch *tb, const char *key, int64_t *value) {
  if (!tb || !key || !value) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  const std::string k = key;
  if (k == "aligned") *value = tb->last_aligned;
  else if (k == "frames_without_edges") *value = tb->last_bare;
  else if (k == "hysteresis_rounds") *value = tb->last_rounds;
  else if (k == "edge_passes") *value = tb->last_edge_passes;
  else if (k == "frames") *value = tb->pushes;
  else if (k == "levels") *value = tb->levels;
  else if (k == "keyframes_taken") *value = tb->last_taken;
  else if (k == "keyframe_mode") *value = tb->key_on ? 1 : 0;
  else if (k == "depth_gate") *value = tb->gate_on ? 1 : 0;
  else if (k == "gated") *value = tb->last_gated;
  else if (k == "point_selection") *value = tb->sel_on ? 1 : 0;
  else if (k == "selected") *value = tb->last_selected;
  else if (k == "point_carry") *value = tb->carry_on ? 1 : 0;
  else if (k == "carried") *value = tb->last_carried;
  else return fail(EA_ERR_INVALID_ARG, "unknown info key: " + k);
  return EA_OK;
}

// read back what the problem holds in HBM: points as n x 3 doubles, DT as H x W doubles ([v][u])
extern "C" int ea_problem_get_points(ea_problem *p, double *xyz, int64_t capacity) {
  if (!p || (!xyz && p->n > 0)) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (capacity < p->n) return fail(EA_ERR_INVALID_ARG, "capacity smaller than the number of points");
  if (p->n == 0) return EA_OK;
  HIPCHK(hipSetDevice(p->device));
  const size_t n = (size_t)p->n, esz = p->dtype == EA_F32 ? 4 : 8;
  std::vector<unsigned char> buf(3 * n * esz);
  HIPCHK(hipMemcpy(buf.data(), p->d_x, n * esz, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(buf.data() + n * esz, p->d_y, n * esz, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(buf.data() + 2 * n * esz, p->d_z, n * esz, hipMemcpyDeviceToHost));
  const int32_t *ord = p->order.empty() ? nullptr : p->order.data();
  for (int c = 0; c < 3; ++c)
    for (size_t i = 0; i < n; ++i)
      xyz[3 * (ord ? (size_t)ord[i] : i) + c] = p->dtype == EA_F32 ? (double)reinterpret_cast<float *>(buf.data())[c * n + i]
                                                                  : reinterpret_cast<double *>(buf.data())[c * n + i];
  return EA_OK;
}

extern "C" int ea_problem_get_dt(ea_problem *p, double *image, int *height, int *width) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (height) *height = p->H;
  if (width) *width = p->W;
  if (!image) return EA_OK;
  if (!p->d_dt) return fail(EA_ERR_STATE, "distance-transform image not set");
  HIPCHK(hipSetDevice(p->device));
  const size_t esz = p->dtype == EA_F32 ? 4 : 8;
  const size_t rows = (size_t)p->H + 2 * kImagePad;
  std::vector<unsigned char> buf((size_t)p->pitch * rows * esz);
  HIPCHK(hipMemcpy(buf.data(), p->d_dt, buf.size(), hipMemcpyDeviceToHost));
  for (int v = 0; v < p->H; ++v)
    for (int u = 0; u < p->W; ++u) {
      const size_t idx = (size_t)(v + kImagePad) * p->pitch + (u + kImagePad);
      image[(size_t)v * p->W + u] = p->dtype == EA_F32 ? (double)reinterpret_cast<float *>(buf.data())[idx]
                                                       : reinterpret_cast<double *>(buf.data())[idx];
    }
  return EA_OK;
}
