// ea_capi_internal.h — what the library's three host translation units share behind include/ea_hip.h: ea_capi.hip (problems,
// batches, solves; it defines everything declared here but auto_scale_losses), ea_frames.hip (frame producers, tracker) and
// ea_segments.hip (the calls that run one segment per problem: quantiles, pose statistics, reproject, overlay, depth gate,
// point selection, point transform and merge).
// Not for ea_comm.hip, which sees problems and batches through the C-ABI and ea_launch.h only.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/ea_hip.h"
#include "ea_prior.h"
#include "ea_types.h"

struct ea_problem {
  int device = 0;
  int dtype = EA_F64;
  ea_camera cam{};
  int loss_kind = EA_LOSS_CAUCHY;  // the reference's `new CauchyLoss(1.)`
  double loss_a = 1.0;
  double z_guard = 0.01, z_eps = 0.0;
  int rot_transposed = 0;
  // residual variants (utils.h:102-421)
  int variant = 0;                       // bit 0 distortion, bit 1 second camera
  double dist[5] = {0, 0, 0, 0, 0};      // k1, k2, p1, p2, k3
  double T12[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  double T12inv[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  std::vector<ea_problem *> terms;       // further residual families sharing this problem's pose
  ea::PriorDesc prior = {};                  // NormalPriors on q / t (ea_problem_set_normal_prior; ea_prior.h)
  int term_of = 0;                       // how many problems hold this one as a term (a term carries no prior)
  int held = 0;                          // tangent coordinates held constant, bit i of [delta | t] (ea_problem_set_constant_parameters)
  // ea_problem_set_loss_auto_scale: factor > 0 = every ea_batch_solve first sets loss_a = max(a_min, factor * Q_prob(|r|)) at
  // the start pose; like `held` it is a setting of the problem, not of its points or image, and no producer touches it
  double auto_factor = 0.0, auto_prob = 0.5, auto_a_min = 1e-6;
  int64_t n = 0;
  void *d_x = nullptr, *d_y = nullptr, *d_z = nullptr;
  bool own_points = false;
  // storage order of the points in HBM (ea_problem_set_point_order): order[i] = caller's index of stored point i;
  // empty = the caller's order
  int order_tile = -1, order_tile_used = 0;
  std::vector<int32_t> order;
  void *d_dt = nullptr;
  size_t dt_cap = 0;   // bytes allocated behind d_dt: a frame of the same size reuses the allocation
  // fp64 problems: the float32 mirror of the image (same padded layout and pitch in texels) and whether it holds every
  // value exactly -- then the plain fp64 kernels read it instead (ProblemDesc::dt32): one 16-byte load per stencil row
  float *d_dt32 = nullptr;
  size_t dt32_cap = 0;
  bool dt32_exact = false;
  size_t pts_cap = 0;  // bytes allocated behind each of d_x, d_y, d_z when own_points (hipFree / hipMalloc per frame
                       // cost more than the whole pre-processing of a 640x480 frame)
  // Per-point weights (ceres::ScaledLoss per residual block; ea_problem_set_weights*, or written by the reference-frame
  // producers under ea_problem_set_depth_weighting).  They belong to the point set: stored in the points' order and dtype
  // BEHIND z in z's own allocation, w_off elements from d_z (ProblemDesc::w_off: the descriptor has four spare bytes, not
  // eight), which is why only points the problem owns can carry weights -- borrowed arrays are copied first.  `weighted`
  // makes the term a variant (bit 2) in every batch that holds it.
  bool weighted = false, weights_from_depth = false;
  int64_t w_off = 0;
  double dw_z_ref = 1.0;  // ea_problem_set_depth_weighting: w = min(1, (z_ref / z)^power), power 0 = off
  int dw_power = 0;
  int W = 0, H = 0, pitch = 0;
  // The current frame's depth (ea_problem_set_now_depth*): nd_H x nd_W samples of their own kind (EA_DEPTH_U16 / EA_DEPTH_F32),
  // copied as they came into a cached block.  Read by the depth gate only: no descriptor names it, so setting or dropping it
  // moves no version, and no other setter or producer touches it.
  void *d_now_depth = nullptr;
  size_t now_depth_cap = 0;
  int nd_kind = 0, nd_H = 0, nd_W = 0;
  double nd_z_scaling = 1.0;
  uint64_t version = 1;  // bumped by every setter; batches rebuild their descriptors lazily
  ea_batch *self = nullptr;
  hipStream_t stream = nullptr;
  // scratch for the frame pre-processing kernels (grown on demand, reused across frames)
  unsigned char *ws = nullptr;
  size_t ws_bytes = 0;
  // full-resolution frames on their way to a half-resolution level (ea_problem_set_*_frame_ros_scaled)
  unsigned char *stage = nullptr;
  size_t stage_bytes = 0;
  // what the last producer call left in the workspace: 1 = set_now_frame (Laplacian strength), 2 = set_now_frame_canny
  // (edge map, no mask), 0 = nothing reusable; with the frame's extent.  The tracker extracts the same frame's edge
  // points from it instead of uploading and filtering the frame a second time.
  int ws_now_kind = 0, ws_now_h = 0, ws_now_w = 0;
};

namespace ea {

// the thread-local message behind ea_last_error(); returns `code`
int fail(int code, const std::string &msg);

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      return fail(e_ == hipErrorNoDevice ? EA_ERR_NO_DEVICE : EA_ERR_HIP,                     \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                        \
  } while (0)

int check_device(int device);

// the resource cache: freed device blocks are kept and handed out again (ea_capi.hip has the rules)
hipError_t cached_malloc(void **out, size_t bytes, int device);
void cached_free(void *p);
// likewise pinned host blocks (hipHostMalloc flags) and non-blocking streams (the caller has synchronised what it hands back)
hipError_t cached_host_malloc(void **out, size_t bytes, unsigned flags, int device);
void cached_host_free(void *p);
hipError_t cached_stream_create(hipStream_t *out, int device);
void cached_stream_destroy(hipStream_t s, int device);
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }
// scope guard for a temporary device block, so that an early HIPCHK return frees it
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) cached_free(p); }  // (blocks that did not come from the cache fall through to hipFree)
  template <typename U> U *as() const { return static_cast<U *>(p); }
};

// room for n points in arrays the problem owns; leaves the problem without points (n = 0)
int reserve_points(ea_problem *p, int64_t n);
inline void *weights_ptr(const ea_problem *p) {
  return static_cast<unsigned char *>(p->d_z) + (size_t)p->w_off * (p->dtype == EA_F32 ? 4 : 8);
}
// bits of ProblemDesc::variant a problem sets as a term
inline int term_variant(const ea_problem *p) { return p->variant | (p->weighted ? 4 : 0); }
// the problem's padded W x H image (and its float32 mirror for fp64 problems), reusing an allocation that fits
int alloc_dt(ea_problem *p, int W, int H);
int check_cov_options(const ea_covariance_options *o);
// the solve options' validity (every solve checks them itself; the multi-stream tracker checks before it touches a stream)
int check_options(const ea_options &o);

// What the other two files see of a batch, whose layout stays ea_capi.hip's: a read-only view.  batch_view: the batch as it
// stands -- its problems in batch order, device, dtype, stream -- with the rest left empty.  batch_built: descriptors rebuilt
// where a problem changed (EA_ERR_STATE without a DT image, as ea_eval) and the calling thread on the batch's device, then the
// whole view: the host copies of that build's descriptor and group tables, the device's descriptors, the rows of the batch's
// layout (ea_batch_row_offsets).
struct BatchView {
  int device = 0, dtype = EA_F64, count = 0, nterms = 0;
  hipStream_t stream = nullptr;
  ea_problem *const *probs = nullptr;                        // count
  const ProblemDesc *h_desc = nullptr, *d_probs = nullptr;   // nterms, on the host and on the device
  const GroupDesc *h_groups = nullptr;                       // count
  int64_t total_rows = 0;
};
BatchView batch_view(ea_batch *b);
int batch_built(ea_batch *b, BatchView *v);

// The batch-owned memory of the batched producers (ea_frames.hip) -- one device block and one pinned staging block of at least
// the sizes asked for, grown on demand, kept across calls and freed with the batch (EA_ERR_ALLOC when either cannot be had;
// what they hold is the producers' business).
int batch_frames_reserve(ea_batch *b, size_t device_bytes, size_t pinned_bytes, unsigned char **device_block,
                         unsigned char **pinned_block);
// ea_batch_get_info's "frames_hysteresis_rounds": looks at the hysteresis flags the batch's last producer call has taken so far
void batch_frames_set_rounds(ea_batch *b, int rounds);
// ea_batch_get_info's "frames_without_edges": current frames of the last ea_batch_set_frames_ros call that had no edge (every
// batched producer call starts by setting it to 0)
void batch_frames_set_without_edges(ea_batch *b, int frames);
// ea_batch_get_info's "frames_uploaded": host-to-device frame copies of the last ea_batch_set_frames_ros_pyramid call, kept by
// the batch of level 0
void batch_frames_set_uploaded(ea_batch *b, int64_t copies);

// What else the per-problem segment calls (ea_segments.hip) need.  batch_upload_poses: one pose per problem into the batch's
// d_poses, on its stream.  batch_gate_reserve: the depth gate's block pair, batch-owned like the producers' (ea_batch says why).
// problem_call_batch: the prologue of a single-problem call -- the problem's batch of one, built (build = false: left to the
// caller, whose own checks come first), EA_ERR_STATE for a problem without points.
int batch_upload_poses(ea_batch *b, const double *q, const double *t, const PoseState **d_poses = nullptr);
int batch_gate_reserve(ea_batch *b, size_t bytes, unsigned char **device_block, unsigned char **pinned_block);
int problem_call_batch(ea_problem *p, ea_batch **b, bool build = true);
// the problem's batch of one as it stands, not built: for point selection, to which a problem without points is a result
int problem_self_batch(ea_problem *p, ea_batch **b);
// no problem or batch exists without a device; this answers the "no device" question before a handle is dereferenced
int require_device();
// borrowed point arrays (ea_problem_set_points_device) into arrays the problem owns
int own_borrowed_points(ea_problem *p);
// points of the problem and its terms: its rows in a batch's layout
int64_t problem_points(const ea_problem *p);
// a caller's device pointer: non-NULL, 16-byte aligned, and -- where this runtime knows the allocation -- memory of `device`
int check_device_pointer(int device, const void *ptr, const char *what);
// rows stored in tile order (ea_problem_set_point_order) back in the caller's order: out[order[i]] = tmp[i], elem_bytes each
void scatter_to_callers_order(const std::vector<int32_t> &order, size_t elem_bytes, const void *tmp, void *out);
// ea_segments.hip's, for the multi-stream tracker (ea_frames.hip): the depth gate of ea_batch_depth_gate on depth images the
// caller names, one per problem of the batch in batch order, all of one kind (EA_DEPTH_*), z_scaling and shift (ea_depth_gate.h:
// the image is 2^shift times the problem's DT extent); complete on the device when the call is made
struct GateImages {
  int kind = 0, shift = 0;
  double z_scaling = 1.0;
  const void *const *depth = nullptr;
};
int batch_depth_gate_images(ea_batch *b, const double *b_T_a, const ea_depth_gate_params *prm, const GateImages &img,
                            ea_depth_gate_stats *stats);
// ea_segments.hip's, for the multi-stream tracker: ea_batch_merge_points with the carried points named as device arrays (the
// detached arrays of a replaced keyframe) instead of problems; src[j] belongs to problem sel[j].  The parameters have been
// checked (point_merge_error), the arrays are of the batch's dtype and device and in the caller's order
struct MergeSource {
  const void *x = nullptr, *y = nullptr, *z = nullptr;
  int64_t n = 0, w_off = 0;  // the weights: w_off elements behind z
  bool weighted = false;
};
int batch_merge_arrays(ea_batch *b, const int *sel, int nsel, const MergeSource *src, const double *dst_T_src,
                       const ea_point_merge *prm, ea_point_merge_stats *stats);
// ea_segments.hip's, for ea_batch_solve: the losses of ea_problem_set_loss_auto_scale set from the residuals at poses q, t
int auto_scale_losses(ea_batch *b, const double *q, const double *t);

}  // namespace ea
