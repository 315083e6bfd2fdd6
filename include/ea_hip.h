/*
 * ea_hip.h — C-ABI of the MI355X-native edge-alignment hot path (libea_hip.so).
 *
 * This is the drop-in boundary for ONE path of kuwt/edge_alignment: the per-edge-point
 * EAResidue evaluation (SE(3) warp -> pinhole -> bicubic DT sample -> 1x6 Jacobian), the
 * JtJ / Jtr / cost reduction, and the trust-region loop the reference hands to ceres::Solve.
 * The reference has no FFI layer (it is a C++ source-level API on top of Ceres); each entry
 * point below names the reference code it replaces (paths relative to the reference root).
 * Host C++ shims that keep the reference's own spellings (EAResidue, SolveEA, a minimal
 * ceres:: facade) sit on top of this header in edge_alignment_amd/include/.
 *
 * Conventions
 *   - plain C types only; every function returns an ea_status (0 = ok, < 0 = error) and
 *     never throws.  ea_last_error() gives a thread-local message for the last failure.
 *   - poses are q = (w,x,y,z), t = (tx,ty,tz), b_T_a (maps frame-A points into frame B),
 *     exactly the raw arrays of PoseManipUtils::eigenmat_to_raw
 *     (standalone/PoseManipUtils.cpp:16-27); ea_solve updates them in place like ceres::Solve.
 *   - host buffers handed to ea_problem_set_* are copied to HBM before the call returns and
 *     may be freed afterwards (the reference's Grid2D merely borrows, utils.h:95).
 *   - a handle is not thread-safe; use one handle per host thread / per GPU.
 *   - there is NO CPU fallback: every compute entry point fails with EA_ERR_NO_DEVICE when
 *     no gfx950 device is usable.
 */
#ifndef EA_HIP_H
#define EA_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  EA_OK = 0,
  EA_ERR_INVALID_ARG = -1,
  EA_ERR_HIP = -2,
  EA_ERR_NO_DEVICE = -3,
  EA_ERR_STATE = -4,
  EA_ERR_ALLOC = -5
} ea_status;

/* arithmetic type of the per-point evaluation (reductions are always fp64) */
typedef enum { EA_F64 = 0, EA_F32 = 1 } ea_dtype;

/* ceres::TrivialLoss / CauchyLoss(a) / HuberLoss(a)
 * (standalone_edge_align.cpp:272, :2604; src/SolveEA.cpp:144) */
typedef enum { EA_LOSS_TRIVIAL = 0, EA_LOSS_CAUCHY = 1, EA_LOSS_HUBER = 2 } ea_loss_kind;

/* ceres::TerminationType as far as this path can produce it */
typedef enum { EA_CONVERGENCE = 0, EA_NO_CONVERGENCE = 1, EA_FAILURE = 2 } ea_termination;

typedef enum {
  EA_WHY_NONE = 0,
  EA_WHY_FUNCTION_TOL = 1,
  EA_WHY_GRADIENT_TOL = 2,
  EA_WHY_PARAMETER_TOL = 3,
  EA_WHY_MAX_ITERATIONS = 4,
  EA_WHY_MIN_RADIUS = 5,
  EA_WHY_INITIAL_EVAL_FAILED = 6,     /* a functor returned false at the start (utils.h:70-73) */
  EA_WHY_TOO_MANY_INVALID_STEPS = 7,
  EA_WHY_EVAL_FAILED = 8
} ea_why;

typedef enum { EA_STRATEGY_LM = 0, EA_STRATEGY_DOGLEG = 1 } ea_strategy;

/* pinhole intrinsics, the four doubles every EAResidue carries (utils.h:41-44,96) */
typedef struct {
  double fx, fy, cx, cy;
} ea_camera;

/* the fields of ceres::Solver::Options the reference touches or relies on by default
 * (standalone_edge_align.cpp:282-284, :2112-2116; src/SolveEA.cpp:184-192) */
typedef struct {
  int max_num_iterations;             /* 50 */
  double function_tolerance;          /* 1e-6 */
  double gradient_tolerance;          /* 1e-10 */
  double parameter_tolerance;         /* 1e-8 */
  double initial_trust_region_radius; /* 1e4 */
  double max_trust_region_radius;     /* 1e16 */
  double min_trust_region_radius;     /* 1e-32 */
  double min_relative_decrease;       /* 1e-3 */
  double min_lm_diagonal;             /* 1e-6 */
  double max_lm_diagonal;             /* 1e32 */
  int max_num_consecutive_invalid_steps; /* 5 */
  int jacobi_scaling;                 /* 1 */
  int strategy;                       /* EA_STRATEGY_LM (LEVENBERG_MARQUARDT) | EA_STRATEGY_DOGLEG */
  int minimizer_progress_to_stdout;   /* 0 */
  int iterations_per_sync;            /* device LM iterations enqueued between host checks; 0 = default */
  double solve_timeout_ms;            /* a solve whose device side shows no progress for this long returns EA_ERR_HIP
                                         instead of spinning for ever; 0 = default (5000 ms), < 0 = no deadline */
} ea_options;

#define EA_MAX_TRACE 128

/* what the drivers read back from ceres::Solver::Summary (FullReport(), :293) */
typedef struct {
  int termination;  /* ea_termination */
  int why;          /* ea_why */
  int num_iterations;          /* successful + unsuccessful steps (+1 if the last one ended the solve) */
  int num_successful_steps;
  int num_unsuccessful_steps;
  double initial_cost, final_cost;
  int64_t num_point_evals;     /* edge-point residual+Jacobian evaluations performed */
  double total_time_ms;        /* host wall time of the call */
  /* per-iteration trace, entries [0 .. min(num_iterations, EA_MAX_TRACE-1)] */
  double it_cost[EA_MAX_TRACE];
  double it_cost_change[EA_MAX_TRACE];
  double it_gradient_max_norm[EA_MAX_TRACE];
  double it_step_norm[EA_MAX_TRACE];
  double it_relative_decrease[EA_MAX_TRACE];
  double it_radius[EA_MAX_TRACE];
  int it_successful[EA_MAX_TRACE];
} ea_summary;

typedef struct ea_problem ea_problem; /* one frame pair: edge points of A + DT image of B */
typedef struct ea_batch ea_batch;     /* several problems evaluated / solved by the same launches */

/* ---- library ------------------------------------------------------------------------- */
const char *ea_last_error(void);
/* Device blocks, pinned host blocks and streams freed by ea_problem_destroy / ea_batch_destroy (and by re-sizing calls) are
 * kept by the library and handed out again (bounded: 1 GiB of device memory, 256 MiB pinned): creating and destroying an
 * ea_problem per solve -- what the ceres facade does per ceres::Solve -- then costs no driver allocation.  This returns
 * everything that is cached to the driver. */
int ea_release_cached_memory(void);
/* Page-locked host memory for the caller's frames (the buffers handed to ea_problem_set_*_frame*, ea_tracker_push_frame,
 * ea_problem_set_points / _set_dt): the uploads of those calls then run as direct DMA instead of being staged through the
 * runtime's bounce buffers -- ea_tracker_push_frame 0.31 -> 0.28 ms per VGA frame (profiles/r03_tracker_pinned.txt).
 * Plain memory to the host (cv::Mat can wrap it); NULL on failure (ea_last_error).  Free with ea_host_free only. */
void *ea_host_alloc(size_t bytes, int device);
void ea_host_free(void *p);
const char *ea_version(void);
int ea_device_count(int *count);            /* number of gfx950 devices visible */
void ea_default_options(ea_options *opt);   /* ceres::Solver::Options() defaults used by test1 */

/* ---- problem = ceres::Problem filled by the loop at standalone_edge_align.cpp:264-278 --- */
int ea_problem_create(ea_problem **out, const ea_camera *cam, int dtype, int device);
void ea_problem_destroy(ea_problem *p);

/* Edge points, replacing the N `EAResidue::Create(fx,fy,cx,cy, X,Y,Z, interp)` +
 * `AddResidualBlock` calls (standalone_edge_align.cpp:267-274; src/SolveEA.cpp:163-175).
 * xyz: host, point i at xyz[i*stride_elems + {0,1,2}] — stride 4 for the 4xN column-major
 * a_X of get_aX (utils.cpp:268-280) or 3 for list_edge_ref (SolveEA.cpp:55).  Converted once
 * to SoA x[],y[],z[] of the problem dtype in HBM. */
int ea_problem_set_points(ea_problem *p, const double *xyz, int64_t n, int64_t stride_elems);
/* Storage order of the points ea_problem_set_points uploads after this call.  tile_px > 0: tiles of
 * tile_px x tile_px pixels of the reference frame (identity-pose projection), tiles in raster order,
 * the caller's order inside a tile -- a wavefront's points then sample a compact patch of the DT image;
 * 0: the caller's order (the reference's: residual blocks in the order of the a_X columns);
 * < 0 (default): automatic, tiles of 16 px from 200 000 points up.  Only the order of summation
 * changes (results agree to rounding); per-point outputs (ea_eval_points) and ea_problem_get_points
 * stay in the caller's order. */
int ea_problem_set_point_order(ea_problem *p, int tile_px);
/* the tile size the stored points are ordered by (0 = the caller's order) */
int ea_problem_get_point_order(const ea_problem *p, int *tile_px);
/* same, from SoA arrays of the problem's dtype already resident in HBM (borrowed, must
 * outlive the problem) */
int ea_problem_set_points_device(ea_problem *p, const void *x, const void *y, const void *z,
                                 int64_t n);

/* Distance-transform image, replacing
 *   ceres::Grid2D<double,1> grid(data, 0, grid_rows, 0, grid_cols);
 *   ceres::BiCubicInterpolator<...> interp(grid);        (standalone_edge_align.cpp:258-259)
 * data: host, row-major, value(r,c) = data[r*grid_cols + c]; the functor samples it at
 * (r = u, c = v) (utils.h:77), so grid_rows is the u extent (image width) and grid_cols the
 * v extent (image height) exactly as the reference passes e_disTrans.cols()/rows(). */
int ea_problem_set_dt(ea_problem *p, const double *data, int grid_rows, int grid_cols);
/* same, from an image already in HBM: row-major [height][width] (u contiguous) of the problem's
 * dtype; copied into the library's padded layout by a device kernel */
int ea_problem_set_dt_image_device(ea_problem *p, const void *image, int height, int width);

/* loss_function argument of AddResidualBlock (:272 `new CauchyLoss(1.)`) */
int ea_problem_set_loss(ea_problem *p, int loss_kind, double a);
/* the loss the problem holds now (either output may be NULL); after a solve of an auto-scaled problem: the scale it used */
int ea_problem_get_loss(const ea_problem *p, int *kind, double *a);
/* Loss scale from the data.  The reference hard-codes CauchyLoss(1.) while its producers emit distance transforms in [0, 1],
 * in [0, 255] or not normalised at all, so the same a means three different things; the usual remedy is a robust statistic of
 * the residuals at the start pose, e.g. sigma = 1.4826 median|r| with Huber at 1.345 sigma (factor 1.994) or Cauchy at
 * 2.385 sigma (factor 3.536).  factor > 0 switches it on: ea_batch_solve -- which is also the solver behind ea_solve, every
 * level of ea_solve_pyramid and ea_tracker_push_frame -- starts with ONE ea_batch_residual_quantiles over the auto-scaled
 * problems of the batch at their start poses and then does, per problem, exactly what the caller could have done by hand:
 *   a = max(a_min, factor * Q_prob)   (one IEEE multiplication)   and   ea_problem_set_loss(kind, a)  with the current kind;
 * ea_problem_get_loss reports that a afterwards.  A problem without a valid block at the start pose keeps its a; the trivial
 * loss is left alone.  Cost per solve: the quantile call's 14 launches and one extra synchronisation, and -- the loss having
 * changed -- a rebuild and upload of the batch's descriptor table (resident poses of ea_batch_set_poses are dropped, as after
 * any ea_problem_set_loss).
 * factor finite and >= 0 (0 = off, the default: the loss stays where the last solve left it), prob in [0, 1], a_min finite
 * and > 0: EA_ERR_INVALID_ARG otherwise, checked before the problem is looked at.  Stored on the problem; survives
 * ea_problem_set_points, ea_problem_set_dt and the frame producers, so a setting made on ea_tracker_problem() holds for every
 * push and one made on a pyramid level for that level.  Refused (EA_ERR_INVALID_ARG) on a problem that has terms or is a
 * term, and ea_problem_add_term refuses an auto-scaled problem on either side.
 * These do NOT re-estimate, they run with the problem's current a: ea_batch_solve_starts / ea_solve_starts /
 * ea_*search_starts (a loss belongs to a problem, not to a start), the three sharded solves (each rank would estimate from
 * its own shard and the ranks would diverge), and every evaluation and covariance call. */
int ea_problem_set_loss_auto_scale(ea_problem *p, double factor, double prob, double a_min);
int ea_problem_get_loss_auto_scale(const ea_problem *p, double *factor, double *prob, double *a_min);
/* functor flavour: standalone (utils.h:48-80) = {z_guard 0.01, z_eps 0, rot_transposed 0}
 * [default]; ROS flavour (include/EAResidue.h:86-118) = {0, 0.001, 1} */
int ea_problem_set_flavour(ea_problem *p, double z_guard, double z_eps, int rot_transposed);
int64_t ea_problem_num_points(const ea_problem *p);

/* Residual variants of standalone/utils.h.
 * Distortion: EAResidueEx / EAResidueSecondCamEx (utils.h:102-177, :295-421), coefficients in the order
 * of EAResidueEx::Create(fx,fy,cx,cy, k1,k2,p1,p2,k3, ...) (utils.h:156-160).  All zero = off. */
int ea_problem_set_distortion(ea_problem *p, double k1, double k2, double p1, double p2, double k3);
/* Second camera of a rigid rig: EAResidueSecondCam[Ex] (utils.h:179-292) evaluates
 * b_T_a_SecCam = trans_1to2 * b_T_a * trans_1to2_inv; both row-major 4x4 with last row 0 0 0 1, exactly the
 * ptrans_1to2 / ptrans_1to2_inv arrays.  NULL, NULL = first camera again. */
int ea_problem_set_second_camera(ea_problem *p, const double trans_1to2[16], const double trans_1to2_inv[16]);
/* Several residual families on ONE pose — the reference adds camera-1 and camera-2 blocks to the same
 * ceres::Problem with the same (q,t) (standalone_edge_align.cpp:791-803, :3205-3218).  `term` keeps its own
 * points, DT image, intrinsics, loss and variant; it must outlive `p` (borrowed).  ea_eval / ea_solve on `p`
 * then cover p and all its terms.  Destroy the head (or ea_problem_clear_terms it) before its terms: ea_problem_destroy of
 * the head updates every term it still holds. */
int ea_problem_add_term(ea_problem *p, ea_problem *term);
int ea_problem_clear_terms(ea_problem *p);

/* Per-point weights: ceres::ScaledLoss(loss, w_i, ...) on residual block i, i.e.
 *   problem.AddResidualBlock(cost, new ceres::ScaledLoss(new ceres::CauchyLoss(1.), w_i, ceres::TAKE_OWNERSHIP), q, t);
 * With weights set every evaluation of the problem computes cost = 1/2 sum w_i rho(r_i^2), JtJ = sum w_i rho'_i J_i^T J_i,
 * Jtr = sum w_i rho'_i J_i^T r_i (trivial loss: w_i r_i^2 / 2 ...): ea_eval, ea_cost, the solves (single, batched, pyramid
 * level by level, sharded: each rank weights its shard, multi-start, search), the pose-batched evaluations, the tracker and
 * terms (each term its own weights); priors and constant parameters are untouched.  n_invalid does not look at the weights
 * (a block of weight 0 whose functor returns false still counts, as in Ceres).  Per-point outputs (ea_eval_points,
 * ea_eval_rows*, ea_batch_eval_rows*): corrected != 0 gives sqrt(w_i rho'_i) r_i and sqrt(w_i rho'_i) J_i, corrected == 0
 * the raw, unweighted r_i and row.  ea_*_covariance with apply_loss_function = 0 drops the weights together with the loss;
 * with 1 it inverts the weighted JtJ.  ea_problem_pixel_cost is the reference's own unweighted report and stays so.
 * The weights belong to the point set: whatever replaces the points (ea_problem_set_points*, a reference-frame producer
 * without depth weighting) drops them.  A weighted problem runs the kernels of the residual variants (as a problem with
 * distortion does); a batch rebuilds when weights appear or disappear, not when their values change.
 *
 * ea_problem_set_weights: w = n host doubles in the caller's point order (n = ea_problem_num_points), each finite and >= 0,
 * rounded once to the problem dtype and kept in HBM beside the points, in their storage order (ea_problem_set_point_order).
 * A wrong n, a negative, NaN or infinite weight (fp32 problems: one that overflows float): EA_ERR_INVALID_ARG, nothing
 * changes (a device allocation or copy that fails afterwards -- EA_ERR_HIP -- leaves the previous weights in an unspecified
 * state, like any failed upload).  w == NULL clears the weights (n is ignored).  Points borrowed through ea_problem_set_points_device are copied
 * into arrays the problem owns first (the weights live in the same allocation as z).
 * ea_problem_set_weights_device: the same from n values of the problem dtype already in HBM, caller's order; copied, not
 * borrowed; the values are the caller's responsibility.
 * ea_problem_get_weights: the stored weights as doubles in the caller's order; *count = n, or 0 when no weights are set
 * (nothing is written then).  capacity < n: EA_ERR_INVALID_ARG. */
int ea_problem_set_weights(ea_problem *p, const double *w, int64_t n);
int ea_problem_set_weights_device(ea_problem *p, const void *w, int64_t n);
int ea_problem_get_weights(ea_problem *p, double *w, int64_t capacity, int64_t *count);
/* Depth weighting, a setting on the problem read by every reference-frame producer (ea_problem_set_ref_frame, _masked,
 * _canny, _ros, _ros_scaled, and the tracker's reference step through ea_tracker_problem(tr)): behind the scatter of the
 * points a device kernel writes w_i = min(1, (z_ref / z_i)^power) -- an RGB-D sensor's depth noise grows with z^2 -- with no
 * host round trip.  Computed in fp64 from the STORED z widened to double: one IEEE division z_ref / z_i, then power - 1
 * multiplications by that ratio left to right, then the min with 1, then one rounding to the problem dtype (numpy
 * reproduces it bit for bit).  Points without a usable depth (the ROS producers keep them: z = 0, NaN, negative) get a
 * weight clamped into [0, 1]; their functor fails or not exactly as without weights.  power in 1..8; power = 0 (default) switches it off and clears weights a producer wrote;
 * z_ref must be finite and > 0.  Takes effect at the next producer call. */
int ea_problem_set_depth_weighting(ea_problem *p, double z_ref, int power);

/* One evaluation of the whole problem at pose (q,t) — what ceres' evaluator computes from the
 * N AutoDiffCostFunction<EAResidue,1,4,3> blocks + QuaternionParameterization + loss:
 *   cost = 1/2 sum rho(r_i^2);  JtJ (6x6 row-major) and Jtr (6) of the loss-corrected 1x6 rows
 *   in the tangent ordering [delta(3) | t(3)];  n_invalid = blocks whose functor returned false
 *   (sums then cover the valid blocks only).  Any output pointer may be NULL. */
int ea_eval(ea_problem *p, const double q[4], const double t[3], double *cost, double JtJ[36],
            double Jtr[6], int64_t *n_invalid);
/* per-point outputs (host, n and n*6 row-major; NaN for failed blocks).  corrected != 0:
 * sqrt(rho') r and sqrt(rho') J as handed to the minimiser (sqrt(w_i rho') with weights); 0: raw r_i and raw row. */
int ea_eval_points(ea_problem *p, const double q[4], const double t[3], double *r, double *J,
                   int corrected);
/* residual-only evaluation (the candidate-cost evaluation inside the trust-region loop) */
int ea_cost(ea_problem *p, const double q[4], const double t[3], double *cost,
            int64_t *n_invalid);

/* The reference's own quantitative self-check, printed before and after its solves (standalone_edge_align.cpp:2494-2567
 * "initialCost / InitialMaxCost / Initialmaxpixel", :2704-2776 the same after): every point warped by the pose, x / z and
 * y / z pushed through K, truncated `(int)` to a pixel, the distance transform read there; total, mean over the points,
 * maximum and the (untruncated) pixel of the first point that attains it.  Computed on the device from the points and the
 * DT image the problem already holds.  Upstream reads outside the image unchecked (undefined behaviour): such points are
 * skipped and counted in `outside`; upstream accumulates in float in point order, this sums in double.  Per-point weights
 * (ea_problem_set_weights) do not enter: this is the reference's report. */
typedef struct {
  double total_cost, mean_cost, max_cost;
  double max_pixel[2];      /* (u, v) before truncation */
  int64_t count, outside;   /* points read / points projecting outside the image */
} ea_pixel_cost;
int ea_problem_pixel_cost(ea_problem *p, const double q[4], const double t[3], ea_pixel_cost *out);

/* Exact order statistics of |r_i| at a pose, computed on the device (no per-point copy): the inlier fraction at a threshold,
 * a "did this alignment land" test, the scale of a robust loss.  r_i is the raw residual of block i -- per-point weights, the
 * loss and priors do not enter -- over the VALID blocks, those whose functor returns true at the pose (the rule n_invalid
 * counts); m = their number, returned in *n_valid (nullable).  For prob in [0, 1]: k = floor(prob * (double)(m - 1)), one
 * IEEE multiplication (numpy's method="lower"), and values[j] is the k-th smallest |r|, 0-based -- bit for bit an element of
 * the multiset, never an interpolated value; prob = 0.5 with even m gives the lower median.  fp32 problems: r is the float
 * the kernels compute, widened exactly.  m == 0: the values are NaN and *n_valid = 0, a result and not an error.
 * 1 <= nq <= 16, every prob finite and in [0, 1]: EA_ERR_INVALID_ARG otherwise, before anything touches a device; a problem
 * without points or DT image: EA_ERR_STATE, as ea_eval.  Order statistics of p's OWN residual family: its terms are not
 * included (call it on a term); a batched problem that has terms reports its head family only.
 * One key pass (projection, four row loads, the value of the bicubic patch) and a six-pass most-significant-digit-first radix
 * select over 64-bit keys with integer counts: the same bits on every run.  One launch sequence (14 launches) serves a
 * whole batch, queued on its stream; one synchronisation.  Resident poses (ea_batch_set_poses) survive the call. */
int ea_problem_residual_quantiles(ea_problem *p, const double q[4], const double t[3], const double *probs, int nq,
                                  double *values /* nq */, int64_t *n_valid);

/* How much of a reference is still seen at a pose -- what a keyframe rule asks after every solve -- counted on the device
 * without a per-point copy.  The statistics cover p's OWN residual family (its terms are not included, as for the quantiles);
 * per-point weights, the loss and priors do not enter.
 *   Projection: (u, v) and validity are the evaluation kernels' own -- the plain functor's for plain and weighted problems,
 *     the variant functor's for distortion / second-camera problems -- with the flavour knobs z_guard, z_eps and
 *     rot_transposed applied, in the problem's dtype.
 *   Visible: a valid point (functor returned true) whose divisor b_z + z_eps is > 0 and for which
 *     margin <= floor(u) <= W - 2 - margin and margin <= floor(v) <= H - 2 - margin (the unsaturated floor: a point far
 *     outside, or with NaN coordinates, is simply not visible).
 *   Inlier: visible and |r| <= inlier_residual, r the raw bicubic value the cost kernel and the quantiles' key pass sample.
 *   Flow: (u0, v0) is the same projection at the identity pose q = (1, 0, 0, 0), t = 0 (a rig: T12 I T12^-1).  A visible
 *     point counts in n_flow when its identity projection is valid with a positive divisor; its term is
 *     sqrt((u - u0)^2 + (v - v0)^2), formed and summed in fp64 from the dtype-typed coordinates.
 *   Determinism: the counts are exact; sum_flow has the same bits on every run, whichever batch the problem is in and
 *     whatever sits beside it: a problem's points are cut into fixed workgroup partials (256 points each, a fixed butterfly
 *     inside), folded in index order by a second launch.  No floating-point atomics.
 * Errors, before anything touches a device: NULL argument, margin < 0, inlier_residual negative or NaN (+Inf is allowed):
 * EA_ERR_INVALID_ARG.  A problem without points or DT image: EA_ERR_STATE, as ea_eval.  Two launches and one synchronisation
 * on the batch's stream serve a whole batch.  Resident poses (ea_batch_set_poses) survive the call. */
typedef struct {
  int64_t n;          /* points of the problem's own residual family */
  int64_t n_invalid;  /* functor returned false at the pose (the rule ea_eval's n_invalid counts) */
  int64_t n_visible;  /* valid, positive depth, inside the image by `margin` */
  int64_t n_inlier;   /* visible and |r| <= inlier_residual */
  int64_t n_flow;     /* visible and also visible-by-depth at the identity pose */
  double  sum_flow;   /* sum over the n_flow points of the pixel distance between the two projections */
} ea_pose_stats;
int ea_problem_pose_stats(ea_problem *p, const double q[4], const double t[3], int margin, double inlier_residual,
                          ea_pose_stats *out);

/* ---- the reference's qualitative self-check: reproject (standalone/utils.cpp:497-592) + s_overlay (:594-608) ----------
 * What every edge_align_test* runs before and after its solve: reproject(a_X, b_T_a, K, b_u); s_overlay(imB, b_u, "initial.png").
 *
 * Pose <-> matrix, host only (no device is looked for): PoseManipUtils::raw_to_eigenmat / eigenmat_to_raw, the convention of
 * this header's first lines.  b_T_a is a row-major 4x4.
 *   ea_pose_to_matrix: Eigen's Quaternion::toRotationMatrix arithmetic on q as given (NOT normalised): tx = 2x, ty = 2y,
 *     tz = 2z; twx = tx w, twy = ty w, twz = tz w, txx = tx x, txy = ty x, txz = tz x, tyy = ty y, tyz = tz y, tzz = tz z;
 *     R00 = 1 - (tyy + tzz), R01 = txy - twz, R02 = txz + twy, R10 = txy + twz, R11 = 1 - (txx + tzz), R12 = tyz - twx,
 *     R20 = txz - twy, R21 = tyz + twx, R22 = 1 - (txx + tyy); column 3 = t; last row 0 0 0 1.
 *   ea_matrix_to_pose: Eigen's quaternion from a matrix.  trace > 0: s = sqrt(trace + 1), w = s / 2, s = 0.5 / s,
 *     x = (m21 - m12) s, y = (m02 - m20) s, z = (m10 - m01) s.  Otherwise the largest diagonal entry i with Eigen's tie rule
 *     (start at 0, then m11 > m00, then m22 > m(i,i)), j = (i + 1) % 3, k = (j + 1) % 3: s = sqrt(m(i,i) - m(j,j) - m(k,k) + 1),
 *     q[i] = s / 2, s = 0.5 / s, w = (m(k,j) - m(j,k)) s, q[j] = (m(j,i) + m(i,j)) s, q[k] = (m(k,i) + m(i,k)) s.
 *     m33 != 1: EA_ERR_INVALID_ARG (the reference's assert( T(3,3) == 1 )).
 *   No multiply-add of either is contracted.  NULL argument: EA_ERR_INVALID_ARG. */
int ea_pose_to_matrix(const double q[4], const double t[3], double b_T_a[16]);
int ea_matrix_to_pose(const double b_T_a[16], double q[4], double t[3]);

/* Reprojection: the per-point (u, v) of the problem's OWN residual family (its terms are not included: call it on a term; a
 * batched problem that has terms reports its head family) at a pose given as the matrix b_T_a, as in the reference's
 * signature.  The overload is chosen by the problem's variant: plain = utils.cpp:497, distortion = :512, second camera =
 * :545, both = :560.  Intrinsics are the problem's own (a rig term: K2, as at the reference's call sites).  Weights, loss,
 * priors, constant masks, z_guard / z_eps and rot_transposed do not enter: reproject has none of them.  The constant third
 * row of the reference's b_u is not returned.
 * Arithmetic -- the specification; fp64 throughout, the stored points widened to double (an fp32 problem uses the floats it
 * holds), IEEE divisions, no contracted multiply-add:
 *   A (host)   M = rows 0-2 of b_T_a; second camera: rows 0-2 of (T12 b_T_a) T12^-1 with the matrices given to
 *              ea_problem_set_second_camera, every 4x4 product entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3 summed in k order.
 *              Eigen's own association for that product is not pinned by the reference's build; this fixed order is this
 *              library's definition and agrees with the reference to rounding.
 *   B (device) bx = ((M00 x + M01 y) + M02 z) + M03, by and bz alike; xn = bx / bz, yn = by / bz; with distortion
 *              r2 = xn xn + yn yn, r4 = r2 r2, r6 = r4 r2, rad = ((1 + k1 r2) + k2 r4) + k3 r6,
 *              xd = (xn rad + ((2 p1) xn) yn) + p2 (r2 + (2 xn) xn), yd = (yn rad + ((2 p2) xn) yn) + p1 (r2 + (2 yn) yn);
 *              u = fx xd + cx, v = fy yd + cy.  No validity test: bz == 0 and points behind the camera give what IEEE
 *              gives (Inf, NaN, mirrored pixels), exactly as upstream.
 *   DEVIATION: upstream's reproject reads its Kc positionally as (k1, k2, k3, p1, p2) while every call site fills it in
 *   EAResidueEx::Create's order (k1, k2, p1, p2, k3) (known defects); here k1, k2, p1, p2, k3 mean what their
 *   names say in ea_problem_set_distortion, as in EAResidueEx.
 * Output: ea_problem_reproject -- uv[2 i], uv[2 i + 1] of point i in the CALLER's order (as ea_eval_points), capacity >= n.
 * The batch forms -- the rows layout of ea_batch_row_offsets, the head families' rows in STORAGE order (the order of
 * ea_batch_eval_rows*), 2 doubles per row; a head family's rows that belong to terms are left untouched; a problem without
 * points contributes no rows.  b_T_a: count x 16.  ea_batch_reproject_device: uv_dev is 16-byte aligned device memory of the
 * batch's device, complete when the call returns.
 * Errors, before anything touches a device: NULL argument, a b_T_a whose last row is not exactly 0 0 0 1 or with a non-finite
 * entry, capacity too small: EA_ERR_INVALID_ARG.  A problem without points or DT image: EA_ERR_STATE, as ea_eval.
 * One launch and one synchronisation on the batch's stream serve a whole batch; the matrices go up in a small array of
 * their own: resident poses (ea_batch_set_poses) survive. */
int ea_problem_reproject(ea_problem *p, const double b_T_a[16], double *uv /* n x 2 */, int64_t capacity);
int ea_batch_reproject(ea_batch *b, const double *b_T_a /* count x 16 */, double *uv, int64_t capacity_rows);
int ea_batch_reproject_device(ea_batch *b, const double *b_T_a, double *uv_dev, int64_t capacity_rows);

/* Overlay: s_overlay on the device.  bgr_out = a copy of bgr_in (height x width x 3 bytes; bgr_out == bgr_in is allowed) in
 * which, for every point of the problem's own family, pixel ((int)v, (int)u) -- the cast truncates toward zero -- of the
 * (u, v) above is set to `color` (B, G, R; NULL = {0, 0, 255}, upstream's red).  Upstream writes outside the image unchecked
 * (undefined behaviour); here such points are skipped and counted in `outside`.  A point is `inside` by the rule of
 * ea_problem_pixel_cost: u and v finite, |u|, |v| < 1e9, 0 <= (int)u < width, 0 <= (int)v < height, u > -1, v > -1 (a u in
 * (-1, 0) paints column 0, as upstream's cast does); so for a plain problem and b_T_a = ea_pose_to_matrix(q, t) of a unit q,
 * inside / outside equal ea_problem_pixel_cost's count / outside.  Points that share a pixel store the same three bytes: the
 * image is the same on every run; the counts are exact integers.
 * height, width must equal the DT extent of the problem (of every problem of the batch) -- imB's extent in every upstream
 * call: EA_ERR_INVALID_ARG otherwise, as for the errors of the reprojection, a NULL entry of a pointer array and, for
 * ea_batch_overlay_device, an entry that hipPointerGetAttributes does not report as memory of the batch's device.
 * ea_problem_overlay on a problem without points: EA_ERR_STATE; in a batch such a problem leaves its image a plain copy and
 * its stats zero.  stats: count entries, or NULL.
 * Host forms: the images go up into a cached device block, are painted and come back.  ea_batch_overlay_device paints count
 * device images in place (they must be complete when the call is made): one launch, one synchronisation, nothing but the
 * stats crosses the bus.
 * Out of scope: an Eigen-typed reproject in the C++ shims (Eigen and OpenCV are not dependencies of this library), overlays
 * taken by the trackers themselves, image file formats, anti-aliased or thick marks. */
typedef struct {
  int64_t n, inside, outside;   /* points of the family; painted; skipped */
} ea_overlay_stats;
int ea_problem_overlay(ea_problem *p, const double b_T_a[16], const uint8_t *bgr_in, int height, int width,
                       const uint8_t color[3], uint8_t *bgr_out, ea_overlay_stats *stats);
int ea_batch_overlay(ea_batch *b, const double *b_T_a, const uint8_t *const *bgr_in, int height, int width,
                     const uint8_t color[3], uint8_t *const *bgr_out, ea_overlay_stats *stats);
int ea_batch_overlay_device(ea_batch *b, const double *b_T_a, uint8_t *const *bgr_dev, int height, int width,
                            const uint8_t color[3], ea_overlay_stats *stats);

/* ---- depth-consistency gate: occlusion weights from the current frame's depth ------------------------------------------
 * No upstream equivalent: SolveEA::setNowFrame clones now_depth and never reads it (src/SolveEA.cpp:86-101).  The gate
 * compares the depth of every warped reference point with the depth MEASURED where it lands in the current frame and, on
 * request, writes the outcome into the problem's per-point weights (ceres::ScaledLoss per block) without a host round trip.
 *
 * The current frame's depth, held by the problem.  height x width, row-major.  EA_DEPTH_U16: uint16 as cv::imread gives TUM
 * depth, metric depth = (double)d / z_scaling (one IEEE division), valid when d != 0.  EA_DEPTH_F32: float32 metres as the ROS
 * callbacks hold it, z_scaling ignored, valid when f > 0 and finite (NaN, <= 0 and Inf are "no measurement").  The image is
 * COPIED into a block of the library's cached allocator and kept in its own kind, nothing is converted on the way in; the
 * _device forms copy device memory of the problem's device (complete when the call is made; anything else, as far as the
 * runtime can tell: EA_ERR_INVALID_ARG).  depth == NULL (batch forms: the array itself) drops the held image.  The image
 * survives ea_problem_set_points*, ea_problem_set_dt* and the frame producers: only these calls replace it.  Batch forms: one
 * entry per problem, copies on the batch's stream and ONE wait; the same problem twice in the batch is an error, as in
 * ea_batch_set_frames.  EA_ERR_INVALID_ARG before a problem is looked at or a device is looked for: an unknown kind, height
 * or width outside 3..32768, for U16 a z_scaling that is not finite or <= 0; also a NULL handle or a NULL entry. */
typedef enum { EA_DEPTH_U16 = 0, EA_DEPTH_F32 = 1 } ea_depth_kind;
int ea_problem_set_now_depth(ea_problem *p, const void *depth, int kind, int height, int width, double z_scaling);
int ea_problem_set_now_depth_device(ea_problem *p, const void *depth_dev, int kind, int height, int width, double z_scaling);
int ea_batch_set_now_depth(ea_batch *b, const void *const *depth, int kind, int height, int width, double z_scaling);
int ea_batch_set_now_depth_device(ea_batch *b, const void *const *depth_dev, int kind, int height, int width, double z_scaling);

/* The gate.  ea_default_depth_gate_params: radius 1, abs_tol 0.02, rel_tol 0.02, w_occluded 0, w_free 0, w_unknown 1,
 * apply 1.  The tolerances (2 cm + 2 %) are API defaults that nobody has measured on real sequences.
 * Arithmetic -- the specification; fp64 throughout, the stored points widened to double, IEEE divisions, no contracted
 * multiply-add; the problem's OWN residual family (as reproject, quantiles and pose stats: call it on a term for a term; a
 * batched problem with terms reports its head family):
 *   1  M = step A of ea_*_reproject (rig product included); bx, by, bz, u, v = its step B, distortion by name included.
 *   2  BEHIND when !(bz > 0 && bz < +Inf) (NaN included).
 *   3  else OUTSIDE when (u, v) is not inside by ea_problem_pixel_cost's rule (see ea_problem_overlay), on the extent H x W of
 *      the problem's DT image; iu = (int)u, iv = (int)v, truncating toward zero.
 *   3b the held depth image is height x width = (H << s) x (W << s) for one s in 0..8 (each problem its own s; H * W << 2 s at
 *      most 2^30): c = (2^s - 1) / 2 (exact), U = u * 2^s + c, V = v * 2^s + c (the multiplication is exact, the addition
 *      rounds once, nothing is contracted), iu = (int)U, iv = (int)V, truncating toward zero.  c is the centre of the
 *      2^s x 2^s block of depth pixels whose mean DT pixel 0 is.  s = 0: U = u -- the depth image has the DT extent.  iu or
 *      iv may be negative or past the last column or row; nothing is clamped (step 4 treats such pixels as no measurement).
 *      For the users of ea_problem_set_*_frame_ros_scaled and of pyramid levels: the reference's own reduction of the depth
 *      (NaN -> 0, then the plain 2 x 2 mean) is what back-projection needs and no gate input -- a block with one hole comes
 *      out at 3/4 of the true depth and would be classed OCCLUDED -- so hand the gate the full-resolution depth.
 *   4  window: the pixels (iv + dy, iu + dx), dy outer and dx inner, each from -radius to radius (in depth pixels), that lie in
 *      0 <= row < height, 0 <= col < width and hold a valid measurement d (converted as above); e = fabs(d - bz); the first
 *      such pixel is kept, and any later one with a STRICTLY smaller e (a tie keeps the first in that raster order).  None:
 *      UNKNOWN.  (Edge points sit on depth discontinuities: the single pixel under a point is the least reliable one.)
 *   5  tol = abs_tol + rel_tol * bz, diff = d - bz of the kept d: fabs(diff) <= tol CONSISTENT; else diff < 0 OCCLUDED (a
 *      measured surface lies in front of the point); else FREE (the point hangs in front of everything measured around it).
 *   6  g = 1 for BEHIND, OUTSIDE and CONSISTENT (what the functor makes of those points is not the gate's business);
 *      w_unknown, w_occluded, w_free for the other three.
 * apply != 0: w_i = g_i * dd_i, one IEEE multiplication, rounded once to the problem dtype, where dd_i = 1, or with
 * ea_problem_set_depth_weighting of power > 0 the fp64 value min(1, (z_ref / z_i)^power) exactly as the producers form it
 * before their rounding (one division, power - 1 multiplications left to right, clamped to [0, 1]).  The result REPLACES the
 * problem's weights (the storage of ea_problem_set_weights, behind z, in storage order; borrowed device points are copied
 * into owned arrays first, as there) and the problem becomes a weighted one: a batch rebuilds when weights APPEAR and drops
 * its resident poses then, as after ea_problem_set_weights; when only the values change nothing is rebuilt and resident poses
 * survive.  ea_problem_set_weights(p, NULL, 0) undoes it; a reference-frame producer replaces the weights as it does today.
 * apply == 0 changes nothing on the problem; resident poses always survive.
 * Outputs: exact integer counts, n = the sum of the six classes; cls, one byte per point (EA_GATE_*), nullable --
 * ea_problem_depth_gate: in the CALLER's order (as ea_eval_points), capacity >= n; the batch forms: the rows layout of
 * ea_batch_row_offsets in STORAGE order, rows of terms untouched, a problem without points contributes none (zero stats);
 * cls_dev is device memory of the batch's device.  stats: count entries (nullable in the batch forms).  Same bytes, counts and
 * weight bits on every run, whichever batch a problem sits in.
 * EA_ERR_INVALID_ARG, before anything touches a device (and before a handle is looked at where only the parameters are
 * wrong): a NULL argument, a b_T_a that ea_*_reproject refuses, radius outside 0..3, a tolerance or weight factor that is
 * negative, NaN or infinite, a weight factor that overflows float for an fp32 problem, a capacity that is too small, with
 * apply the same problem twice in the batch (its weights can be written once per call), a cls_dev that is not device
 * memory of the batch's device.
 * EA_ERR_STATE: a problem without points (ea_problem_depth_gate only), DT image or now-depth; a now-depth whose extent is not
 * the DT extent times one power of two as step 3b says (checked here, not by the setters); problems of one call that hold depth of different kinds.  In a batch
 * a problem without depth fails the whole call before any launch.
 * One launch and one synchronisation on the batch's stream serve a whole batch; the matrices go up in a small array of their
 * own; no per-point data crosses the bus unless cls is asked for.
 * ea_tracker_batch_set_depth_gate runs this gate inside the multi-stream tracker, on the pushed depth.
 * Out of scope: gating inside the single ea_tracker_*, gating of terms through the head, soft or continuous weights, any use of the depth as a residual. */
typedef struct {
  int radius;                 /* window half-width in pixels, 0..3 */
  double abs_tol, rel_tol;    /* tol = abs_tol + rel_tol * bz, metres */
  double w_occluded, w_free, w_unknown;   /* weight factors of the three non-consistent classes */
  int apply;                  /* != 0: write the problem's weights */
} ea_depth_gate_params;
void ea_default_depth_gate_params(ea_depth_gate_params *prm);
typedef struct { int64_t n, n_behind, n_outside, n_unknown, n_consistent, n_occluded, n_free; } ea_depth_gate_stats;
enum { EA_GATE_BEHIND = 0, EA_GATE_OUTSIDE = 1, EA_GATE_UNKNOWN = 2, EA_GATE_CONSISTENT = 3, EA_GATE_OCCLUDED = 4, EA_GATE_FREE = 5 };
int ea_problem_depth_gate(ea_problem *p, const double b_T_a[16], const ea_depth_gate_params *prm,
                          uint8_t *cls /* n, caller's order, nullable */, int64_t capacity, ea_depth_gate_stats *stats);
int ea_batch_depth_gate(ea_batch *b, const double *b_T_a /* count x 16 */, const ea_depth_gate_params *prm,
                        uint8_t *cls /* rows layout, nullable */, int64_t capacity_rows, ea_depth_gate_stats *stats /* count, nullable */);
int ea_batch_depth_gate_device(ea_batch *b, const double *b_T_a, const ea_depth_gate_params *prm,
                               uint8_t *cls_dev, int64_t capacity_rows, ea_depth_gate_stats *stats);

/* ---- point selection: the reference's stride, and one point per cell ------------------------------------------------------
 * Every standalone test of the reference thins its edge points before it builds the problem: `i += 30`
 * (standalone_edge_align.cpp:267), `i += 10` (:470), iterStep = N / minNumOfPointsPerimage when N exceeds it (:1216-1221,
 * :2590-2596).  These calls do it to the points a problem holds, on the device: no point or weight crosses the bus.
 * The rule -- the specification; fp64 throughout, the STORED points (the problem dtype) widened to double, IEEE divisions, no
 * contracted multiply-add; the problem's OWN residual family (call it on a term to thin the term):
 *   pixel   the plain pinhole of the problem's own camera at the identity pose, no distortion and no rig (what is wanted is
 *           the reference frame's own pixel): a = x / z, b = y / z; u = fx * a, rounded, then + cx; v = fy * b, rounded, then
 *           + cy; pu = floor(u + 0.5), pv = floor(v + 0.5).  The point HAS A PIXEL iff z > 0 (false for NaN), u and v are
 *           finite, 0 <= pu < width and 0 <= pv < height, compared in double before any conversion to int.  (+ 0.5: a
 *           producer's point lands on the pixel it came from in spite of the rounding of back- and re-projection.)
 *           height x width: as given, or with 0 x 0 the extent of the problem's DT image.
 *   cell    (pv / cell_px) * ceil(width / cell_px) + pu / cell_px, integer divisions.
 *   index   a point's position in the problem's order: the caller's, which for producer points is raster order.
 *   1  cell step (cell_px > 0): of the points that have a pixel one winner per occupied cell -- EA_CELL_FIRST the lowest
 *      index, EA_CELL_NEAREST the smallest z (positive doubles order like their bit patterns), ties by lowest index.  Points
 *      without a pixel: outside == 0 dropped, outside == 1 all kept (they bypass the cell step).  cell_px == 0: no cell step,
 *      no pixel is computed, every point survives it and no_pixel reports 0.
 *   2  stride step, on the ordinal among the survivors of step 1 in point order: ordinals 0, s, 2 s, ... are kept, s = stride,
 *      or with target > 0 the reference's iterStep rule s = m > target ? m / target : 1 (integer division, m = survivors of
 *      step 1).  The survivors keep their relative order.
 *   stats: n_before, no_pixel, after_cells = m, n_after = ceil(m / stride_used), stride_used = s.
 * After the call the problem holds exactly the surviving points, in their order, bit for bit as they were stored, in arrays it
 * owns (borrowed device points are not written); their weights are compacted by the same flags, `weighted` and the origin of
 * the weights unchanged; the version moves: batches rebuild and drop resident poses as after any points setter.  Loss,
 * auto-scale, priors, held coordinates, DT image, now-depth, depth-weighting setting and terms are not touched.  With
 * cell_px == 0, stride == 1, target == 0 the call changes nothing and moves no version.  A problem without points is a
 * result: all stats zero, stride_used 1.
 * One launch sequence -- clear, key pass(es), flag + count, scan, compaction -- and ONE synchronisation on the batch's stream
 * serve a whole call; the same bits on every run.  sel: the problems of the batch the call thins, each at most once, in the
 * order of `stats`; NULL: every problem (nsel ignored).
 * EA_ERR_INVALID_ARG, before a device or a problem is touched: a NULL handle or prm, cell_px outside 0..4096, an unknown
 * cell_rule or outside, stride < 1, target < 0, stride > 1 together with target > 0, a negative extent or only one of
 * height / width, more than 2^26 cells; then: an index of sel out of range or twice.  EA_ERR_STATE, before any problem
 * changes: cell_px > 0 with no extent given and no DT image on a problem; a problem whose points are held in a storage order
 * (tiles: ea_problem_set_point_order(p, 0) before the points are set keeps the caller's order).
 * Out of scope: the single ea_tracker, a knob on the per-problem producers, storage-ordered point sets, selection by residual
 * or by gate class (which composes through the depth gate's weights). */
enum { EA_CELL_FIRST = 0, EA_CELL_NEAREST = 1 };
typedef struct {
  int cell_px;        /* 0: no cell step.  1..4096: side of the square cells, in pixels */
  int cell_rule;      /* EA_CELL_FIRST: lowest point index in the cell; EA_CELL_NEAREST: smallest z, ties by lowest index */
  int outside;        /* points that have no pixel: 0 dropped, 1 all kept (they bypass the cell step) */
  int height, width;  /* pixel grid of the cell step; 0, 0: the extent of the problem's DT image */
  int64_t stride;     /* >= 1: of the survivors of the cell step, in point order, keep ordinals 0, stride, 2 stride, ... */
  int64_t target;     /* 0: off.  > 0: stride_used = m > target ? m / target : 1.  Needs stride == 1 */
} ea_point_selection;
typedef struct { int64_t n_before, no_pixel, after_cells, n_after, stride_used; } ea_point_selection_stats;
void ea_default_point_selection(ea_point_selection *prm);   /* cell 0, FIRST, outside 0, 0 x 0, stride 1, target 0 */
int ea_problem_select_points(ea_problem *p, const ea_point_selection *prm, ea_point_selection_stats *stats /* nullable */);
int ea_batch_select_points(ea_batch *b, const int *sel /* nullable: every problem */, int nsel, const ea_point_selection *prm,
                           ea_point_selection_stats *stats /* nullable, one per selected problem */);

/* ---- carrying reference points between frames: transform in place, and merge -------------------------------------------------
 * The reference places its model points before its main solve: a_X = TransformPrior * o_X (standalone_edge_align.cpp:2385), then
 * a_X2 = TransformFromFirstCam * a_X (:2388).  These calls do both to the points a problem holds, on the device: no point or
 * weight crosses the bus.  The problem's OWN residual family only (call it on a term for a term).
 *
 * TRANSFORM (ea_*_transform_points) -- the specification; fp64 throughout, the STORED point widened to double, no contracted
 * multiply-add:
 *   x' = ((M00 x + M01 y) + M02 z) + M03,  y' = ((M10 x + M11 y) + M12 z) + M13,  z' = ((M20 x + M21 y) + M22 z) + M23
 * (step B's first line of ea_*_reproject), each rounded ONCE to the problem dtype on store.  A point with NaN or Inf gives what
 * IEEE gives.  n, the order and the weights are unchanged; a problem with points has its version moved: batches rebuild and
 * drop resident poses as after any points setter.  Borrowed device points are first copied into arrays the problem owns and
 * are never written.  Two calls round twice: the chain is not the product matrix.  One launch and ONE synchronisation per call
 * for any number of problems; the matrices travel in the call's records.
 * EA_ERR_INVALID_ARG, before a device or a problem is touched: a NULL argument, a non-finite entry, a last row that is not
 * exactly 0 0 0 1, an index of sel out of range or twice.  EA_ERR_STATE: points held in a storage order (tiles).
 *
 * MERGE (ea_*_merge_points).  After the call dst holds its own points first -- unchanged, bit for bit, in their order -- and
 * behind them the carried points of src, in src order.  src is not touched.  The rule for a src point; every step fp64 in the
 * stated order:
 *   1  transform as above with dst_T_src and round to dst's dtype.  Every later step sees this rounded value widened again, so
 *      the pixel and cell of a carried point are exactly what ea_problem_select_points computes for it afterwards.
 *   2  pixel test, with require_pixel, and implied by max_dt >= 0 or cell_px > 0: the point must HAVE A PIXEL (point selection's
 *      rule above) under dst's camera on height x width -- as given, or with 0 x 0 the extent of dst's DT image -- with
 *      margin <= pu < width - margin and margin <= pv < height - margin.  A failing point counts in no_pixel.
 *   3  edge test (max_dt >= 0): the value ea_problem_get_dt returns at (pv, pu) -- the image in the problem dtype, not its
 *      float32 mirror --, widened to double, must be <= max_dt; NaN fails.  A failing point counts in off_edge.  A given extent
 *      must lie inside the DT image's.
 *   4  cell step (cell_px > 0), on point selection's cells: a cell that holds any dst point with a pixel (no margin) is
 *      occupied, and candidates there count in `occupied`; a free cell takes one winner -- EA_CELL_FIRST the lowest src index,
 *      EA_CELL_NEAREST the smallest z', ties by lowest index -- and the losers count in lost_cell.
 *   5  cap (max_carried > 0): of the survivors in src order those whose ordinal is >= max_carried count in `capped`.
 *   stats: n_dst, n_src, the five counts, carried, n_after = n_dst + carried;
 *          n_src = no_pixel + off_edge + occupied + lost_cell + capped + carried.
 * Weights: the result is weighted iff dst is, src is, or weight_scale != 1.  Then the own points of a dst that was not weighted
 * get exactly 1, and a carried point w_src * weight_scale (w_src = 1 for an unweighted src): one IEEE multiplication in double,
 * rounded to the dtype.  weights_from_depth is cleared when any point is carried.
 * carried == 0 changes nothing and moves no version.  Otherwise dst's points live in fresh arrays it owns (borrowed ones are
 * not written) and its version moves.  A dst without points and every filter off is the reference's a_X2 = T * a_X copy.
 * One launch sequence -- clear, occupancy, key pass(es), flag + count, scan, copy + compaction -- and ONE synchronisation on
 * the batch's stream serve a whole call; plain stores and integer minima: the same bits on every run.
 * sel: the dst problems of the batch, each at most once, in the order of src, dst_T_src and stats; NULL: every problem.
 * EA_ERR_INVALID_ARG, before a device or a problem is touched: a NULL argument, require_pixel outside 0 / 1, margin < 0, max_dt
 * NaN, cell_px outside 0..4096, an unknown cell_rule, a negative extent or only one of height / width, more than 2^26 cells,
 * max_carried < 0, weight_scale not finite or <= 0, a bad matrix (as above); then: an index of sel out of range or twice,
 * dst == src, a src that is also a dst of the call, differing dtypes or devices, a given extent beyond the DT image with
 * max_dt >= 0.  EA_ERR_STATE, before any problem changes: a pixel test without an extent (no height / width, no DT image),
 * max_dt >= 0 without a DT image, points held in a storage order on either side.
 * Out of scope: per-point age or observation counts, depth fusion of a carried point with the new frame's depth, pyramid
 * levels and the single ea_tracker (see ea_tracker_batch_set_point_carry), storage-ordered point sets, merging terms through
 * the head. */
typedef struct {
  int require_pixel;    /* 1: a carried point must have a pixel in dst (select_pixel) */
  int margin;           /* >= 0: ... at least this many pixels inside the extent */
  double max_dt;        /* >= 0: and dst's DT image at that pixel must be <= max_dt; < 0: off */
  int cell_px;          /* 0: off; else carried points never enter a cell dst already occupies,
                           and at most one carried point enters a free cell */
  int cell_rule;        /* EA_CELL_FIRST / EA_CELL_NEAREST among the candidates of one free cell */
  int height, width;    /* 0, 0: dst's DT extent */
  int64_t max_carried;  /* 0: no cap; else the first max_carried survivors in src order */
  double weight_scale;  /* > 0, finite; 1 by default */
} ea_point_merge;
typedef struct { int64_t n_dst, n_src, no_pixel, off_edge, occupied, lost_cell, capped,
                 carried, n_after; } ea_point_merge_stats;
void ea_default_point_merge(ea_point_merge *prm);   /* everything off, weight_scale 1 */
int ea_problem_transform_points(ea_problem *p, const double a_T_o[16]);
int ea_batch_transform_points(ea_batch *b, const int *sel /* NULL: all */, int nsel,
                              const double *a_T_o /* nsel x 16 */);
int ea_problem_merge_points(ea_problem *dst, const ea_problem *src, const double dst_T_src[16],
                            const ea_point_merge *prm, ea_point_merge_stats *stats /* nullable */);
int ea_batch_merge_points(ea_batch *dst, const int *sel, int nsel, ea_problem *const *src,
                          const double *dst_T_src /* nsel x 16 */, const ea_point_merge *prm,
                          ea_point_merge_stats *stats /* nullable, one per dst */);

/* ceres::Solve(options, &problem, &summary) (standalone_edge_align.cpp:286; SolveEA.cpp:198).
 * q,t in/out.  The whole trust-region loop runs on the device. */
int ea_solve(ea_problem *p, const ea_options *opt, double q[4], double t[3], ea_summary *summary);

/* One problem whose points are sharded over several processes / GPUs: every rank holds a shard of
 * the points (ea_problem_set_points with its slice) and the whole DT image.  Per iteration: local fused evaluation ->
 * 32 accumulator slots -> `allreduce` (in-place sum over all ranks; 0 = success) -> the same trust-region step on every
 * rank (deterministic: no broadcast).  Every rank must call it with the same options and initial pose.  summary->
 * num_point_evals counts the local shard.
 * A rank may hold no point at all (ea_problem_set_points with n = 0, or never called), or none of one term: it takes part
 * in every exchange with zeros and ends with the pose, summary and trace of the other ranks.  Loss, functor, flavour,
 * terms, prior and constant parameters are set alike on every rank; the prior and the mask are applied once, to the reduced
 * system.  A block that fails on one rank fails the evaluation on all (the count travels in the exchange). */
typedef int (*ea_allreduce_fn)(double *buf, int count, void *user);
int ea_solve_sharded(ea_problem *p, const ea_options *opt, ea_allreduce_fn allreduce, void *user, double q[4], double t[3],
                     ea_summary *summary);
/* The same solve with the exchange kept ON THE STREAM ("no host round-trip"): per iteration
 * the library enqueues, on one HIP stream, fused evaluation -> fold into `device_sums` (32 doubles of 16-byte aligned DEVICE memory owned
 * by the caller, e.g. the storage of a torch tensor) -> `allreduce(device_sums, 32, stream, user)`, which must ENQUEUE an
 * in-place sum over all ranks on that stream (RCCL: ncclAllReduce on it, or torch.distributed under an ExternalStream)
 * and return without waiting -> the trust-region step kernel, which reads `device_sums`.  Iterations are enqueued in
 * rounds of opt->iterations_per_sync (default 4); the host looks at the device's progress word once per round, and since
 * every rank computes the same state from the same sums, every rank stops after the same round: the number of
 * collectives enqueued is identical on all ranks.  `hip_stream` is the hipStream_t as a void pointer. */
typedef int (*ea_device_allreduce_fn)(void *device_buf, int count, void *hip_stream, void *user);
int ea_solve_sharded_device(ea_problem *p, const ea_options *opt, ea_device_allreduce_fn allreduce, void *user,
                            double *device_sums, double q[4], double t[3], ea_summary *summary);

/* ---- several GPUs: one communicator rank per GPU, RCCL over xGMI, called from librccl directly -------------------------
 * The path shards by INDEPENDENT frame pairs -- the unit is one ceres::Solve per pair (standalone_edge_align.cpp:286,
 * src/SolveEA.cpp:198): every GPU solves its own ea_batch, no data-path collective -- and the one exchange step is the
 * all-gather of the solved poses.  librccl is opened on first use (dlopen): callers that stay on one GPU never load it.
 * One rank per GPU, either as one process per GPU (ea_comm_get_unique_id on rank 0, the 128 bytes handed to the others
 * by whatever launched them, ea_comm_create on every rank) or as host threads of one process (ea_comm_create_all, one
 * communicator per device, each used by the thread that drives that device). */
typedef struct ea_comm ea_comm;
#define EA_COMM_ID_BYTES 128
int ea_comm_get_unique_id(unsigned char id[EA_COMM_ID_BYTES]);
int ea_comm_create(ea_comm **out, const unsigned char id[EA_COMM_ID_BYTES], int nranks, int rank, int device);
int ea_comm_create_all(ea_comm **out /* ndev entries */, const int *devices /* NULL = 0 .. ndev-1 */, int ndev);
void ea_comm_destroy(ea_comm *c);
int ea_comm_rank(const ea_comm *c);
int ea_comm_size(const ea_comm *c);
/* THE collective of the batch mode: every rank hands in the `count` poses it solved (q: count x 4, t: count x 3, status:
 * count ints such as ea_summary.termination, NULL = zeros) and receives all nranks x count of them in rank order (any of
 * the three outputs may be NULL).  ONE ncclAllGather of count x 8 doubles, enqueued on the stream of `after` -- the batch
 * whose ea_batch_solve produced the poses; NULL = the communicator's own stream -- one synchronisation.  `count` must be
 * the same on every rank (BASELINE config C4: 32). */
int ea_comm_gather_poses(ea_comm *c, ea_batch *after, const double *q, const double *t, const int *status, int count,
                         double *all_q, double *all_t, int *all_status);
/* The point-sharded solve with the exchange issued by the library itself, nothing leaving the device.  Every rank calls it
 * with its shard of the points (and the whole DT image), the same options and the same start pose.  When every rank's shard
 * is small enough for one workgroup per CU (settled by one small MAX all-reduce up front) an iteration is ONE kernel launch
 * + ONE in-place ncclAllReduce of the shard's partial rows (a few tens of KB): the next launch folds the summed rows, takes
 * the trust-region step in every workgroup and evaluates at the new pose.  Otherwise: evaluation -> fold ->
 * ncclAllReduce(32 doubles, sum) -> step kernel per iteration (ea_solve_sharded_device's sequence). */
int ea_solve_sharded_comm(ea_problem *p, const ea_options *opt, ea_comm *c, double q[4], double t[3], ea_summary *summary);
/* key in {"allreduces", "allgathers", "row_solves", "device"}: collectives enqueued so far (tests: equal on every rank);
 * sharded solves that took the one-launch-per-iteration form */
int ea_comm_get_info(const ea_comm *c, const char *key, int64_t *value);
/* number of HIP runtimes (libamdhip64) mapped in this process.  1 is the only healthy answer: PyTorch-ROCm ships its own
 * copy under the same SONAME, so a process that imports torch FIRST shares one runtime with this library, while loading
 * this library first maps two -- streams and device pointers of one are then not objects of the other (ea_comm_* and the
 * on-stream collectives refuse to run). */
int ea_hip_runtime_copies(void);

/* Coarse-to-fine driver (BASELINE config C3; the reference has no pyramid): levels[0] = finest.
 * Solves levels[nlevels-1] first and carries q, t down level by level; every level is a complete problem with its own
 * points, DT image and (caller-scaled) intrinsics.  summaries: nlevels entries or NULL. */
int ea_solve_pyramid(ea_problem *const *levels, int nlevels, const ea_options *opt, double q[4], double t[3],
                     ea_summary *summaries);

/* Frame-to-frame driver (upstream aligns one stored pair, src/ea.cpp:155-200): every pushed frame
 * is aligned against the previous one, starting from the last relative pose; pre-processing (flavour 0: get_aX /
 * get_distance_transform, 1: the Canny forms) and solve stay on the device.  q_rel, t_rel: pose of the previous frame
 * in the new frame's coordinates (identity for the first frame); *aligned (nullable) = 1 when a solve took place. */
typedef struct ea_tracker ea_tracker;
int ea_tracker_create(ea_tracker **out, const ea_camera *cam, int dtype, int device, int flavour);
void ea_tracker_destroy(ea_tracker *tr);
ea_problem *ea_tracker_problem(ea_tracker *tr); /* the problem it drives (set loss / flavour knobs on it) */
int ea_tracker_push_frame(ea_tracker *tr, const uint8_t *bgr, const uint16_t *depth, int height, int width,
                          double z_scaling, const ea_options *opt, double q_rel[4], double t_rel[3],
                          ea_summary *summary, int *aligned);

/* ---- batches of independent frame pairs (one launch sequence for all of them) --------- */
int ea_batch_create(ea_batch **out, ea_problem *const *problems, int count);
void ea_batch_destroy(ea_batch *b);
int ea_batch_count(const ea_batch *b);
/* q: count x 4, t: count x 3, cost: count, JtJ: count x 36, Jtr: count x 6, n_invalid: count */
int ea_batch_eval(ea_batch *b, const double *q, const double *t, double *cost, double *JtJ,
                  double *Jtr, int64_t *n_invalid);
int ea_batch_solve(ea_batch *b, const ea_options *opt, double *q, double *t,
                   ea_summary *summaries);
/* q: count x 4, t: count x 3; values: count x nq; n_valid: count or NULL (ea_problem_residual_quantiles per problem, one
 * launch sequence, one synchronisation; a problem without points gives NaN and 0) */
int ea_batch_residual_quantiles(ea_batch *b, const double *q, const double *t, const double *probs, int nq,
                                double *values, int64_t *n_valid);
/* q: count x 4, t: count x 3; out: count (ea_problem_pose_stats per problem, bit for bit; two launches, one synchronisation;
 * a problem without points gives zeros, as the batched quantiles give NaN and 0) */
int ea_batch_pose_stats(ea_batch *b, const double *q, const double *t, int margin, double inlier_residual, ea_pose_stats *out);

/* K evaluations of every problem of the batch at K DIFFERENT poses, one call -- what a caller that runs its own optimiser,
 * a line search, multi-start or a cost-surface probe asks of the evaluator: ceres::Problem::Evaluate once per pose (the
 * reference's own call of it: src/SolveEA.cpp:241).  q: K x count x 4, t: K x count x 3 (pose k of problem i at
 * [k * count + i]); outputs in the layout of ea_batch_eval with the same leading index: cost K x count, JtJ K x count x 36,
 * Jtr K x count x 6, n_invalid K x count; any of them may be NULL.  Independent evaluations do not queue up behind each
 * other: the pose is a batch dimension of the launch -- G poses per evaluation launch (grid = chunks x G x terms, every
 * (point, pose) pair through the whole per-point arithmetic) and one fold launch for their partial rows, ceil(K / G) such
 * pairs, the results folded straight into pinned host memory, ONE synchronisation: well under 1 us per evaluation of a
 * 5e4-point pair from a few dozen poses on, against ~27 us through ea_batch_eval.  The sums of pose k are those
 * ea_batch_eval returns at pose k up to rounding (the pose-batched launch takes a throughput shape -- more points per
 * lane -- so the partial rows are cut differently, and the pose-dependent constants are built on the device); any split of
 * the K poses over launches gives the same bits.  From 1024 poses on an fp64 batch is evaluated with one pose per lane
 * (tuning key "poses_lane_per_pose" below).  Every kind of batch is covered (variant functors, shared-pose terms,
 * LDS staging). */
int ea_batch_eval_poses(ea_batch *b, int K, const double *q, const double *t, double *cost, double *JtJ, double *Jtr,
                        int64_t *n_invalid);
/* The same in two halves, for a caller that evaluates the same poses again (or wants the upload off its critical path):
 * ea_batch_set_poses makes K poses per problem resident in HBM (56 bytes per pose go up; the pose-dependent constants
 * the kernels read are built by a device kernel); ea_batch_eval_resident_poses runs their K evaluations.  A change of
 * the batch's problems (points, DT image, loss, tuning) drops the resident poses: EA_ERR_STATE until they are set again. */
int ea_batch_set_poses(ea_batch *b, int K, const double *q, const double *t);
int ea_batch_eval_resident_poses(ea_batch *b, double *cost, double *JtJ, double *Jtr, int64_t *n_invalid);

/* Multi-start: K trust-region solves of every problem of the batch from K different starting poses, in lock-step on the device
 * -- K independent ceres::Solve calls on the same ceres::Problem from K initial values, for a caller that does not trust one
 * start (relocalisation, a dropped frame, a wide baseline) and wants the best of several.
 * q: K x count x 4, t: K x count x 3 (start k of problem i at [k * count + i], the layout of ea_batch_eval_poses),
 * overwritten with the K x count solved poses; summaries: K x count or NULL; best: count entries or NULL --
 * the start with the smallest final_cost among those whose termination is not EA_FAILURE (ties: lowest k), -1 if none.
 * Every start is a complete solve under `opt` (LM or dogleg, Ceres' radius rules and termination tests, its own summary and
 * trace); the problem's NormalPriors and constant coordinates apply to every start of it; a start whose first evaluation fails
 * ends with EA_WHY_INITIAL_EVAL_FAILED on its own.  Per iteration one pose-batched evaluation launch covers the starts still
 * running and one step launch runs their state machines; finished starts leave the launches.  A start's result -- pose,
 * iterations, trace -- is bit for bit what the same start gives alone (K = 1): it does not depend on K, on the other starts,
 * on "poses_per_launch" or on when another start finished, and it_cost[0] is the cost ea_batch_eval_poses returns at the
 * start pose -- to the bit where that call evaluates with the same kernel (fewer poses than the "poses_lane_per_pose"
 * threshold, or the key at 0), to rounding above it.  (Against ea_batch_solve from the same start the iterates agree up to rounding only: the pose-batched launch
 * cuts the partial rows differently.)
 * Covered in lock-step: the batches ea_batch_eval_poses evaluates in its flat form -- plain functor, one term per problem,
 * any dtype -- at the pose path's default 256-thread shape; every other batch (variant functors, shared-pose terms, LDS
 * staging, "wide_accumulate", "threads" = 1024) is solved start after start through ea_batch_solve.  ea_batch_get_info
 * "starts_form" reports which form the last call took (1 = lock-step), "starts_launches" its evaluation launches.
 * K < 1 or K x count > 16384: EA_ERR_INVALID_ARG.  Poses made resident by ea_batch_set_poses SURVIVE the call:
 * ea_batch_eval_resident_poses afterwards returns what it returned before. */
int ea_batch_solve_starts(ea_batch *b, int K, const ea_options *opt, double *q, double *t,
                          ea_summary *summaries, int *best);
int ea_solve_starts(ea_problem *p, int K, const ea_options *opt, double *q, double *t,
                    ea_summary *summaries, int *best);   /* one problem: count = 1 */

/* Cost-only evaluation at K poses per problem: cost = 1/2 sum rho(r^2) (+ the problem's NormalPriors) and n_invalid, in the
 * layout of ea_batch_eval_poses (cost, n_invalid: K x count, either may be NULL) -- what a line search, a cost-surface
 * probe or a ranking of candidate poses needs.  A kernel of its own runs the projection, the four row loads, the VALUE of
 * the bicubic patch and rho per (point, pose): no Jacobian row, no JtJ / Jtr products, two sums instead of 28.  The cost
 * agrees with ea_batch_eval_poses' at the same pose up to rounding (the same points summed in another order), n_invalid
 * exactly; a pose gives the same bits alone, in any split over launches ("poses_per_launch"), in either "poses_order" and
 * in any company.  ea_batch_cost_poses = ea_batch_set_poses + ea_batch_cost_resident_poses; the poses stay resident, and
 * the call may be interleaved with ea_batch_eval_resident_poses on the same poses.  No poses resident: EA_ERR_STATE.
 * Covered by the cost kernel: the batches ea_batch_eval_poses evaluates in its flat form at 256-thread workgroups; every
 * other batch (variant functors, shared-pose terms, LDS staging, "wide_accumulate", "threads" = 1024) runs the full
 * evaluation with only the cost fetched.  ea_batch_get_info "cost_form": 1 = the cost kernel served the last call, 0 = the
 * fall-back; ea_batch_set_tuning "cost_form" = 0 forces the fall-back (A/B). */
int ea_batch_cost_poses(ea_batch *b, int K, const double *q, const double *t, double *cost, int64_t *n_invalid);
int ea_batch_cost_resident_poses(ea_batch *b, double *cost, int64_t *n_invalid);
/* Ranked search in front of the multi-start solve: K candidate poses per problem (q: K x count x 4, t: K x count x 3, not
 * modified) are ranked by one cost-only evaluation each, and the M best of every problem are solved in lock-step
 * (ea_batch_solve_starts with M starts).  A candidate is ELIGIBLE if its cost is finite and n_invalid == 0 (a start whose
 * functor fails ends EA_WHY_INITIAL_EVAL_FAILED anyway, and a sum over fewer points would rank unfairly); ranks are the
 * eligible candidates by ascending cost, ties to the lower candidate index, then the ineligible ones by ascending index.
 * picked: M x count or NULL, picked[m * count + i] = the candidate of rank m for problem i.  q_out: M x count x 4, t_out:
 * M x count x 3 = the solved poses of the picked starts; summaries: M x count or NULL; best: count entries or NULL, as in
 * ea_batch_solve_starts over the M ranks (an index into the ranks, not into the candidates).  Requires 1 <= M <= K and
 * M x count <= 16384: EA_ERR_INVALID_ARG otherwise, before anything touches the device.  Afterwards the K CANDIDATES are
 * the batch's resident poses (whatever ea_batch_set_poses had made resident before is replaced). */
int ea_batch_search_starts(ea_batch *b, int K, const double *q, const double *t, int M, const ea_options *opt,
                           double *q_out, double *t_out, int *picked, ea_summary *summaries, int *best);
int ea_search_starts(ea_problem *p, int K, const double *q, const double *t, int M, const ea_options *opt,
                     double *q_out, double *t_out, int *picked, ea_summary *summaries, int *best);   /* count = 1 */

/* ---- pose covariance: ceres::Covariance (Ceres <= 2.1) at one pose per problem ----------------------------------------
 * C = (JtJ)^-1 over the tangent coordinates [delta(3) | t(3)]: the JtJ ea_eval returns at that pose (every term of the
 * problem summed in), loss-corrected rows sum rho' J J^T when apply_loss_function != 0 (every shipped loss has
 * rho'' <= 0), raw rows sum J J^T otherwise.  A residual block whose functor fails at the pose (n_invalid > 0) leaves
 * the covariance "not computed", as Ceres' failed Jacobian evaluation does.
 * Rank: eigenvalues lambda_1 >= ... >= lambda_6 of JtJ (the squared singular values of J).
 *   EA_COV_DENSE_SVD: max_rank = 6 - null_space_rank; for i < max_rank lambda_i / lambda_1 >= min_reciprocal_condition_number,
 *     a failure = "not computed" when null_space_rank >= 0, truncation from there on when it is -1; C = the
 *     pseudo-inverse over the kept eigenpairs.
 *   EA_COV_SPARSE_QR (Ceres' default): full rank required, C = the plain inverse.  DEVIATION: Ceres decides the rank by
 *     SuiteSparseQR's column-norm tolerance; here by the DENSE_SVD test with null_space_rank = 0.
 * Ambient blocks (GetCovarianceBlock): qq = L C_dd L^T, qt = L C_dt, tt = C_tt, with L the 4x3
 * QuaternionParameterization::ComputeJacobian at q as given (not normalised).
 * A rank-deficient system is a RESULT (ok = 0), not an error.  The evaluation, the decomposition and the lift run on the
 * device, behind one synchronisation; resident poses (ea_batch_set_poses) are left in place. */
typedef enum { EA_COV_SPARSE_QR = 0, EA_COV_DENSE_SVD = 1 } ea_cov_algorithm;
typedef struct {
  int algorithm;                           /* ea_cov_algorithm */
  double min_reciprocal_condition_number;  /* 1e-14 */
  int null_space_rank;                     /* 0; -1 = automatic truncation (DENSE_SVD) */
  int apply_loss_function;                 /* 1 */
} ea_covariance_options;
typedef struct {
  int ok;                  /* 1: computed */
  int why;                 /* 0 ok, 1 rank deficient / ill-conditioned, 2 invalid residual blocks, 3 no points,
                              4 (tracker) the solve failed */
  int rank;                /* eigenpairs kept */
  int64_t n_invalid;       /* blocks whose functor failed at the pose */
  double cost;             /* 1/2 sum rho(r^2) (1/2 sum r^2 with the loss off) */
  double eigenvalues[6];   /* of JtJ, descending */
  double tangent[36];      /* 6x6 row-major, [delta | t] */
  double qq[16], qt[12], tt[9];  /* ambient blocks, row-major */
} ea_covariance;
void ea_default_covariance_options(ea_covariance_options *o);  /* SPARSE_QR, 1e-14, 0, 1 */
/* q, t: the pose; EA_ERR_STATE for a problem without points or DT image (as ea_eval) */
int ea_problem_covariance(ea_problem *p, const double q[4], const double t[3], const ea_covariance_options *o,
                          ea_covariance *out);
/* q: count x 4, t: count x 3, out: count entries; a problem without points gives ok = 0, why = 3 */
int ea_batch_covariance(ea_batch *b, const double *q, const double *t, const ea_covariance_options *o, ea_covariance *out);
/* o = NULL: off (default).  On: every ea_tracker_push_frame that solves computes the covariance at the pose it returns,
 * from the points and DT image that solve used (before the new frame's points replace them). */
int ea_tracker_set_covariance(ea_tracker *tr, const ea_covariance_options *o);
/* the covariance of the last push (ok = 0 when its solve failed); EA_ERR_STATE when the last push did not align or
 * covariance is off */
int ea_tracker_last_covariance(ea_tracker *tr, ea_covariance *out);

/* ---- pose priors: ceres::NormalPrior(A, b) on the q or t block (Ceres <= 2.1) ----------------------------------------
 * Residual r = A (x - b) with A k x n (k >= 1, n = 4 for q, 3 for t), cost 1/2 |A (x - b)|^2, no loss function; tangent
 * Jacobian A P(q) on q (P = QuaternionParameterization::ComputeJacobian), A on t.  It enters the solve only through the 6x6
 * system: H = A^T A (formed once here in fp64 and kept with b -- a deviation from keeping A, at rounding level) adds P^T H P
 * or H to JtJ, P^T H (q - b) or H (t - b) to Jtr and 1/2 (x - b)^T H (x - b) to the cost, always in fp64 (fp32 problems
 * too).  Priors on q and t are independent.
 * Included: ea_eval, ea_cost, ea_batch_eval, ea_batch_eval_poses / _resident_poses, every solve (ea_solve, ea_batch_solve,
 * ea_solve_pyramid per level, the sharded forms), ea_problem_covariance / ea_batch_covariance (whatever
 * apply_loss_function says: a prior has no loss; a prior can make a rank-deficient system full rank).
 * NOT included: the per-point outputs -- ea_eval_points, the rows API (ea_eval_rows*, ea_batch_eval_rows*), and
 * ea_problem_pixel_cost.
 * Sharded solves add the prior once, to the all-reduced system, on every rank: every rank must set the same prior.
 * block: 0 = quaternion, 1 = translation; A: k x n row-major; A == NULL or k == 0 clears the block's prior.
 * EA_ERR_INVALID_ARG (checked before anything else): bad block, k < 0, non-finite A or b, b == NULL with A given, and a
 * problem that is a term of another (ea_problem_add_term, which in turn refuses a term that carries a prior).
 * Bumps the problem's version: batches holding it rebuild their tables. */
int ea_problem_set_normal_prior(ea_problem *p, int block, const double *A, int k, const double *b);
/* Motion prior of the tracker: each push's solve carries NormalPriors centred on its start pose (the constant-velocity
 * prediction), A = I4 / sigma_rot on q and A = I3 / sigma_trans on t.  sigma_rot is in quaternion-component units: about
 * half the rotation angle in radians for small rotations.  sigma_trans is in the units of t.  0 disables that block; both
 * 0 (the default) = off.  While on, it replaces any prior set on ea_tracker_problem() at every push; switching it off clears
 * a block only while it still holds the prior the last push installed (a prior the caller set since is kept).  Tracker
 * covariance (ea_tracker_set_covariance) includes it. */
int ea_tracker_set_motion_prior(ea_tracker *tr, double sigma_rot, double sigma_trans);

/* ---- constant parameters: Problem::SetParameterBlockConstant / SubsetParameterization (Ceres <= 2.1) ------------------
 * tangent_constant[6] in the solver's ordering [delta0 delta1 delta2 | tx ty tz]; non-zero = held.  NULL = all variable.
 * What Ceres <= 2.1 can express: all three delta held = SetParameterBlockConstant(q); any subset of t held =
 * SubsetParameterization(3, ...) on t, all three = SetParameterBlockConstant(t).  EXTENSION: holding only some of the delta
 * -- the update rotation's delta then stays in the span of the free axes (q itself is still updated by
 * QuaternionParameterization::Plus with that delta); Ceres has no counterpart.
 * Solves (ea_solve, ea_batch_solve with a mask per problem, ea_solve_pyramid with each level's own mask, the sharded forms,
 * the tracker) remove the held coordinates from the program as Ceres does: the step is the LM / dogleg step of the reduced
 * m x m system over the free coordinates; Jacobi scaling, the LM diagonal, the model cost change, the step norm and the
 * gradient max-norm come from the free columns only; x_norm of the parameter-tolerance test covers the ambient coordinates
 * of the non-constant blocks (q while any delta is free, t while any component is).  Held t components, and q when all delta
 * are held, come back bit-identical to the input.  Priors are added first, the mask afterwards: a prior on a constant block
 * contributes only to the reported cost.  All six held: one cost evaluation, no step, EA_CONVERGENCE / EA_WHY_FUNCTION_TOL,
 * num_iterations = 0, initial_cost == final_cost (Ceres' "no non-constant parameter blocks"); a failed evaluation there
 * gives EA_FAILURE / EA_WHY_INITIAL_EVAL_FAILED.  The held columns of an evaluation are not inspected.
 * Covariance (ea_problem_covariance, ea_batch_covariance, the tracker's): decomposition and rank rule run on the reduced
 * m x m JtJ (DENSE_SVD: max_rank = m - null_space_rank; SPARSE_QR: full rank m); `tangent` has zero rows and columns for
 * held coordinates, `eigenvalues` the m values in descending order followed by zeros, the ambient blocks are lifted from
 * the reduced result (a constant block gives zero blocks); all six held: ok = 1, rank = 0, everything zero.
 * NOT affected -- these return the full 6x6 system as without a mask: ea_eval, ea_cost, ea_batch_eval, ea_batch_eval_poses /
 * _resident_poses, ea_eval_points, the rows API.
 * Stored on the head problem only: EA_ERR_INVALID_ARG for a problem that is a term of another, and ea_problem_add_term
 * refuses a term that carries a mask.  Sharded solves apply the mask to the all-reduced system: every rank must set the same
 * mask.  Bumps the problem's version; survives ea_problem_set_points, ea_problem_set_dt and the frame producers, so a mask
 * set on ea_tracker_problem() holds for every push. */
int ea_problem_set_constant_parameters(ea_problem *p, const int tangent_constant[6]);
int ea_problem_get_constant_parameters(const ea_problem *p, int tangent_constant[6]);

/* ---- materialised mode: the "EAResidue batch Evaluate" view -------------------------------------------------------
 * Replaces N calls of ceres::AutoDiffCostFunction<EAResidue,1,4,3>::Evaluate followed by the parameterisation's 4x3
 * plus-Jacobian (standalone/utils.h:48-92, standalone_edge_align.cpp:261-278): residual r and the effective 1x6 row
 * [d r / d delta | d r / d t] of EVERY point, written in the batch's dtype (float / double) -- for a caller that runs its
 * own solver on the rows.  Rows of problem i are [offsets[i], offsets[i+1]) (terms of a problem adjacent, points in
 * their storage order: ea_problem_get_points).  layout 0: J row-major [rows][6]; 1: column-major [6][rows].
 * corrected != 0: rows scaled by sqrt(rho'(r^2)) (Ceres' Corrector, alpha = 0).  A functor that returns false
 * (utils.h:70-73) leaves a NaN row and is counted in *n_invalid (Ceres fails the whole evaluation then).
 * This mode is bandwidth-bound: 3 s bytes in, 7 s bytes out per point plus one pass over the DT image. */
int ea_batch_row_offsets(ea_batch *b, int64_t *offsets /* count + 1 */);
/* into DEVICE memory of the batch's GPU owned by the caller (e.g. the storage of a torch tensor), 16-byte aligned,
 * capacity_rows >= offsets[count]; complete and visible when the call returns (the batch's stream is synchronised).
 * r_dev == J_dev == NULL: into the library's own arrays (then read them with ea_batch_eval_rows). */
int ea_batch_eval_rows_device(ea_batch *b, const double *q, const double *t, int corrected, int layout, void *r_dev,
                              void *J_dev, int64_t capacity_rows, int64_t *n_invalid);
/* the same into host arrays of the batch's dtype holding capacity_rows >= offsets[count] rows (either may be NULL) */
int ea_batch_eval_rows(ea_batch *b, const double *q, const double *t, int corrected, int layout, void *r_host,
                       void *J_host, int64_t capacity_rows, int64_t *n_invalid);

/* the same for one problem (its terms included, in term order; rows = ea_problem_num_rows) */
int ea_problem_num_rows(ea_problem *p, int64_t *rows);
int ea_eval_rows(ea_problem *p, const double q[4], const double t[3], int corrected, int layout, void *r_host, void *J_host,
                 int64_t capacity_rows, int64_t *n_invalid);
int ea_eval_rows_device(ea_problem *p, const double q[4], const double t[3], int corrected, int layout, void *r_dev, void *J_dev,
                        int64_t capacity_rows, int64_t *n_invalid);

/* ---- tuning ---------------------------------------------------------------------------- */
/* tuning knobs: key in {"lds_bytes", "points_per_thread", "use_lds", "xcd_remap", "threads", "buffer_loads",
 * "solve_streams", "rows_staged", "rows_nontemporal", "wide_accumulate", "dt_f32", "poses_per_launch", "poll_results",
 * "fused_iterations", "zero_copy_poses", "starts_events", "cost_form", "poses_wave_exchange", "poses_lane_per_pose"};
 * value < 0 restores the default.
 * "poses_lane_per_pose": which calls of ea_batch_eval_poses / ea_batch_eval_resident_poses evaluate with one pose per LANE
 * (a lane owns a pose, the wavefront walks the points; no sum crosses lanes) instead of one point per lane: -1 (default) = from
 * 1024 poses on, 0 = never, N >= 1 = from N poses on.  It applies to fp64 batches of the plain functor in the flat form (one
 * term per problem, no LDS staging, no "wide_accumulate") at the pose path's 256 x 2 shape with at most 2048 partial rows per
 * pose; every other batch keeps its kernel whatever the key says.  The choice follows from the batch and K alone, never from
 * "poses_per_launch": on either path any split of the K poses over launches gives the same bits.  Between the paths the sums
 * differ in the last places (another fixed summation order); n_invalid is equal.  On this path "poses_per_launch" is rounded
 * down to a multiple of 64 (left alone below 64: launches of one partly filled group, slow).  This path folds its partial
 * rows inside the evaluation launch (runs of 16 rows in row order, then the runs in run order: a pose's sums depend on the
 * pose and the problem's point count only) and hands the results over in groups of 64 poses while the launch still runs;
 * its default item order is "poses_order" 1.  Setting the key drops resident
 * poses; ea_batch_get_info "poses_lane_per_pose" reports 1 if the last pose-batched call ran that kernel.
 * "poses_wave_exchange" = 0: the fp64 pose-batched evaluation in 256-lane workgroups (ea_batch_eval_poses, the evaluations of
 * ea_batch_solve_starts) reduces with one 32-value butterfly per wavefront; default 1: the four wavefronts of a workgroup
 * first add their sums lane by lane through LDS and each runs the butterfly over the 8 slots it is left with (another fixed
 * summation order: results agree to rounding).  Setting it drops resident poses; ea_batch_get_info "poses_wave_exchange"
 * reports what the last pose-batched launch ran (0 for fp32, 1024-lane workgroups and the forms the flat launch does not cover).
 * "starts_events" = 1 (measurement): ea_batch_solve_starts brackets the launches it queues with an event pair and waits
 * for it; ea_batch_get_info "starts_device_ns" / "starts_iterations" then report the device time and the iterations queued.
 * "dt_f32" = 0: an fp64 batch reads its fp64 images even where a float32 mirror holds them exactly (default: the mirror
 * when every term has one; results are bit-identical either way).  "poses_per_launch" = g > 0 caps the poses one
 * evaluation launch of ea_batch_eval_poses covers (default: enough to fill the chip, ~32k workgroups).  "poll_results" = 0:
 * ea_batch_eval / ea_batch_eval_poses wait for the stream's completion signal instead of returning on the flag their last
 * fold workgroup raises in pinned memory ~6 us earlier (default 1; a caller that synchronises the whole device right behind
 * the call is better off with 0: profiles/r03_ab_poll.txt).
 * "zero_copy_poses" = 0: ea_batch_eval / ea_eval always upload the pose constants before the launch (default: for up to four
 * problems the kernel reads them from the pinned host block they were written to -- one transfer less in front of a lone
 * evaluation, 26 -> 24 us per call).
 * "fused_iterations" = 0: ea_solve / ea_batch_solve always run (evaluate, step) pairs; default: a solve of problems small
 * enough for one workgroup per CU (LM strategy, one plain residual family each) runs ONE launch per iteration, every workgroup
 * taking the LM step itself before it evaluates -- the same iterates bit for bit (ea_batch_get_info "fused_iterations"
 * reports which form the last solve took; for a batch solved as sub-batches on several streams: 1 if every part ran it).
 * The launch shape is chosen with the key in view (the fused form needs 256-thread workgroups and at most 255 chunks), so
 * changing it rebuilds the batch like "threads" and "points_per_thread" do, and the sub-batches of "solve_streams" take it too.
 * "wide_accumulate" = 1: an fp32 batch sums in fp64 from a lane's sum of <= points_per_thread products on (default: a
 * lane's and a wavefront's sums are fp32, everything above fp64).  Plain functor on the L2 path; ignored for fp64
 * batches, variant functors and the LDS-staged form (ea_batch_get_info "wide_accumulate" reports what is in effect).
 * Applies to ea_batch_eval and the solves; cost: profiles/r02_ab_wide_accumulate.txt.
 * ea_batch_get_info "weighted": the number of terms of the current build that carry per-point weights (ea_problem_set_weights;
 * any such term puts the batch on the variant kernels: "starts_form" and "cost_form" then report 0). */
int ea_batch_set_tuning(ea_batch *b, const char *key, int value);
int ea_batch_get_info(const ea_batch *b, const char *key, int64_t *value);

/* ---- producers either side of the hot path, on the device ----------------
 * Reference frame: replaces get_aX (standalone/utils.cpp:201-281) + the residual-block loop at stride 1:
 * GaussianBlur 3x3 -> CV_RGB2GRAY -> Laplacian k3 -> |.| > threshold && depth > 0 -> back-projection with the
 * problem's intrinsics, points kept in raster order.  bgr: H x W x 3 bytes as cv::imread returns them,
 * depth: H x W uint16 (TUM: z_scaling 5000).  Host pointers. */
int ea_problem_set_ref_frame(ea_problem *p, const uint8_t *bgr, const uint16_t *depth, int height, int width,
                             double z_scaling, int threshold);
/* get_aX_mask (utils.cpp:283-369; call sites standalone_edge_align.cpp:1039, :1081): the same, and mask > 0
 * (mask: H x W bytes) */
int ea_problem_set_ref_frame_masked(ea_problem *p, const uint8_t *bgr, const uint8_t *mask, const uint16_t *depth,
                                    int height, int width, double z_scaling, int threshold);
/* Current frame: replaces get_distance_transform (utils.cpp:38-83) + cv2eigen + Grid2D (:201-206, :258):
 * edge map (same gradient, > threshold) -> [3x3 median] -> 3x3 chamfer DT (DIST_L2, mask 3) -> [min-max
 * normalise to [0,1]] written straight into the problem's DT image in HBM. */
int ea_problem_set_now_frame(ea_problem *p, const uint8_t *bgr, int height, int width, int threshold, int median,
                             int normalize);
/* same, and copies the intermediate stages back (any may be NULL): |Laplacian| (H*W bytes), edge mask after
 * the median (0 = edge), chamfer distance in 16.16 fixed point, final float32 DT */
int ea_problem_debug_now_frame(ea_problem *p, const uint8_t *bgr, int height, int width, int threshold, int median,
                               int normalize, uint8_t *lap_out, uint8_t *mask_out, int32_t *chamfer_fix_out,
                               float *dt_out);
/* The two producers above for EVERY problem of a batch in one launch sequence: N = ea_batch_count(b) frame pairs of equal
 * extent, the frame a grid dimension of each step -- the 12 launches of one pair (13 with depth weighting) and two waits for
 * the whole batch, where the per-problem calls cost 12-13 launches and three waits per pair.
 *
 * Each pointer array has N entries, one per problem in batch order.  ref_bgr and ref_depth are given or NULL together; NULL:
 * only the current frames are set.  now_bgr NULL: only the reference frames.  Both sides NULL is an error.
 *
 * After the call every problem p_i is in the state that
 *     ea_problem_set_ref_frame(p_i, ref_bgr[i], ref_depth[i], height, width, z_scaling, ref_threshold);
 *     ea_problem_set_now_frame(p_i, now_bgr[i], height, width, now_threshold, now_median, now_normalize);
 * leave it in, in that order, bit for bit: the same points in the same order, the same padded DT image and float32 mirror
 * (exact), the same depth weights where the problem has ea_problem_set_depth_weighting, the version bumped so that the batch
 * rebuilds its descriptors.  Each problem uses its own camera and its own depth weighting; its terms are not touched.  The one
 * difference: the frames pass through a workspace the batch owns (31.5 bytes per pixel per frame: 295 MB for 32 frames of
 * 640 x 480, kept until the batch is destroyed), and what a problem's own producer workspace holds afterwards is unspecified
 * (the tracker's short cut from the last current frame does not apply).
 *
 * EA_ERR_INVALID_ARG, checked before a device or a problem is touched (batch and problems unchanged): NULL batch or params; a
 * NULL entry in a given array; height or width outside 3..32768, more than 2^30 - 1 pixels, or with current frames a width
 * above 16384; z_scaling <= 0; the same problem twice in the batch (each pair needs a problem of its own); more than 65535
 * problems; for the _device form an entry that hipPointerGetAttributes does not report as device memory of the batch's device
 * (or a depth frame at an odd address).  EA_ERR_ALLOC: no memory for the workspace.  A failure past the checks leaves each
 * problem as the per-problem producers leave a problem on the same failure: without points when its reference step did not
 * complete, with the image of the previous frame's extent not marked exact when its current step did not.
 *
 * ea_batch_set_frames: host pointers (pinned memory, ea_host_alloc, goes up as direct DMA).  ea_batch_set_frames_device: every
 * entry a device pointer on the batch's device, read in place without a staging copy; as with the other _device setters the
 * caller's frames must be COMPLETE when the call is made (the stream that produced them synchronised: the producers run on
 * the null stream, which does not wait for non-blocking streams), and the call returns with every read of them finished. */
typedef struct {
  int height, width;      /* of every frame of the call */
  double z_scaling;       /* ea_problem_set_ref_frame's */
  int ref_threshold;      /* ea_problem_set_ref_frame's threshold (35) */
  int now_threshold, now_median, now_normalize; /* ea_problem_set_now_frame's (35, 1, 1) */
} ea_frame_params;
void ea_default_frame_params(ea_frame_params *prm, int height, int width); /* z_scaling 5000 and the values above */
int ea_batch_set_frames(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth,
                        const uint8_t *const *now_bgr, const ea_frame_params *prm);
int ea_batch_set_frames_device(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth,
                               const uint8_t *const *now_bgr, const ea_frame_params *prm);
/* Canny flavour of the two producers -- what every standalone test after edge_align_test1 uses:
 * blur 3x3 -> CV_RGB2GRAY -> Canny(low, high) (aperture 3, L1 gradient; the reference passes 30, 90).
 * Reference frame: get_aX_canny (utils.cpp:371-462): edge pixel && depth > 0 -> back-projection, raster order. */
int ea_problem_set_ref_frame_canny(ea_problem *p, const uint8_t *bgr, const uint16_t *depth, int height, int width,
                                   double z_scaling, double low_threshold, double high_threshold);
/* Current frame: get_distance_transform2 (utils.cpp:85-106), _masked (:108-141; mask: H x W bytes, edges survive where
 * mask > 1), _NoNormalize (:142-165), _masked_NoNormalize (:166-199): edges -> 3x3 chamfer DT -> [min-max normalise to
 * [norm_lo, norm_hi]: (0,1) at :103, (0,255) at :138] written into the problem's DT image.  mask may be NULL. */
int ea_problem_set_now_frame_canny(ea_problem *p, const uint8_t *bgr, const uint8_t *mask, int height, int width,
                                   double low_threshold, double high_threshold, int normalize, double norm_lo,
                                   double norm_hi);
/* same, and copies the stages back (any may be NULL): edge map (0/255), chamfer distance in 16.16 fixed point,
 * final float32 DT, number of hysteresis launches */
int ea_problem_debug_now_frame_canny(ea_problem *p, const uint8_t *bgr, const uint8_t *mask, int height, int width,
                                     double low_threshold, double high_threshold, int normalize, double norm_lo,
                                     double norm_hi, uint8_t *edges_out, int32_t *chamfer_fix_out, float *dt_out,
                                     int *hysteresis_launches);
/* The two Canny producers above for EVERY problem of a batch in one launch sequence: ea_batch_set_frames for the flavour of
 * every standalone test after edge_align_test1 and of the tracker's flavour 1.  N = ea_batch_count(b) frame pairs of equal
 * extent, the frame a grid dimension of each step.  The hysteresis converges per frame: its launches go out eight at a time
 * for all frames, each frame with change flags of its own, and the host looks at all N x 8 flags at once; a frame that has
 * reached its fixed point costs the later launches an early exit, and the call goes on when every frame has.  Per side 4
 * launches, 8 per look (one look for most frames, a second for chains that cross many 62 x 62 tiles), then 3 (reference:
 * count, scan, scatter; 4 with depth weighting) or 4 (current: the chamfer's three, the store); waits: one per look, the
 * counts, the end -- for the whole batch, where the per-problem calls cost the same launches and at least four waits per PAIR.
 *
 * The pointer arrays, the two sides and what a NULL side means are ea_batch_set_frames'.  now_mask (nullable): N masks of
 * H x W bytes for the current frames, edges survive where mask > 1; without now_bgr it is an error, and a given array has no
 * NULL entry.
 *
 * After the call every problem p_i is in the state that
 *     ea_problem_set_ref_frame_canny(p_i, ref_bgr[i], ref_depth[i], height, width, z_scaling, low_threshold, high_threshold);
 *     ea_problem_set_now_frame_canny(p_i, now_bgr[i], now_mask ? now_mask[i] : NULL, height, width, low_threshold,
 *                                    high_threshold, now_normalize, norm_lo, norm_hi);
 * leave it in, in that order, bit for bit: the same points in the same order, the same padded DT image and float32 mirror
 * (exact), the same depth weights where the problem has ea_problem_set_depth_weighting, the version bumped.  (The fixed point
 * of the hysteresis is unique, so the edge map does not depend on how many sweeps a frame was given.)  As with
 * ea_batch_set_frames the frames pass through the batch's workspace, the same one, and what a problem's own producer workspace
 * holds afterwards is unspecified: the tracker's short cut from the last current frame does not apply.
 *
 * EA_ERR_INVALID_ARG, checked before a device or a problem is touched (batch and problems unchanged): everything
 * ea_batch_set_frames checks (masks included, for the _device form too); a NaN threshold; z_scaling not finite; a
 * non-finite norm_lo or norm_hi when now_normalize is set; now_mask without now_bgr.  EA_ERR_ALLOC and a failure past the
 * checks: as for ea_batch_set_frames.  ea_batch_get_info("frames_hysteresis_rounds"): the looks at the flags the last call
 * took, both sides summed (0 after ea_batch_set_frames).
 *
 * ea_batch_set_frames_canny: host pointers.  ea_batch_set_frames_canny_device: every entry a device pointer on the batch's
 * device, read in place, complete when the call is made (see ea_batch_set_frames_device). */
typedef struct {
  int height, width;                    /* of every frame of the call */
  double z_scaling;                     /* ea_problem_set_ref_frame_canny's (5000) */
  double low_threshold, high_threshold; /* both sides (30, 90); ordered and floored as the per-problem calls do */
  int now_normalize;                    /* 1 */
  double norm_lo, norm_hi;              /* (0, 1); get_distance_transform2_masked uses (0, 255) */
} ea_canny_frame_params;
void ea_default_canny_frame_params(ea_canny_frame_params *prm, int height, int width);
int ea_batch_set_frames_canny(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth,
                              const uint8_t *const *now_bgr, const uint8_t *const *now_mask,
                              const ea_canny_frame_params *prm);
int ea_batch_set_frames_canny_device(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth,
                                     const uint8_t *const *now_bgr, const uint8_t *const *now_mask,
                                     const ea_canny_frame_params *prm);
/* ROS flavour of the two producers (src/SolveEA.cpp:29-119): cv::Canny(rgb, 150, 100, 3, true) on the 3-channel image
 * (per pixel the channel with the largest dx^2 + dy^2; squared thresholds).
 * setRefFrame (:29-82): every edge pixel gives a point; depth: H x W float32 in metres, Z == 0 -> 1.0. */
int ea_problem_set_ref_frame_ros(ea_problem *p, const uint8_t *bgr, const float *depth, int height, int width,
                                 double threshold1, double threshold2);
/* setNowFrame (:86-119): 255 - edges -> distanceTransform(DIST_L2, DIST_MASK_PRECISE) (exact Euclidean) -> normalize to
 * [0, 255].  A frame without any edge returns EA_ERR_STATE.  The debug form copies the edge map / float32 DT back. */
int ea_problem_set_now_frame_ros(ea_problem *p, const uint8_t *bgr, int height, int width, double threshold1,
                                 double threshold2);
int ea_problem_debug_now_frame_ros(ea_problem *p, const uint8_t *bgr, int height, int width, double threshold1,
                                   double threshold2, uint8_t *edges_out, float *dt_out);
/* The same two producers fed with the frames as the ROS callbacks RECEIVE them (full resolution), the node's reduction to
 * its working resolution done on the device first: `halvings` times cv::resize(src, dst, cv::Size(), 0.5, 0.5) -- the
 * 2 x 2 area mean OpenCV's linear resize is at an exact factor of two -- on the bgr8 frame and on the float32 depth frame
 * after NaN -> 0 (src/ea.cpp:38, :56-62).  full_height / full_width must be divisible by 2^halvings; the problem's
 * intrinsics are those of the working resolution (SolveEA's constructor: TUM x 0.5, src/SolveEA.cpp:15-18).  With
 * halvings = 0..L these calls build the levels of ea_solve_pyramid from one pair of full-resolution frames. */
int ea_problem_set_ref_frame_ros_scaled(ea_problem *p, const uint8_t *bgr, const float *depth, int full_height,
                                        int full_width, int halvings, double threshold1, double threshold2);
int ea_problem_set_now_frame_ros_scaled(ea_problem *p, const uint8_t *bgr, int full_height, int full_width, int halvings,
                                        double threshold1, double threshold2);
/* The two ROS producers above for EVERY problem of a batch in one launch sequence: the third sibling of ea_batch_set_frames
 * and ea_batch_set_frames_canny, in the shape the node runs -- N = ea_batch_count(b) full-resolution frame pairs of equal
 * extent, halved `halvings` times on the device, the frame a grid dimension of each step.  For halvings = 0 and one look at
 * the hysteresis flags per side: 31 launches (32 with depth weighting), 3 more per halving, and five waits (a look per side,
 * the counts of each side, the end) for the whole batch, where the per-problem calls wait six times per PAIR.
 *
 * The pointer arrays, the two sides and what a NULL side means are ea_batch_set_frames'.  ref_depth: full_height x full_width
 * float32 in metres.
 *
 * After the call every problem p_i is in the state that
 *     ea_problem_set_ref_frame_ros_scaled(p_i, ref_bgr[i], ref_depth[i], full_height, full_width, halvings, threshold1, threshold2);
 *     ea_problem_set_now_frame_ros_scaled(p_i, now_bgr[i], full_height, full_width, halvings, threshold1, threshold2);
 * leave it in, in that order, bit for bit: the same points in the same order (Z == 0 -> 1.0; NaN and negative depths kept),
 * the same padded DT image and float32 mirror (exact), the same depth weights where the problem has
 * ea_problem_set_depth_weighting, each problem's own camera, the version bumped, its terms untouched.  A reference frame
 * without edges gives a problem with zero points.  As with the other two batch calls the frames pass through the batch's
 * workspace, the same one -- here each frame's workspace at the working extent and, behind it, the stage of the halving: at
 * most 9.19 bytes per full-size pixel from host frames, 2.19 from device frames, none without halvings -- and what a problem's
 * own producer workspace holds afterwards is unspecified.
 *
 * A current frame without any edge: the per-problem producer returns EA_ERR_STATE for it and leaves the problem's image,
 * extent, exactness mark and version alone.  The batched call completes the reference side of every problem and the current
 * side of every frame that has an edge, leaves each edge-less frame's problem exactly as the per-problem call would (its image
 * is not even re-allocated: one of another extent survives), and then returns EA_ERR_STATE; ea_last_error() names the first
 * such frame's index and how many there were, ea_batch_get_info("frames_without_edges") is their number in the last ROS call
 * (0 after a clean one and after the other two batch calls).  "frames_hysteresis_rounds": as for ea_batch_set_frames_canny.
 *
 * EA_ERR_INVALID_ARG, checked before a device or a problem is touched (batch and problems unchanged): everything
 * ea_batch_set_frames checks, with its extent limits applied to the working extent (full >> halvings, at least 3 x 3; with
 * current frames no wider than 16384) and the full extent within 3..32768 and 2^30 - 1 pixels; halvings outside 0..8 or a
 * full extent not divisible by 2^halvings; a NaN threshold; for the _device form a depth frame that is not device memory of
 * the batch's device or not 4-byte aligned.  EA_ERR_ALLOC and a failure past the checks: as for ea_batch_set_frames.
 *
 * ea_batch_set_frames_ros: host pointers.  ea_batch_set_frames_ros_device: every entry a device pointer on the batch's device,
 * read in place (by the first halving step, or by the producers themselves without halvings), complete when the call is made
 * (see ea_batch_set_frames_device). */
typedef struct {
  int full_height, full_width;   /* of every frame as handed in */
  int halvings;                  /* 0..8; the producers work at full >> halvings */
  double threshold1, threshold2; /* cv::Canny(rgb, 150, 100, 3, true): (150, 100) */
} ea_ros_frame_params;
void ea_default_ros_frame_params(ea_ros_frame_params *prm, int full_height, int full_width); /* halvings 0 */
int ea_batch_set_frames_ros(ea_batch *b, const uint8_t *const *ref_bgr, const float *const *ref_depth,
                            const uint8_t *const *now_bgr, const ea_ros_frame_params *prm);
int ea_batch_set_frames_ros_device(ea_batch *b, const uint8_t *const *ref_bgr, const float *const *ref_depth,
                                   const uint8_t *const *now_bgr, const ea_ros_frame_params *prm);
/* ---- the batched ROS producers over pyramid levels: N frame pairs, L levels, frames handed in once ----------------------
 * levels[l] is a batch of the same N problems' level-l counterparts (levels[0] the finest, working extent full >>
 * (prm->halvings + l); cameras are the caller's, scaled per level as for ea_solve_pyramid).  One call leaves EVERY levels[l],
 * bit for bit, in the state
 *     ea_batch_set_frames_ros(levels[l], ref_bgr, ref_depth, now_bgr, &prm_l),   prm_l.halvings = prm->halvings + l
 * leaves it in -- points and their order, padded images and float32 mirrors, depth weights, cameras untouched, versions, terms
 * -- while each side's frames go up ONCE (not at all for device frames) and one halving chain per side and kind produces all
 * levels from one read of the full-size frames: a workgroup stages a tile in LDS, halves it up to three times there and
 * writes each kept level straight into that level's frame workspace; the first prm->halvings - 1 steps never reach memory.
 * The arithmetic is ea_resize_half's step by step (colour rounded to uint8 at every level, NaN -> 0 on the first step from the
 * full-size depth frame only; with halvings = 0 level 0 of a host frame is the uploaded frame as it is).  Behind the chain
 * every level runs the launches and waits of ea_batch_set_frames_ros; the reference side of all levels is complete before the
 * current side reuses the stage.  All frames pass through the workspace of levels[0]: frame_pyramid (ea_frame_ws.h).
 *
 * A current frame without an edge at some level leaves that level's problem alone, as ea_batch_set_frames_ros does; the call
 * completes everything else and returns EA_ERR_STATE naming the first (level, frame); "frames_without_edges" on each level's
 * batch is that level's number.  ea_batch_get_info(levels[0], "frames_uploaded"): the host-to-device frame copies of the last
 * pyramid call -- 3 N for a host call with both sides whatever nlevels is, 0 for device frames.
 *
 * EA_ERR_INVALID_ARG before anything is touched: everything ea_batch_set_frames_ros checks, on every level; nlevels < 1 or
 * halvings + nlevels - 1 > 8; a full extent not divisible by 2^(halvings + nlevels - 1); a coarsest extent below 3 x 3;
 * batches of different counts, devices or dtypes; a problem appearing twice across the levels.
 *
 * ea_batch_solve_pyramid is ea_solve_pyramid for every problem: one ea_batch_solve per level, the coarsest first, the poses
 * (q: count x 4, t: count x 3) carried down.  A problem whose level ends in EA_FAILURE stops descending: its finer summaries
 * are zeroed and its pose is what that level returned; the others go on, and get the bits of a loop of ea_batch_solve over
 * the levels (a stopped problem rides along in the finer solves and its results are discarded; a finer counterpart with an
 * auto-scaled loss has that scale re-estimated, nothing else of it changes).  A level's non-OK return is returned as is.
 * summaries: nlevels x count, level-major, or NULL. */
int ea_batch_set_frames_ros_pyramid(ea_batch *const *levels, int nlevels, const uint8_t *const *ref_bgr,
                                    const float *const *ref_depth, const uint8_t *const *now_bgr, const ea_ros_frame_params *prm);
int ea_batch_set_frames_ros_pyramid_device(ea_batch *const *levels, int nlevels, const uint8_t *const *ref_bgr,
                                           const float *const *ref_depth, const uint8_t *const *now_bgr,
                                           const ea_ros_frame_params *prm);
int ea_batch_solve_pyramid(ea_batch *const *levels, int nlevels, const ea_options *opt, double *q, double *t,
                           ea_summary *summaries);

/* ---- multi-stream frame tracker: N cameras pushed in lock-step ---------------------------------------------------------
 * ea_tracker for `count` independent streams of one extent (N cameras; BASELINE configuration C4's 32 pairs per GPU): every
 * push takes one frame per stream, runs the batched producers ONCE per frame -- the frame a grid dimension of each launch,
 * its edge strength / edge map serving first as the current side (chamfer or exact transform into the stream's image) and
 * then as the next reference (count, scan, scatter, depth weights) -- and solves all aligned streams in one ea_batch_solve.
 * The tracker owns its problems, one ea_batch over them (and with it the batch's frame workspace) and per stream the state
 * ea_tracker keeps: frame count, last relative pose, installed prior, covariance.
 *
 * flavour 0 (Laplacian: threshold 35, median on, normalised) and 1 (Canny 30 / 90, range [0, 1]) are ea_tracker's; depth is
 * uint16.  flavour 2 is the ROS node's chain (SolveEA::setRefFrame / setNowFrame, cv::Canny(150, 100), the exact transform
 * normalised to [0, 255]): depth is float32 in metres at the extent handed in, z_scaling is ignored, and the chain works at
 * (height, width) >> halvings -- the cameras belong to that working resolution, as with ea_problem_set_*_frame_ros_scaled.
 *
 * Per stream the semantics are ea_tracker_push_frame's.  A stream is ALIGNED in a push when it has had a frame
 * before, its reference has more than 0 points and (flavour 2) the new frame has at least one edge; it is then solved from
 * its last relative pose, with the motion prior centred there if one is set, the problem's own camera, loss, auto-scaled
 * loss, depth weighting and constant mask (ea_tracker_batch_problem).  A solve that ends in EA_FAILURE keeps the prior
 * (aligned[i] is still 1).  Aligned streams whose problems run one kernel family -- the usual case: the same settings for
 * all -- are solved by ONE ea_batch_solve; a stream with per-point weights (depth weighting), distortion or a second camera
 * among plain ones would put those on the variant kernels, whose sums agree with the plain kernels' to rounding only, so
 * such families are solved one after the other, each stream by the kernels, and to the bits, of a tracker of its own.
 * (What a stream gets is what ea_batch_solve gives its problem among those streams.  That is the lone tracker's result to the
 * bit while the batch resolves to a lone problem's launch shape -- below 80000 points in all for fp64; a larger batch takes
 * a throughput shape, two points per lane, and agrees with the lone tracker to rounding: 1e-16 on the poses of 32 VGA
 * streams, profiles/tracker_batch_ab.txt.  Points, depth weights and images are the lone tracker's bits at every size.)
 * A stream that is not aligned takes no part in any solve, returns its unchanged prior in q_rel / t_rel, a zeroed summary and aligned[i] = 0.  Then the frame's edge
 * points become the stream's reference.  A flavour-2 frame without any edge is a result, not an error: the stream is not
 * aligned, its image is left alone, its new reference has zero points (so the next push does not align it either) and the
 * push returns EA_OK; ea_tracker_batch_get_info("frames_without_edges") counts such frames of the last push.
 *
 * q_rel: count x 4, t_rel: count x 3; summaries, aligned: count entries or NULL.  bgr / depth: count frame pointers --
 * host memory (pinned memory, ea_host_alloc, goes up as direct DMA), or for the _device form device memory of the tracker's
 * device, read in place and complete when the call is made (see ea_batch_set_frames_device).
 *
 * EA_ERR_INVALID_ARG, before a device or a stream is touched (the tracker stays exactly as it was): a NULL array or entry;
 * an extent outside the batched producers' limits at the working extent (3..32768, at most 2^30 - 1 pixels, no wider than
 * 16384); an extent not divisible by 2^halvings; z_scaling <= 0 (flavours 0, 1); for the _device form a frame that is not
 * device memory of the tracker's device.  ea_tracker_batch_create: count outside 1..65535, an unknown flavour, halvings
 * outside 0..8 or != 0 with flavours 0 and 1.
 * A failure PAST the checks (a HIP error, no memory, a failed solve call) resets EVERY stream -- no reference, frame count 0,
 * the prior kept -- so that the next push starts fresh chains instead of aligning against frames of different pushes.
 *
 * ea_tracker_batch_reset(i): stream i forgets its reference and its prior (i < 0: every stream).  set_covariance,
 * last_covariance(i), set_motion_prior: ea_tracker's, for every stream (why = 4 after a failed solve; EA_ERR_STATE when
 * stream i was not aligned in the last push).  get_info keys: "aligned" (streams solved in the last push),
 * "frames_without_edges", "hysteresis_rounds" (looks at the hysteresis flags, 0 for flavour 0), "edge_passes" (N-frame
 * edge-detection chains the last push ran: 1, whether streams were aligned or not -- the shared frame), "frames" (pushes
 * since creation that passed the checks). */
typedef struct ea_tracker_batch ea_tracker_batch;
int ea_tracker_batch_create(ea_tracker_batch **out, const ea_camera *cams, int count, int dtype, int device, int flavour,
                            int halvings);
void ea_tracker_batch_destroy(ea_tracker_batch *tb);
int ea_tracker_batch_count(const ea_tracker_batch *tb);
ea_problem *ea_tracker_batch_problem(ea_tracker_batch *tb, int i); /* stream i's problem (loss, auto-scale, depth weighting, constant mask, flavour knobs) */
int ea_tracker_batch_push_frames(ea_tracker_batch *tb, const uint8_t *const *bgr, const void *const *depth, int height,
                                 int width, double z_scaling, const ea_options *opt, double *q_rel, double *t_rel,
                                 ea_summary *summaries, int *aligned);
int ea_tracker_batch_push_frames_device(ea_tracker_batch *tb, const uint8_t *const *bgr, const void *const *depth, int height,
                                        int width, double z_scaling, const ea_options *opt, double *q_rel, double *t_rel,
                                        ea_summary *summaries, int *aligned);
int ea_tracker_batch_reset(ea_tracker_batch *tb, int i);
int ea_tracker_batch_set_covariance(ea_tracker_batch *tb, const ea_covariance_options *o);
int ea_tracker_batch_last_covariance(ea_tracker_batch *tb, int i, ea_covariance *out);
int ea_tracker_batch_set_motion_prior(ea_tracker_batch *tb, double sigma_rot, double sigma_trans);
int ea_tracker_batch_get_info(const ea_tracker_batch *tb, const char *key, int64_t *value);
/* Coarse-to-fine multi-stream tracking (flavour 2 only): `levels` pyramid levels per stream, level l working at (height,
 * width) >> (halvings + l).  cams: levels x count, level-major, each the caller's intrinsics at that level's working extent.
 * ea_tracker_batch_create(..., halvings) is levels = 1; the push calls keep their signatures.  Per push the frames go up once,
 * one halving chain produces every level (ea_batch_set_frames_ros_pyramid), and on every level the frame passes the edge
 * detection once and serves both sides: "edge_passes" is `levels`; "levels" is a key of its own; "frames_without_edges" and
 * the ALIGNED rule are level 0's.  A coarser level is usable for a stream when that level's reference has points and that
 * level's frame has an edge.  An aligned stream's result is ea_solve_pyramid over its usable levels, coarsest first, from its
 * last relative pose: the motion prior, if set, is installed on every usable level's problem at that pose; a level ending in
 * EA_FAILURE stops the descent and the stream keeps its prior; the covariance is level 0's at the returned pose; summaries[i]
 * is the summary of the finest level the descent reached, ea_tracker_batch_last_summaries(i) gives all `levels` of them (level
 * 0 first, zeros for levels not solved; with levels = 1 the one summary of the push).  On each level the streams to solve are
 * grouped by kernel family and solved through that level's (sub-)batches; afterwards every level's edge points become that
 * level's reference.  Reset and a failure past the checks drop every level.  Loss, auto-scale, depth weighting and constant
 * masks are whatever the caller sets on each level's problem (ea_tracker_batch_level_problem; level 0 ==
 * ea_tracker_batch_problem).  EA_ERR_INVALID_ARG from the push as before, with the extent divisible by 2^(halvings + levels - 1)
 * and the coarsest level at least 3 x 3; from create_pyramid for levels < 1 or halvings + levels - 1 > 8. */
int ea_tracker_batch_create_pyramid(ea_tracker_batch **out, const ea_camera *cams, int count, int levels, int dtype, int device,
                                    int halvings);
ea_problem *ea_tracker_batch_level_problem(ea_tracker_batch *tb, int level, int i);
int ea_tracker_batch_last_summaries(ea_tracker_batch *tb, int i, ea_summary *out /* levels entries */);

/* Keyframe mode of the multi-stream tracker: a stream's reference is HELD while enough of it is still seen, instead of being
 * replaced by every pushed frame.  Off by default: a tracker on which it is never switched on runs the frame-to-frame push.
 *   set_keyframes(p): accepted only while no stream holds a reference (before the first push, or after
 *     ea_tracker_batch_reset(-1)), else EA_ERR_STATE; EA_ERR_STATE with levels > 1 (keyframes across pyramid levels are out
 *     of scope); a NaN field, margin < 0 or inlier_residual < 0: EA_ERR_INVALID_ARG; p == NULL: back to frame-to-frame.  All three flavours,
 *     halvings included, host and device frames.
 *   Current side: unchanged -- every pushed frame passes the edge detection once and its transform lands in every stream's
 *     image.
 *   Alignment: a stream is aligned by the frame-to-frame rule and solved from its stored pose, which is the pose of the
 *     KEYFRAME in the previous frame's coordinates (zero-velocity start); the motion prior is centred there, the covariance is
 *     taken as before.
 *   Statistics: after the solves, ea_batch_pose_stats at the returned poses on the (sub-)batches that solved, one call per
 *     solved group, for the streams whose solve did not end in EA_FAILURE, before anything overwrites points.
 *   Decision (csrc/ea_keyframe.h, keyframe_decide): the comparisons written beside ea_keyframe_params' fields, each with one
 *     IEEE multiplication; a stream that was not aligned: EA_KEY_FIRST; a failed solve: EA_KEY_SOLVE_FAILED; several bits may
 *     be set.
 *   A replaced stream takes the pushed frame's edge points as its reference (scatter, depth weights), age = 0,
 *     keyframe_push = get_info("frames"), and its stored pose becomes the identity.  A kept stream's point, weight and
 *     point-order arrays are not touched; age += 1 and its stored pose becomes the solved pose.  When no stream replaces, no
 *     scatter and no depth-weight launch is issued.
 *   q_rel / t_rel of an aligned stream: the pose solved in this push against the keyframe in use DURING this push, also when
 *     the push then replaces it (callers chain poses themselves); a failed solve returns the pose it started from, an
 *     unaligned stream the identity.
 *   Flavour 2, a frame without any edge: the stream is not aligned, its image is left alone and it KEEPS the keyframe it has
 *     (replaced = 0, age unchanged); if it holds none it stays without one.
 *   A failure past the checks resets every stream; reset(i) also clears stream i's keyframe state.
 *   get_info: "keyframes_taken" (streams that replaced in the last push), "keyframe_mode" (0 / 1).
 * Out of scope: the single ea_tracker (a tracker batch of one stream is its keyframe form), pyramid levels, composing poses
 * along the keyframe chain into a world pose, a constant-velocity start after a replacement.  The default
 * min_visible_fraction of 0.75 is an untuned starting value. */
typedef struct {
  double min_visible_fraction;  /* replace when (double)n_visible < min_visible_fraction * (double)n;  <= 0: off */
  double min_inlier_fraction;   /* replace when (double)n_inlier  < min_inlier_fraction  * (double)n;  <= 0: off */
  double inlier_residual;       /* in the units of the stream's DT ([0,1] for flavours 0/1, [0,255] for flavour 2) */
  double max_mean_flow;         /* replace when n_flow > 0 and sum_flow > max_mean_flow * (double)n_flow;  <= 0: off */
  int max_frames;               /* replace when this many frames have been solved against the keyframe;   <= 0: off */
  int margin;
} ea_keyframe_params;
enum { EA_KEY_FIRST = 1, EA_KEY_SOLVE_FAILED = 2, EA_KEY_VISIBLE = 4, EA_KEY_INLIERS = 8, EA_KEY_FLOW = 16, EA_KEY_AGE = 32 };
typedef struct {
  int64_t keyframe_push;  /* value of get_info("frames") at the push that delivered the keyframe now held; 0: none */
  int age;                /* frames solved against it so far */
  int replaced;           /* reason mask of the last push, 0 = the keyframe was kept */
  ea_pose_stats stats;    /* at the pose the last push returned; zeros when the stream was not aligned or its solve failed */
} ea_keyframe_state;
void ea_default_keyframe_params(ea_keyframe_params *p);   /* min_visible_fraction 0.75, everything else off */
int ea_tracker_batch_set_keyframes(ea_tracker_batch *tb, const ea_keyframe_params *p);
int ea_tracker_batch_keyframe_state(ea_tracker_batch *tb, int i, ea_keyframe_state *out);

/* The depth gate inside the multi-stream tracker: every solve of a push is preceded by ea_batch_depth_gate's arithmetic on the
 * streams it solves, against the depth frame of THIS push.  Off by default: a tracker on which it is never set issues exactly
 * the launches it issued before.
 *   set_depth_gate(prm): prm == NULL: off.  Accepted only while no stream holds a reference (before the first push or after
 *     ea_tracker_batch_reset(-1)), else EA_ERR_STATE -- the rule of ea_tracker_batch_set_keyframes.  Parameter errors are
 *     ea_batch_depth_gate's (EA_ERR_INVALID_ARG), found before the handle is looked at; a factor that overflows the float of
 *     an fp32 tracker likewise.  All flavours, halvings, pyramid levels and keyframe mode, host and device frames.
 *   Which depth: flavours 0 and 1 the pushed uint16 frame with the push's z_scaling, s = 0; flavour 2 the pushed float32 frame
 *     at FULL resolution, s = halvings + level (step 3b above: the level's own depth is the reference's reduction and no gate
 *     input).  It is read where the push has put it already -- the caller's device frame in place; of a host frame the
 *     workspace's `depth` region or the halving stage's full-size region, which the upload alone writes -- no second upload,
 *     no copy.
 *   When: behind the priors, inside the descent, on every level directly in front of that level's solve, for the streams that
 *     solve on that level, at the pose they carry into it -- on the coarsest usable level the start pose, below it the pose
 *     the level above returned -- with M = ea_pose_to_matrix(q, t).  It runs on the (sub-)batch that solves the group and on
 *     its stream: one launch and one wait of its own per solved (level, group).
 *   apply != 0: w = g * dd replaces the weights of each gated level problem before its solve (dd: the problem's depth
 *     weighting, or 1).  Every stream of such a tracker is a WEIGHTED problem from its first reference on -- the reference
 *     scatter leaves a new reference with weights dd, or exactly 1.0 without depth weighting -- so streams with otherwise
 *     equal settings stay one kernel family, a problem never flips between weighted and unweighted from push to push, and
 *     ea_tracker_batch_problem(i) may be evaluated between pushes.  A kept keyframe is gated again every push from its own
 *     z: nothing accumulates.  The covariance sees the gated weights; pose statistics ignore weights, as documented.
 *   apply == 0: counts only; poses, summaries, points, images, covariance and keyframe decisions are bit for bit those of a
 *     tracker without a gate.
 *   Not gated: streams that are not aligned, and levels that are not usable for a stream or that its descent did not reach;
 *     their counts are zero (n = 0).
 *   last_depth_gate(level, i): the counts of stream i on `level` in the last push.  get_info: "depth_gate" (0 / 1), "gated"
 *     (the (stream, level) pairs gated in the last push).  A rejected push leaves both as they were; a failure past the checks
 *     resets every stream, as in every phase.
 * Out of scope: the single ea_tracker, a keyframe rule on the occlusion counts, soft or continuous weights, depth as a
 * residual, gating of terms, overlapping the uploads with the solve.  The default tolerances remain API defaults that nobody
 * has measured on real sequences. */
int ea_tracker_batch_set_depth_gate(ea_tracker_batch *tb, const ea_depth_gate_params *prm);
int ea_tracker_batch_last_depth_gate(ea_tracker_batch *tb, int level, int i, ea_depth_gate_stats *out);

/* Point selection inside the multi-stream tracker: every new reference is thinned by ea_batch_select_points' rule before it is
 * first solved against.  Off by default: a tracker on which it is never set issues no launch, wait or copy more than before.
 *   set_point_selection(prm): prm == NULL: off.  May be set at any time; it acts on the references taken from then on.
 *     Parameter errors are ea_batch_select_points' (EA_ERR_INVALID_ARG, found before the handle is looked at); prm->height and
 *     prm->width must be 0 -- each level uses the extent of its own DT image, and cell_px is in that level's pixels.
 *   Where: in every push, directly after a level's references have landed (scatter, then depth weights), over the streams
 *     that TOOK a new reference on that level, on that level's batch: one ea_batch_select_points launch sequence and one wait
 *     per level.  A kept keyframe's points are not touched.  With a depth gate, the gate's weights are written before the
 *     NEXT push's solve: they see the selected points.  A push equals, bit for bit, the batched producer followed by
 *     ea_batch_select_points and ea_batch_solve by hand.
 *   last_point_selection(stats, capacity): levels x streams rows, level-major (capacity >= that many).  The row of a (level,
 *     stream) holds the stats of the push that last selected that reference: a kept keyframe keeps its row; a reset or a
 *     stream without a reference reports zeros.  get_info("selected"): the streams thinned by the last push (on every
 *     level); get_info("point_selection"): 0 / 1. */
int ea_tracker_batch_set_point_selection(ea_tracker_batch *tb, const ea_point_selection *prm /* NULL: off */);
int ea_tracker_batch_last_point_selection(const ea_tracker_batch *tb, ea_point_selection_stats *stats, int capacity);

/* Points carried across a keyframe replacement.  In keyframe mode a replaced reference is only the pushed frame's own edge
 * points: an edge pixel of that frame without a depth reading is lost (flavours 0 and 1; in flavour 2 it carries the fake depth
 * 1.0), though the old keyframe may have held a 3-D point for that edge.  With a carry set, the old keyframe's points are moved
 * into the new frame by the pose the push solved and merged behind the new reference by ea_batch_merge_points' rule.  Off by
 * default: a tracker on which it is never set issues no launch, wait or copy more than before.
 *   set_point_carry(prm): prm == NULL: off.  Keyframe mode only (EA_ERR_STATE otherwise; so: a single level), all three
 *     flavours, host and device frames; and, as ea_tracker_batch_set_keyframes, only while no stream holds a reference
 *     (EA_ERR_STATE).  Parameter errors are ea_batch_merge_points' (EA_ERR_INVALID_ARG, found before the handle is looked at);
 *     prm->height and prm->width must be 0: a stream uses the extent of its own DT image -- the new frame's, which the push has
 *     already put in place.
 *   Where: a stream CARRIES in a push when it replaces its keyframe and its solve did not fail (the reason mask holds neither
 *     EA_KEY_FIRST nor EA_KEY_SOLVE_FAILED).  Its old point arrays are detached -- moved, not copied -- before the new
 *     reference takes room; after the new references have landed (scatter, depth weights, the depth gate's ones) ONE merge call
 *     runs over the carrying streams: src the detached arrays, dst_T_src the matrix ea_pose_to_matrix gives for the pose this
 *     push solved (the q_rel, t_rel it returns).  Then point selection, when set: a `target` caps the merged reference.  A kept
 *     keyframe, a first keyframe and a failed solve launch nothing.  A push equals, bit for bit, the batched producer followed
 *     by ea_batch_merge_points (and ea_batch_select_points) and ea_batch_solve by hand.  The carried weights follow the merge's
 *     rule.  Flavour 2's fake-depth points occupy cells like any other point.  A push that fails past its checks resets every
 *     stream as before; the detached arrays are freed either way.
 *   last_point_carry(stats, capacity): one row per stream (capacity >= streams): the merge of the last push, zeros for a stream
 *     that did not carry in it.  get_info("carried"): the streams that carried in the last push; get_info("point_carry"): 0 / 1.
 * Out of scope: pyramid levels, the single ea_tracker, per-point age or observation counts, depth fusion. */
int ea_tracker_batch_set_point_carry(ea_tracker_batch *tb, const ea_point_merge *prm /* NULL: off */);
int ea_tracker_batch_last_point_carry(const ea_tracker_batch *tb, ea_point_merge_stats *stats, int capacity);

/* the half-resolution step by itself, host in / host out: kind 0 = bgr8 (height x width x 3 bytes), 1 = float32 with
 * NaN -> 0 first, 2 = float32 as is; dst = (height / 2) x (width / 2); height and width even */
int ea_resize_half(int device, int kind, const void *src, int height, int width, void *dst);
/* levels skip .. skip + keep - 1 of the halving chain of one frame (level k = k halvings) from one upload and one read of the
 * frame per three steps; kind as ea_resize_half; dst[j]: (height >> (skip + j)) x (width >> (skip + j)); height, width
 * divisible by 2^(skip + keep - 1), at most 8 steps.  skip = 0 returns the frame itself as level 0; kind 1 replaces NaN on
 * the first step only, so from level 1 on.  Every level holds the bits of ea_resize_half applied that many times. */
int ea_resize_half_levels(int device, int kind, const void *src, int height, int width, int skip, int keep, void *const *dst);
/* read back what the problem holds in HBM: points (n x 3 doubles), DT image (H x W doubles, [v][u]) */
int ea_problem_get_points(ea_problem *p, double *xyz, int64_t capacity);
int ea_problem_get_dt(ea_problem *p, double *image, int *height, int *width);

/* Self-test of the wavefront reduction primitives the kernels rely on (write-masked DPP adds,
 * v_permlane16/32_swap, quad_perm): in = 32 slots x 64 lanes (fp32, slot-major); out32 / out64 = the 32
 * wave totals from the fp32 and the fp64 reduction; stages (nullable, 30 x 64 floats) = the
 * intermediate levels of the fp32 reduction. */
int ea_selftest_wave_reduce(int device, const float *in, double *out32, double *out64, float *stages);
/* Self-test of the select kernels behind ea_*_residual_quantiles, on caller-supplied values: values = host doubles, segment s
 * = [offsets[s], offsets[s+1]) (nseg + 1 offsets); NaN = a failed block, everything else enters by absolute value (+Inf is
 * valid); out: nseg x nq, n_valid: nseg or NULL. */
int ea_selftest_select(int device, const double *values, const int64_t *offsets, int nseg, const double *probs, int nq,
                       double *out, int64_t *n_valid);

#ifdef __cplusplus
}
#endif
#endif /* EA_HIP_H */
