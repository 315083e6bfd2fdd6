// ea_segments.hip — the host side of the calls that run one launch over "one segment per problem of the call: the head
// family of that problem": residual quantiles and the auto-scaled losses, pose visibility statistics, reproject, overlay and
// the depth-consistency gate (with the current-frame depth it reads), point selection and the transform and merge of point
// sets.  Host code only: this file holds no kernel, and it sees
// a batch through the functions and the read-only BatchView of ea_capi_internal.h; ea_batch's layout stays ea_capi.hip's.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ea_hip.h"
#include "ea_capi_internal.h"
#include "ea_launch.h"
#include "ea_types.h"

using namespace ea;

// ---- the scaffold the four drivers share ------------------------------------------------------------------------------------
//
// A call fills one record per problem (SelectSeg, ReprojectSeg, DepthGateSeg: the kernels' layouts) in a pinned block, sends
// it up in ONE copy, launches over the segments on the batch's stream, and gets its results back behind the records of the
// same block; the caller queues what else must come down and synchronises ONCE.

// a launch takes one segment per problem in grid y
static int check_segment_count(size_t nseg, const char *call) {
  if (nseg > 65535) return fail(EA_ERR_INVALID_ARG, std::string("more than 65535 problems in one ") + call + " call");
  return EA_OK;
}

namespace {
// The head family of problem j of a call over a built batch -- problem sel[j] of the batch, or j without a selection: its
// term, its rows in the batch's layout and its problem.  max_n: the longest family handed out so far.
struct HeadFamily { int term; int64_t row_begin; int32_t n; const ea_problem *problem; };
struct HeadFamilies {
  const BatchView &v;
  const int *sel = nullptr;
  int max_n = 0;
  HeadFamily operator()(int j) {
    const int i = sel ? sel[j] : j;
    const int term = v.h_groups[i].term_begin;  // the head family; its terms are not included
    max_n = std::max(max_n, (int)v.h_desc[term].n);
    return HeadFamily{term, v.h_desc[term].row_begin, v.h_desc[term].n, v.probs[i]};
  }
};

// The block of a call twice, in pinned memory and on the device, laid out alike: [records | results], the results 16-aligned
// behind the records.  up() copies the upload prefix [0, up_bytes) to the device -- records and zeroed results, unless the
// caller shortens it -- and down() the download suffix, the down_bytes of results, back.  take_*: cached blocks that return
// to the cache with the call; the depth gate sets `pinned` and `dev` to the batch's own pair instead and clears `cached`.
struct SegmentBlock {
  unsigned char *pinned = nullptr, *dev = nullptr;
  size_t o_results = 0, up_bytes = 0, down_bytes = 0;
  bool cached = true;
  ~SegmentBlock() { if (cached) { cached_host_free(pinned); cached_free(dev); } }
  size_t layout(size_t record_bytes, size_t result_bytes) {  // (returns the size of both parts)
    o_results = align16(record_bytes); down_bytes = result_bytes;
    return up_bytes = o_results + result_bytes;
  }
  hipError_t take_pinned(size_t bytes, int device) {
    return cached_host_malloc(reinterpret_cast<void **>(&pinned), bytes, hipHostMallocDefault, device);
  }
  hipError_t take_device(size_t bytes, int device) { return cached_malloc(reinterpret_cast<void **>(&dev), bytes, device); }
  template <typename T> T *records() const { return reinterpret_cast<T *>(pinned); }
  template <typename T> const T *results() const { return reinterpret_cast<const T *>(pinned + o_results); }
  template <typename T> const T *dev_records() const { return reinterpret_cast<const T *>(dev); }
  template <typename T> T *dev_results() const { return reinterpret_cast<T *>(dev + o_results); }
  hipError_t up(hipStream_t stream) const { return hipMemcpyAsync(dev, pinned, up_bytes, hipMemcpyHostToDevice, stream); }
  hipError_t down(hipStream_t stream) const {
    return hipMemcpyAsync(pinned + o_results, dev + o_results, down_bytes, hipMemcpyDeviceToHost, stream);
  }
};
}  // namespace

// is this caller pointer device memory of this device, as far as the runtime can tell?  A pointer the runtime does not know
// is refused (check_device_pointer is the form that takes those on trust)
static bool device_memory_of(const void *ptr, int device) {
  hipPointerAttribute_t at;
  const hipError_t e = hipPointerGetAttributes(&at, ptr);
  if (e != hipSuccess) (void)hipGetLastError();
  return e == hipSuccess && at.type == hipMemoryTypeDevice && at.device == device;
}

// the 3x4 matrix of step A for one problem of a call: b_T_a, through the rig where the problem has a second camera
static void segment_matrix(const ea_problem *p, const double *b_T_a, double M[12]) {
  const bool rig = (p->variant & 2) != 0;
  reproject_matrix(b_T_a, rig ? p->T12 : nullptr, rig ? p->T12inv : nullptr, M);
}

// rows of elem_bytes each in the batch's layout: the head families' rows come down, adjacent ones in one copy; rows of terms
// stay as the caller left them
static int download_head_rows(const BatchView &v, size_t elem_bytes, const void *dev, void *host) {
  HeadFamilies heads{v};
  for (int j = 0; j < v.count;) {
    const int64_t begin = heads(j).row_begin;
    int64_t end = begin + heads(j).n;
    for (++j; j < v.count && heads(j).row_begin == end; ++j) end += heads(j).n;
    if (end > begin)
      HIPCHK(hipMemcpyAsync(static_cast<unsigned char *>(host) + (size_t)begin * elem_bytes,
                            static_cast<const unsigned char *>(dev) + (size_t)begin * elem_bytes, (size_t)(end - begin) * elem_bytes,
                            hipMemcpyDeviceToHost, v.stream));
  }
  return EA_OK;
}

// ---- exact order statistics of |r| (ea_select.h; kernels: ea_select_*_kernel) ------------------------------------------
//
// One launch sequence per call, whatever the number of problems: clear, key pass, six (histogram, scan) pairs -- 14 launches --
// on the batch's stream, the bin choice staying on the device between the passes; segments and probabilities go up, values and
// valid counts come back through one pinned block, ONE synchronisation at the end.
namespace {
struct SelectBuffers {
  SegmentBlock blk;                   // pinned: [segs | probs || values | n_valid]; the device block starts alike
  SelectWork w;
  double *d_input = nullptr;          // ea_selftest_select: the caller's values
  SelectSeg *h_segs = nullptr;
  double *h_probs = nullptr, *h_values = nullptr;
  int64_t *h_n_valid = nullptr;
};
}  // namespace

static int select_reserve(SelectBuffers &s, int device, int nseg, int nq, int64_t total_keys, bool with_input) {
  const size_t sq = (size_t)nseg * nq;
  const size_t o_segs = 0, o_probs = o_segs + align16((size_t)nseg * sizeof(SelectSeg)), o_vals = o_probs + align16((size_t)nq * 8);
  const size_t o_nv64 = o_vals + align16(sq * 8), o_prefix = o_nv64 + align16((size_t)nseg * 8), o_rank = o_prefix + align16(sq * 8);
  const size_t o_nvalid = o_rank + align16(sq * 8), o_hist = o_nvalid + align16((size_t)nseg * 4);
  const size_t o_keys = o_hist + sq * kSelectBins * sizeof(unsigned), o_input = o_keys + align16((size_t)total_keys * 8);
  const size_t bytes = o_input + (with_input ? align16((size_t)total_keys * 8) : 0);
  HIPCHK(s.blk.take_device(bytes, device));
  HIPCHK(s.blk.take_pinned(o_prefix, device));
  unsigned char *d = s.blk.dev, *h = s.blk.pinned;
  s.blk.o_results = s.blk.up_bytes = o_vals; s.blk.down_bytes = o_prefix - o_vals;
  s.h_segs = reinterpret_cast<SelectSeg *>(h + o_segs);
  s.h_probs = reinterpret_cast<double *>(h + o_probs);
  s.h_values = reinterpret_cast<double *>(h + o_vals);
  s.h_n_valid = reinterpret_cast<int64_t *>(h + o_nv64);
  SelectWork &w = s.w;
  w.nseg = nseg; w.nq = nq;
  w.segs = reinterpret_cast<const SelectSeg *>(d + o_segs);
  w.probs = reinterpret_cast<const double *>(d + o_probs);
  w.out_values = reinterpret_cast<double *>(d + o_vals);
  w.out_n_valid = reinterpret_cast<int64_t *>(d + o_nv64);
  w.prefix = reinterpret_cast<uint64_t *>(d + o_prefix);
  w.rank = reinterpret_cast<int64_t *>(d + o_rank);
  w.n_valid = reinterpret_cast<unsigned *>(d + o_nvalid);
  w.hist = reinterpret_cast<unsigned *>(d + o_hist);
  w.clear_bytes = o_keys - o_nvalid;
  w.keys = reinterpret_cast<uint64_t *>(d + o_keys);
  s.d_input = with_input ? reinterpret_cast<double *>(d + o_input) : nullptr;
  return EA_OK;
}

// segments and probabilities up, the counts cleared: what comes before either key pass
static int select_begin(SelectBuffers &s, const double *probs, hipStream_t stream) {
  int max_n = 0;
  for (int i = 0; i < s.w.nseg; ++i) max_n = std::max(max_n, (int)s.h_segs[i].n);
  s.w.max_n = max_n;
  for (int i = 0; i < s.w.nq; ++i) s.h_probs[i] = probs[i];
  HIPCHK(s.blk.up(stream));
  HIPCHK(launch_select_clear(s.w, stream));
  return EA_OK;
}

// the six passes, the results down, the call's one synchronisation
static int select_finish(SelectBuffers &s, hipStream_t stream, double *values, int64_t *n_valid) {
  HIPCHK(launch_select(s.w, stream));
  HIPCHK(s.blk.down(stream));
  HIPCHK(hipStreamSynchronize(stream));
  std::memcpy(values, s.h_values, (size_t)s.w.nseg * s.w.nq * sizeof(double));
  if (n_valid) std::memcpy(n_valid, s.h_n_valid, (size_t)s.w.nseg * sizeof(int64_t));
  return EA_OK;
}

static int check_quantile_args(const double *probs, int nq) {
  if (!probs) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (nq < 1 || nq > kSelectMaxQ) return fail(EA_ERR_INVALID_ARG, "nq must be in 1..16");
  for (int i = 0; i < nq; ++i)
    if (!select_prob_ok(probs[i])) return fail(EA_ERR_INVALID_ARG, "every prob must be in [0, 1]");
  return EA_OK;
}

// the quantiles of the head families of problems sel[0 .. nsel) (sel == NULL: all of them) at the batch's poses q, t
// (count x 4, count x 3: the poses of ALL problems of the batch); values: nsel x nq, n_valid: nsel or NULL
static int batch_quantiles(ea_batch *b, const double *q, const double *t, const int *sel, int nsel, const double *probs, int nq,
                           double *values, int64_t *n_valid) {
  BatchView v;
  int rc = batch_built(b, &v);
  if (rc == EA_OK) rc = check_segment_count((size_t)nsel, "quantile");
  if (rc != EA_OK) return rc;
  SelectBuffers s;
  if ((rc = select_reserve(s, v.device, nsel, nq, v.total_rows, false)) != EA_OK) return rc;
  HeadFamilies heads{v, sel};
  for (int j = 0; j < nsel; ++j) {
    const HeadFamily h = heads(j);
    s.h_segs[j] = SelectSeg{h.row_begin, h.n, h.term};
  }
  if ((rc = select_begin(s, probs, v.stream)) != EA_OK) return rc;
  const PoseState *d_poses;
  if ((rc = batch_upload_poses(b, q, t, &d_poses)) != EA_OK) return rc;
  HIPCHK(launch_select_keys(v.dtype, s.w, v.d_probs, d_poses, v.stream));
  return select_finish(s, v.stream, values, n_valid);
}

extern "C" int ea_batch_residual_quantiles(ea_batch *b, const double *q, const double *t, const double *probs, int nq,
                                           double *values, int64_t *n_valid) {
  if (!b || !q || !t || !values) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = check_quantile_args(probs, nq);
  if (rc == EA_OK) rc = require_device();
  if (rc != EA_OK) return rc;
  return batch_quantiles(b, q, t, nullptr, batch_view(b).count, probs, nq, values, n_valid);
}

extern "C" int ea_problem_residual_quantiles(ea_problem *p, const double q[4], const double t[3], const double *probs, int nq,
                                             double *values, int64_t *n_valid) {
  if (!p || !q || !t || !values) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = check_quantile_args(probs, nq);
  if (rc == EA_OK) rc = require_device();
  if (rc != EA_OK) return rc;
  ea_batch *b;
  if ((rc = problem_call_batch(p, &b)) != EA_OK) return rc;
  return batch_quantiles(b, q, t, nullptr, 1, probs, nq, values, n_valid);
}

// ---- how much of a reference is seen at a pose (ea_pose_stats; kernels: ea_pose_stats_kernel and its fold) ----------------
//
// Segments and poses up, the two launches, the rows down through one pinned block, ONE synchronisation: all on the batch's
// stream.  The poses go through d_poses, like the quantiles': the resident poses of ea_batch_set_poses live elsewhere.
static_assert(sizeof(PoseStatsRow) == sizeof(ea_pose_stats), "the fold writes ea_pose_stats as it stands");
static int check_pose_stats_args(int margin, double inlier_residual) {
  if (margin < 0) return fail(EA_ERR_INVALID_ARG, "margin must be >= 0");
  if (!(inlier_residual >= 0.0)) return fail(EA_ERR_INVALID_ARG, "inlier_residual must be >= 0 (+Inf is allowed)");
  return EA_OK;
}

static int batch_pose_stats(ea_batch *b, const double *q, const double *t, int margin, double inlier_residual, ea_pose_stats *out) {
  BatchView v;
  int rc = batch_built(b, &v);
  if (rc == EA_OK) rc = check_segment_count((size_t)v.count, "statistics");
  if (rc != EA_OK) return rc;
  const int nseg = v.count;
  // [segments | one row per segment], and on the device the kernel's partials behind them
  SegmentBlock blk;
  const size_t o_parts = align16(blk.layout((size_t)nseg * sizeof(SelectSeg), (size_t)nseg * sizeof(PoseStatsRow)));
  blk.up_bytes = blk.o_results;  // (the kernel writes every row: only the segments go up)
  HIPCHK(blk.take_pinned(o_parts, v.device));
  HeadFamilies heads{v};
  int64_t rows = 0;
  for (int j = 0; j < nseg; ++j) {
    const HeadFamily h = heads(j);
    blk.records<SelectSeg>()[j] = SelectSeg{rows, h.n, h.term};
    rows += pose_stats_rows(h.n);
  }
  HIPCHK(blk.take_device(o_parts + (size_t)std::max<int64_t>(rows, 1) * sizeof(PoseStatsPartial), v.device));
  PoseStatsWork w;
  w.nseg = nseg; w.max_n = heads.max_n; w.margin = margin; w.inlier_residual = inlier_residual;
  w.segs = blk.dev_records<SelectSeg>();
  w.out = blk.dev_results<PoseStatsRow>();
  w.partials = reinterpret_cast<PoseStatsPartial *>(blk.dev + o_parts);
  HIPCHK(blk.up(v.stream));
  const PoseState *d_poses;
  if ((rc = batch_upload_poses(b, q, t, &d_poses)) != EA_OK) return rc;
  HIPCHK(launch_pose_stats(v.dtype, w, v.d_probs, d_poses, v.stream));
  HIPCHK(blk.down(v.stream));
  HIPCHK(hipStreamSynchronize(v.stream));
  std::memcpy(out, blk.results<ea_pose_stats>(), (size_t)nseg * sizeof(ea_pose_stats));
  return EA_OK;
}

extern "C" int ea_batch_pose_stats(ea_batch *b, const double *q, const double *t, int margin, double inlier_residual,
                                   ea_pose_stats *out) {
  if (!b || !q || !t || !out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = check_pose_stats_args(margin, inlier_residual);
  if (rc == EA_OK) rc = require_device();
  if (rc != EA_OK) return rc;
  return batch_pose_stats(b, q, t, margin, inlier_residual, out);
}

extern "C" int ea_problem_pose_stats(ea_problem *p, const double q[4], const double t[3], int margin, double inlier_residual,
                                     ea_pose_stats *out) {
  if (!p || !q || !t || !out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = check_pose_stats_args(margin, inlier_residual);
  if (rc == EA_OK) rc = require_device();
  if (rc != EA_OK) return rc;
  ea_batch *b;
  if ((rc = problem_call_batch(p, &b)) != EA_OK) return rc;
  return batch_pose_stats(b, q, t, margin, inlier_residual, out);
}

// the select kernels alone, on the caller's values
extern "C" int ea_selftest_select(int device, const double *values, const int64_t *offsets, int nseg, const double *probs, int nq,
                                  double *out, int64_t *n_valid) {
  if (!offsets || !out || nseg < 1 || nseg > 65535) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = check_quantile_args(probs, nq);
  if (rc != EA_OK) return rc;
  if (offsets[0] < 0) return fail(EA_ERR_INVALID_ARG, "offsets must start at >= 0 and not decrease");
  for (int i = 0; i < nseg; ++i)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 0x7fffff00LL)
      return fail(EA_ERR_INVALID_ARG, "offsets must not decrease (at most 2^31 values per segment)");
  const int64_t total = offsets[nseg];
  if (total > 0 && !values) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if ((rc = check_device(device)) != EA_OK) return rc;
  HIPCHK(hipSetDevice(device));
  SelectBuffers s;
  if ((rc = select_reserve(s, device, nseg, nq, total, true)) != EA_OK) return rc;
  for (int i = 0; i < nseg; ++i) s.h_segs[i] = SelectSeg{offsets[i], (int32_t)(offsets[i + 1] - offsets[i]), 0};
  hipStream_t stream = nullptr;
  HIPCHK(cached_stream_create(&stream, device));
  rc = select_begin(s, probs, stream);
  hipError_t e = hipSuccess;
  if (rc == EA_OK && total > 0) e = hipMemcpyAsync(s.d_input, values, (size_t)total * sizeof(double), hipMemcpyHostToDevice, stream);
  if (rc == EA_OK && e == hipSuccess) e = launch_select_keys_values(s.w, s.d_input, stream);
  if (rc == EA_OK && e == hipSuccess) rc = select_finish(s, stream, out, n_valid);
  (void)hipStreamSynchronize(stream);
  cached_stream_destroy(stream, device);
  if (e != hipSuccess) return fail(EA_ERR_HIP, hipGetErrorString(e));
  return rc;
}

// Auto-scaled losses (ea_problem_set_loss_auto_scale): ONE quantile call over the auto-scaled problems of the batch at their
// start poses, then, per problem, what the caller could have done by hand: ea_problem_set_loss(kind, max(a_min, factor * Q)).
// The trivial loss is left alone; a problem without a valid block (or a product that is not finite) keeps its scale.
int ea::auto_scale_losses(ea_batch *b, const double *q, const double *t) {
  const BatchView v = batch_view(b);
  const std::vector<ea_problem *> members(v.probs, v.probs + v.count);
  std::vector<double> probs;
  for (const ea_problem *p : members)
    if (p->auto_factor > 0.0 && p->loss_kind != EA_LOSS_TRIVIAL && std::find(probs.begin(), probs.end(), p->auto_prob) == probs.end())
      probs.push_back(p->auto_prob);
  // (problems may ask for different probabilities: up to 16 of them share a call)
  for (size_t first = 0; first < probs.size(); first += kSelectMaxQ) {
    const int nq = (int)std::min<size_t>(kSelectMaxQ, probs.size() - first);
    std::vector<int> sel, which;
    for (size_t i = 0; i < members.size(); ++i) {
      const ea_problem *p = members[i];
      if (!(p->auto_factor > 0.0) || p->loss_kind == EA_LOSS_TRIVIAL) continue;
      const size_t at = (size_t)(std::find(probs.begin(), probs.end(), p->auto_prob) - probs.begin());
      if (at >= first && at < first + (size_t)nq) { sel.push_back((int)i); which.push_back((int)(at - first)); }
    }
    std::vector<double> values(sel.size() * (size_t)nq);
    std::vector<int64_t> m(sel.size());
    int rc = require_device();
    if (rc == EA_OK) rc = batch_quantiles(b, q, t, sel.data(), (int)sel.size(), probs.data() + first, nq, values.data(), m.data());
    if (rc != EA_OK) return rc;
    for (size_t j = 0; j < sel.size(); ++j) {
      ea_problem *p = members[(size_t)sel[j]];
      if (m[j] <= 0) continue;
      const double a = select_loss_scale(p->auto_factor, values[j * (size_t)nq + (size_t)which[j]], p->auto_a_min);
      if (!(a <= DBL_MAX) || a == p->loss_a) continue;
      if ((rc = ea_problem_set_loss(p, p->loss_kind, a)) != EA_OK) return rc;
    }
  }
  return EA_OK;
}

// ---- reprojection and overlay: reproject + s_overlay (ea_reproject.h; kernel: ea_reproject_kernel) -----------------------
//
// One segment per problem of the call (its head family) with the 3x4 matrix of step A, built here; the results are the
// overlay's counters.  The matrices travel in the segments: d_poses is not written, and no problem changes, so resident
// poses (ea_batch_set_poses) survive.
extern "C" int ea_pose_to_matrix(const double q[4], const double t[3], double b_T_a[16]) {
  if (!q || !t || !b_T_a) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  pose_to_matrix(q, t, b_T_a);
  return EA_OK;
}

extern "C" int ea_matrix_to_pose(const double b_T_a[16], double q[4], double t[3]) {
  if (!b_T_a || !q || !t) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!matrix_to_pose(b_T_a, q, t)) return fail(EA_ERR_INVALID_ARG, "b_T_a[15] must be 1 (the reference's assert( T(3,3) == 1 ))");
  return EA_OK;
}

static int check_reproject_poses(const double *b_T_a, int count) {
  for (int i = 0; i < count; ++i)
    if (!reproject_pose_ok(b_T_a + 16 * (size_t)i))
      return fail(EA_ERR_INVALID_ARG, "b_T_a must be finite with the last row exactly 0 0 0 1");
  return EA_OK;
}

// upload + launch (+ the counters on their way back) for a batch that is built; the caller queues what else must come down
// and synchronises.  paint: images[i] = device image of problem i (H x W x 3)
static int reproject_enqueue(const BatchView &v, const double *b_T_a, bool paint, double *uv_dev, unsigned char *const *images,
                             const uint8_t color[3], SegmentBlock &blk) {
  const int nseg = v.count;
  int rc = check_segment_count((size_t)nseg, "reprojection");
  if (rc != EA_OK) return rc;
  const size_t bytes = blk.layout((size_t)nseg * sizeof(ReprojectSeg), (size_t)nseg * 2 * sizeof(unsigned long long));
  HIPCHK(blk.take_pinned(bytes, v.device));
  std::memset(blk.pinned, 0, bytes);
  HeadFamilies heads{v};
  for (int j = 0; j < nseg; ++j) {
    const HeadFamily h = heads(j);
    ReprojectSeg &sg = blk.records<ReprojectSeg>()[j];
    sg.row = h.row_begin; sg.n = h.n; sg.term = h.term;
    segment_matrix(h.problem, b_T_a + 16 * (size_t)j, sg.M);
    sg.image = paint ? images[j] : nullptr;
  }
  HIPCHK(blk.take_device(bytes, v.device));
  HIPCHK(blk.up(v.stream));
  ReprojectWork w;
  w.nseg = nseg; w.max_n = heads.max_n; w.paint = paint ? 1 : 0;
  w.color = color ? ((unsigned)color[0] | ((unsigned)color[1] << 8) | ((unsigned)color[2] << 16)) : (255u << 16);  // NULL: upstream's red
  w.segs = blk.dev_records<ReprojectSeg>();
  w.uv = uv_dev;
  w.counts = blk.dev_results<unsigned long long>();
  HIPCHK(launch_reproject(v.dtype, w, v.d_probs, v.stream));
  if (paint) HIPCHK(blk.down(v.stream));
  return EA_OK;
}

static void reproject_stats(const BatchView &v, const SegmentBlock &blk, ea_overlay_stats *stats) {
  if (!stats) return;
  for (int j = 0; j < v.count; ++j) {
    stats[j].n = blk.records<ReprojectSeg>()[j].n;
    stats[j].inside = (int64_t)blk.results<unsigned long long>()[2 * j];
    stats[j].outside = (int64_t)blk.results<unsigned long long>()[2 * j + 1];
  }
}

// rows of the batch's layout (ea_batch_row_offsets) as the problems stand, without a device
static int64_t batch_rows_host(const BatchView &v) {
  int64_t rows = 0;
  for (int i = 0; i < v.count; ++i) rows += problem_points(v.probs[i]);
  return rows;
}

// what the two batch forms check before a device is looked for, then the built batch
static int batch_reproject_prepare(ea_batch *b, const double *b_T_a, const void *uv, int64_t capacity_rows, BatchView *v) {
  if (!b || !b_T_a || !uv) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  *v = batch_view(b);
  int rc = check_reproject_poses(b_T_a, v->count);
  if (rc != EA_OK) return rc;
  if (capacity_rows < batch_rows_host(*v)) return fail(EA_ERR_INVALID_ARG, "capacity_rows is smaller than the batch's row count (ea_batch_row_offsets)");
  if ((rc = require_device()) != EA_OK) return rc;
  return batch_built(b, v);
}

// the rows of a built batch into host memory: `rows` of them on the device, the head families' down to uv
static int reproject_to_host(const BatchView &v, const double *b_T_a, int64_t rows, double *uv) {
  DevBuf d_uv;
  HIPCHK(cached_malloc(&d_uv.p, (size_t)rows * 2 * sizeof(double), v.device));
  SegmentBlock blk;
  int rc = reproject_enqueue(v, b_T_a, false, d_uv.as<double>(), nullptr, nullptr, blk);
  if (rc == EA_OK) rc = download_head_rows(v, 2 * sizeof(double), d_uv.p, uv);
  if (rc != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(v.stream));
  return EA_OK;
}

extern "C" int ea_batch_reproject_device(ea_batch *b, const double *b_T_a, double *uv_dev, int64_t capacity_rows) {
  BatchView v;
  int rc = batch_reproject_prepare(b, b_T_a, uv_dev, capacity_rows, &v);
  if (rc != EA_OK) return rc;
  if ((rc = check_device_pointer(v.device, uv_dev, "uv_dev")) != EA_OK) return rc;
  SegmentBlock blk;
  if ((rc = reproject_enqueue(v, b_T_a, false, uv_dev, nullptr, nullptr, blk)) != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(v.stream));  // the rows are complete (and visible to any other stream) when this returns
  return EA_OK;
}

extern "C" int ea_batch_reproject(ea_batch *b, const double *b_T_a, double *uv, int64_t capacity_rows) {
  BatchView v;
  int rc = batch_reproject_prepare(b, b_T_a, uv, capacity_rows, &v);
  if (rc != EA_OK) return rc;
  return reproject_to_host(v, b_T_a, v.total_rows, uv);
}

extern "C" int ea_problem_reproject(ea_problem *p, const double b_T_a[16], double *uv, int64_t capacity) {
  if (!p || !b_T_a || !uv) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = check_reproject_poses(b_T_a, 1);
  if (rc != EA_OK) return rc;
  if (capacity < p->n) return fail(EA_ERR_INVALID_ARG, "capacity is smaller than ea_problem_num_points");
  if ((rc = require_device()) != EA_OK) return rc;
  ea_batch *b;
  BatchView v;
  if ((rc = problem_call_batch(p, &b)) != EA_OK) return rc;
  if ((rc = batch_built(b, &v)) != EA_OK) return rc;
  std::vector<double> tmp(p->order.empty() ? 0 : (size_t)p->n * 2);  // (tile order: by way of tmp)
  rc = reproject_to_host(v, b_T_a, p->n, tmp.empty() ? uv : tmp.data());  // (the head family's rows start at 0)
  if (rc == EA_OK) scatter_to_callers_order(p->order, 2 * sizeof(double), tmp.data(), uv);
  return rc;
}

// what the batch forms of the overlay check before a device is looked for (entries: the pointer arrays whose `count` entries
// must not be NULL), then the built batch and the extent of its images
static int batch_overlay_prepare(ea_batch *b, const double *b_T_a, const void *const *entries_a, const void *const *entries_b,
                                 int height, int width, BatchView *v) {
  if (!b || !b_T_a || !entries_a || !entries_b) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (height < 1 || width < 1) return fail(EA_ERR_INVALID_ARG, "height and width must be positive");
  *v = batch_view(b);
  int rc = check_reproject_poses(b_T_a, v->count);
  if (rc != EA_OK) return rc;
  for (int i = 0; i < v->count; ++i)
    if (!entries_a[i] || !entries_b[i]) return fail(EA_ERR_INVALID_ARG, "NULL entry in an image pointer array");
  if ((rc = require_device()) != EA_OK || (rc = batch_built(b, v)) != EA_OK) return rc;
  for (int i = 0; i < v->count; ++i)
    if (v->probs[i]->H != height || v->probs[i]->W != width)
      return fail(EA_ERR_INVALID_ARG, "height, width must equal the extent of every problem's distance-transform image");
  return EA_OK;
}

extern "C" int ea_batch_overlay_device(ea_batch *b, const double *b_T_a, uint8_t *const *bgr_dev, int height, int width,
                                       const uint8_t color[3], ea_overlay_stats *stats) {
  BatchView v;
  int rc = batch_overlay_prepare(b, b_T_a, reinterpret_cast<const void *const *>(bgr_dev),
                                 reinterpret_cast<const void *const *>(bgr_dev), height, width, &v);
  if (rc != EA_OK) return rc;
  for (int i = 0; i < v.count; ++i)
    if (!device_memory_of(bgr_dev[i], v.device))
      return fail(EA_ERR_INVALID_ARG, "an entry of bgr_dev is not device memory of the batch's device");
  SegmentBlock blk;
  if ((rc = reproject_enqueue(v, b_T_a, true, nullptr, bgr_dev, color, blk)) != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(v.stream));  // the images are complete (and visible to any other stream) when this returns
  reproject_stats(v, blk, stats);
  return EA_OK;
}

extern "C" int ea_batch_overlay(ea_batch *b, const double *b_T_a, const uint8_t *const *bgr_in, int height, int width,
                                const uint8_t color[3], uint8_t *const *bgr_out, ea_overlay_stats *stats) {
  BatchView v;
  int rc = batch_overlay_prepare(b, b_T_a, reinterpret_cast<const void *const *>(bgr_in),
                                 reinterpret_cast<const void *const *>(bgr_out), height, width, &v);
  if (rc != EA_OK) return rc;
  // the images go up into one cached device block, are painted there and come back
  const size_t count = (size_t)v.count, image_bytes = (size_t)height * (size_t)width * 3, stride = align16(image_bytes);
  DevBuf images;
  HIPCHK(cached_malloc(&images.p, count * stride, v.device));
  std::vector<unsigned char *> d_images(count);
  for (size_t i = 0; i < count; ++i) {
    d_images[i] = images.as<unsigned char>() + i * stride;
    HIPCHK(hipMemcpyAsync(d_images[i], bgr_in[i], image_bytes, hipMemcpyHostToDevice, v.stream));
  }
  SegmentBlock blk;
  if ((rc = reproject_enqueue(v, b_T_a, true, nullptr, d_images.data(), color, blk)) != EA_OK) return rc;
  for (size_t i = 0; i < count; ++i)
    HIPCHK(hipMemcpyAsync(bgr_out[i], d_images[i], image_bytes, hipMemcpyDeviceToHost, v.stream));
  HIPCHK(hipStreamSynchronize(v.stream));
  reproject_stats(v, blk, stats);
  return EA_OK;
}

extern "C" int ea_problem_overlay(ea_problem *p, const double b_T_a[16], const uint8_t *bgr_in, int height, int width,
                                  const uint8_t color[3], uint8_t *bgr_out, ea_overlay_stats *stats) {
  if (!p || !b_T_a || !bgr_in || !bgr_out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (height < 1 || width < 1) return fail(EA_ERR_INVALID_ARG, "height and width must be positive");
  int rc = check_reproject_poses(b_T_a, 1);
  if (rc == EA_OK) rc = require_device();
  if (rc != EA_OK) return rc;
  ea_batch *b;
  if ((rc = problem_call_batch(p, &b)) != EA_OK) return rc;
  return ea_batch_overlay(b, b_T_a, &bgr_in, height, width, color, &bgr_out, stats);
}

// ---- depth-consistency gate (ea_depth_gate.h; kernel: ea_depth_gate_kernel) ------------------------------------------------
//
// The current frame's depth is held by the problem in its own kind (a cached block, copied as it came).  It is read by the
// gate only -- no descriptor names it -- so setting it moves no version: batches do not rebuild, resident poses survive.
static void now_depth_drop(ea_problem *p) {
  if (p->d_now_depth) cached_free(p->d_now_depth);
  p->d_now_depth = nullptr;
  p->now_depth_cap = 0;
  p->nd_kind = p->nd_H = p->nd_W = 0;
  p->nd_z_scaling = 1.0;
}

static size_t now_depth_bytes(int kind, int height, int width) {
  return (size_t)height * (size_t)width * (kind == EA_DEPTH_F32 ? sizeof(float) : sizeof(uint16_t));
}

// room for the image in the problem's block (the previous allocation when it fits and is not four times too large) and the
// image's description; the samples are the caller's to copy
static int now_depth_reserve(ea_problem *p, int kind, int height, int width, double z_scaling) {
  const size_t need = now_depth_bytes(kind, height, width);
  if (!(p->d_now_depth && p->now_depth_cap >= need && p->now_depth_cap <= 4 * need + 4096)) {
    now_depth_drop(p);
    HIPCHK(cached_malloc(&p->d_now_depth, need, p->device));
    p->now_depth_cap = need;
  }
  p->nd_kind = kind; p->nd_H = height; p->nd_W = width;
  p->nd_z_scaling = kind == EA_DEPTH_U16 ? z_scaling : 1.0;
  return EA_OK;
}

// a depth image the caller says is in device memory: of this device, as far as the runtime can tell, aligned for its samples
static int check_device_depth(const void *ptr, int device, int kind) {
  if (reinterpret_cast<uintptr_t>(ptr) % (kind == EA_DEPTH_F32 ? 4 : 2) != 0) return fail(EA_ERR_INVALID_ARG, "depth_dev: misaligned image");
  if (!device_memory_of(ptr, device)) return fail(EA_ERR_INVALID_ARG, "depth_dev is not device memory of the problem's device");
  return EA_OK;
}

static int problem_set_now_depth(ea_problem *p, const void *depth, int kind, int height, int width, double z_scaling, bool on_device) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  if (!depth) { now_depth_drop(p); return EA_OK; }
  if (const char *why = now_depth_args_error(kind, height, width, z_scaling)) return fail(EA_ERR_INVALID_ARG, why);
  int rc = require_device();
  if (rc != EA_OK) return rc;
  HIPCHK(hipSetDevice(p->device));
  if (on_device && (rc = check_device_depth(depth, p->device, kind)) != EA_OK) return rc;
  if ((rc = now_depth_reserve(p, kind, height, width, z_scaling)) != EA_OK) return rc;
  hipError_t e = hipMemcpy(p->d_now_depth, depth, now_depth_bytes(kind, height, width),
                           on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // (a device-to-device copy may return before it has run)
  if (e != hipSuccess) {
    now_depth_drop(p);
    return fail(EA_ERR_HIP, std::string("ea_problem_set_now_depth: ") + hipGetErrorString(e));
  }
  return EA_OK;
}

extern "C" int ea_problem_set_now_depth(ea_problem *p, const void *depth, int kind, int height, int width, double z_scaling) {
  return problem_set_now_depth(p, depth, kind, height, width, z_scaling, false);
}

extern "C" int ea_problem_set_now_depth_device(ea_problem *p, const void *depth_dev, int kind, int height, int width,
                                               double z_scaling) {
  return problem_set_now_depth(p, depth_dev, kind, height, width, z_scaling, true);
}

static bool batch_has_duplicates(const BatchView &v) {
  std::vector<const ea_problem *> sorted(v.probs, v.probs + v.count);
  std::sort(sorted.begin(), sorted.end());
  return std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end();
}

// N images, one per problem: the copies on the batch's stream, ONE wait
static int batch_set_now_depth(ea_batch *b, const void *const *depth, int kind, int height, int width, double z_scaling, bool on_device) {
  if (!b) return fail(EA_ERR_INVALID_ARG, "NULL batch");
  const BatchView v = batch_view(b);
  if (!depth) {
    for (int i = 0; i < v.count; ++i) now_depth_drop(v.probs[i]);
    return EA_OK;
  }
  if (const char *why = now_depth_args_error(kind, height, width, z_scaling)) return fail(EA_ERR_INVALID_ARG, why);
  for (int i = 0; i < v.count; ++i)
    if (!depth[i]) return fail(EA_ERR_INVALID_ARG, "NULL entry in the depth pointer array");
  if (batch_has_duplicates(v))
    return fail(EA_ERR_INVALID_ARG, "the same problem twice in the batch: each depth image needs a problem of its own");
  int rc = require_device();
  if (rc != EA_OK) return rc;
  HIPCHK(hipSetDevice(v.device));
  if (on_device)
    for (int i = 0; i < v.count; ++i)
      if ((rc = check_device_depth(depth[i], v.device, kind)) != EA_OK) return rc;
  const size_t bytes = now_depth_bytes(kind, height, width);
  hipError_t e = hipSuccess;
  for (int i = 0; i < v.count && rc == EA_OK && e == hipSuccess; ++i) {
    ea_problem *p = v.probs[i];
    if ((rc = now_depth_reserve(p, kind, height, width, z_scaling)) != EA_OK) break;
    e = hipMemcpyAsync(p->d_now_depth, depth[i], bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, v.stream);
  }
  const hipError_t es = hipStreamSynchronize(v.stream);
  if (e == hipSuccess) e = es;
  if (rc != EA_OK || e != hipSuccess) {  // no problem keeps an image that may be half written
    for (int i = 0; i < v.count; ++i) now_depth_drop(v.probs[i]);
    return rc != EA_OK ? rc : fail(EA_ERR_HIP, std::string("ea_batch_set_now_depth: ") + hipGetErrorString(e));
  }
  return EA_OK;
}

extern "C" int ea_batch_set_now_depth(ea_batch *b, const void *const *depth, int kind, int height, int width, double z_scaling) {
  return batch_set_now_depth(b, depth, kind, height, width, z_scaling, false);
}

extern "C" int ea_batch_set_now_depth_device(ea_batch *b, const void *const *depth_dev, int kind, int height, int width,
                                             double z_scaling) {
  return batch_set_now_depth(b, depth_dev, kind, height, width, z_scaling, true);
}

extern "C" void ea_default_depth_gate_params(ea_depth_gate_params *prm) {
  if (!prm) return;
  prm->radius = 1;
  prm->abs_tol = 0.02; prm->rel_tol = 0.02;
  prm->w_occluded = 0.0; prm->w_free = 0.0; prm->w_unknown = 1.0;
  prm->apply = 1;
}

// The gate itself.  One segment per problem of the call (its head family) with the 3x4 matrix of step A; the results are the
// class counters.  The matrices travel in the segments: d_poses is not written.  With `apply` the kernel writes the problems'
// weight storage in place; a problem that had no weights becomes a weighted one afterwards (its version moves: the batches
// that hold it rebuild, as after ea_problem_set_weights), one that had keeps its version.

// what needs neither a handle nor a device
static int depth_gate_params_check(const ea_depth_gate_params *prm) {
  if (const char *why = depth_gate_params_error(prm)) return fail(EA_ERR_INVALID_ARG, why);
  return EA_OK;
}

// what the problems of a call must be, read off the problems themselves: nothing has touched a device or changed a problem yet
static int depth_gate_state_checks(const BatchView &v, const ea_depth_gate_params *prm) {
  if (int rc = check_segment_count((size_t)v.count, "depth gate")) return rc;
  if (!depth_gate_factors_fit(prm, v.dtype == EA_F32 ? (double)FLT_MAX : DBL_MAX))
    return fail(EA_ERR_INVALID_ARG, "a weight factor overflows the float of an fp32 problem");
  if (prm->apply && batch_has_duplicates(v))
    return fail(EA_ERR_INVALID_ARG, "the same problem twice in the batch: its weights can be written once per call");
  for (int i = 0; i < v.count; ++i) {
    const ea_problem *p = v.probs[i];
    if (!p->d_dt) return fail(EA_ERR_STATE, "distance-transform image not set (ea_problem_set_dt)");
    if (!p->d_now_depth) return fail(EA_ERR_STATE, "current-frame depth not set (ea_problem_set_now_depth)");
    if (depth_gate_shift(p->H, p->W, p->nd_H, p->nd_W) < 0)
      return fail(EA_ERR_STATE, "the current-frame depth is not the distance-transform image's extent times one power of two (2^0..2^8, at most 2^30 pixels)");
    if (p->nd_kind != v.probs[0]->nd_kind)
      return fail(EA_ERR_STATE, "the problems of one depth gate call must hold depth of one kind");
  }
  return EA_OK;
}

// upload + launch + the counters on their way back, for a batch that is built; the caller queues what else must come down and
// synchronises.  cls_dev: class bytes in the rows layout, or NULL
// img: the depth images of the call when they are not the problems' held now-depth (the multi-stream tracker's pushed frames)
static int depth_gate_enqueue(ea_batch *b, const BatchView &v, const double *b_T_a, const ea_depth_gate_params *prm,
                              unsigned char *cls_dev, SegmentBlock &blk, const GateImages *img = nullptr) {
  const int nseg = v.count;
  const size_t bytes = blk.layout((size_t)nseg * sizeof(DepthGateSeg), (size_t)nseg * kDepthGateClasses * sizeof(unsigned long long));
  blk.cached = false;  // (the batch's own pair: ea_batch says why)
  int rc = batch_gate_reserve(b, bytes, &blk.dev, &blk.pinned);
  if (rc != EA_OK) return rc;
  std::memset(blk.pinned, 0, bytes);
  HeadFamilies heads{v};
  for (int j = 0; j < nseg; ++j) {
    const HeadFamily h = heads(j);
    const ea_problem *p = h.problem;
    DepthGateSeg &sg = blk.records<DepthGateSeg>()[j];
    sg.row = h.row_begin; sg.n = h.n; sg.term = h.term;
    segment_matrix(p, b_T_a + 16 * (size_t)j, sg.M);
    sg.depth = img ? img->depth[j] : p->d_now_depth;
    sg.z_scaling = img ? img->z_scaling : p->nd_z_scaling;
    sg.shift = img ? img->shift : depth_gate_shift(p->H, p->W, p->nd_H, p->nd_W);
    sg.weights = (prm->apply && sg.n > 0) ? weights_ptr(p) : nullptr;
    sg.cls = cls_dev ? cls_dev + sg.row : nullptr;
    sg.dw_z_ref = p->dw_z_ref;
    sg.dw_power = p->dw_power;
  }
  HIPCHK(blk.up(v.stream));
  DepthGateWork w;
  w.nseg = nseg; w.max_n = heads.max_n; w.kind = img ? img->kind : v.probs[0]->nd_kind; w.radius = prm->radius;
  w.rule = depth_gate_rule(prm);
  w.segs = blk.dev_records<DepthGateSeg>();
  w.counts = blk.dev_results<unsigned long long>();
  HIPCHK(launch_depth_gate(v.dtype, w, v.d_probs, v.stream));
  HIPCHK(blk.down(v.stream));
  return EA_OK;
}

// after the synchronisation: the counts, and with `apply` the problems' new state
static void depth_gate_finish(const BatchView &v, const ea_depth_gate_params *prm, const SegmentBlock &blk, ea_depth_gate_stats *stats) {
  const DepthGateSeg *segs = blk.records<DepthGateSeg>();
  for (int j = 0; j < v.count; ++j) {
    if (stats) {
      const unsigned long long *c = blk.results<unsigned long long>() + (size_t)kDepthGateClasses * j;
      stats[j].n = segs[j].n;
      stats[j].n_behind = (int64_t)c[EA_GATE_BEHIND]; stats[j].n_outside = (int64_t)c[EA_GATE_OUTSIDE];
      stats[j].n_unknown = (int64_t)c[EA_GATE_UNKNOWN]; stats[j].n_consistent = (int64_t)c[EA_GATE_CONSISTENT];
      stats[j].n_occluded = (int64_t)c[EA_GATE_OCCLUDED]; stats[j].n_free = (int64_t)c[EA_GATE_FREE];
    }
    ea_problem *p = v.probs[j];
    if (prm->apply && segs[j].n > 0) {
      p->weights_from_depth = false;
      if (!p->weighted) { p->weighted = true; p->version++; }  // (new values alone need no rebuild of a batch)
    }
  }
}

// the checks of the three forms and everything up to a built batch whose problems own their points (apply)
static int depth_gate_prepare(ea_batch *b, const ea_depth_gate_params *prm, BatchView *v) {
  *v = batch_view(b);
  int rc = depth_gate_state_checks(*v, prm);
  if (rc == EA_OK) rc = require_device();
  if (rc != EA_OK) return rc;
  HIPCHK(hipSetDevice(v->device));
  if (prm->apply)
    for (int i = 0; i < v->count; ++i)
      if ((rc = own_borrowed_points(v->probs[i])) != EA_OK) return rc;  // (the weights live behind z in an allocation of the problem's)
  return batch_built(b, v);
}

static int batch_depth_gate_checks(ea_batch *b, const double *b_T_a, const ea_depth_gate_params *prm, const void *cls,
                                   int64_t capacity_rows) {
  if (!b || !b_T_a || !prm) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = depth_gate_params_check(prm);  // (the batch is looked at only for what depends on it)
  const BatchView v = batch_view(b);
  if (rc == EA_OK) rc = check_reproject_poses(b_T_a, v.count);
  if (rc != EA_OK) return rc;
  if (cls && capacity_rows < batch_rows_host(v))
    return fail(EA_ERR_INVALID_ARG, "capacity_rows is smaller than the batch's row count (ea_batch_row_offsets)");
  return EA_OK;
}

extern "C" int ea_batch_depth_gate_device(ea_batch *b, const double *b_T_a, const ea_depth_gate_params *prm, uint8_t *cls_dev,
                                          int64_t capacity_rows, ea_depth_gate_stats *stats) {
  int rc = batch_depth_gate_checks(b, b_T_a, prm, cls_dev, capacity_rows);
  if (rc != EA_OK) return rc;
  if (cls_dev) {  // (before a problem is changed)
    if ((rc = require_device()) != EA_OK) return rc;
    if (!device_memory_of(cls_dev, batch_view(b).device))
      return fail(EA_ERR_INVALID_ARG, "cls_dev is not device memory of the batch's device");
  }
  BatchView v;
  if ((rc = depth_gate_prepare(b, prm, &v)) != EA_OK) return rc;
  SegmentBlock blk;
  if ((rc = depth_gate_enqueue(b, v, b_T_a, prm, cls_dev, blk)) != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(v.stream));  // weights and classes are complete (and visible to any other stream) when this returns
  depth_gate_finish(v, prm, blk, stats);
  return EA_OK;
}

// weights, counters and, with cls, the class bytes of a built batch into host memory: `rows` of them on the device, the head
// families' down to cls
static int depth_gate_to_host(ea_batch *b, const BatchView &v, const double *b_T_a, const ea_depth_gate_params *prm, int64_t rows,
                              uint8_t *cls, ea_depth_gate_stats *stats) {
  DevBuf d_cls;
  if (cls && rows > 0) HIPCHK(cached_malloc(&d_cls.p, (size_t)rows, v.device));
  SegmentBlock blk;
  int rc = depth_gate_enqueue(b, v, b_T_a, prm, d_cls.as<unsigned char>(), blk);
  if (rc == EA_OK && d_cls.p) rc = download_head_rows(v, 1, d_cls.p, cls);
  if (rc != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(v.stream));
  depth_gate_finish(v, prm, blk, stats);
  return EA_OK;
}

// The multi-stream tracker's gate of one solved (level, group), on the batch that solves it: the parameters were checked when
// the gate was set, the poses are the tracker's own, every problem owns its points and has its image (usable), and the depth
// images are the pushed frames (img) -- no held now-depth is read or touched.  One launch and one wait on the batch's stream.
int ea::batch_depth_gate_images(ea_batch *b, const double *b_T_a, const ea_depth_gate_params *prm, const GateImages &img,
                                ea_depth_gate_stats *stats) {
  BatchView v = batch_view(b);
  int rc = check_segment_count((size_t)v.count, "depth gate");
  if (rc != EA_OK) return rc;
  for (int i = 0; i < v.count; ++i) {
    const ea_problem *p = v.probs[i];
    if (!p->d_dt || !img.depth[i]) return fail(EA_ERR_STATE, "depth gate: a stream without an image or a depth frame");
    if (img.shift < 0 || img.shift > kDepthGateMaxShift || (((int64_t)p->H * p->W) << (2 * img.shift)) > ((int64_t)1 << 30))
      return fail(EA_ERR_STATE, "depth gate: the depth frame is more than 2^8 times the level's extent or more than 2^30 pixels");
  }
  HIPCHK(hipSetDevice(v.device));
  if ((rc = batch_built(b, &v)) != EA_OK) return rc;
  SegmentBlock blk;
  if ((rc = depth_gate_enqueue(b, v, b_T_a, prm, nullptr, blk, &img)) != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(v.stream));
  depth_gate_finish(v, prm, blk, stats);
  return EA_OK;
}

extern "C" int ea_batch_depth_gate(ea_batch *b, const double *b_T_a, const ea_depth_gate_params *prm, uint8_t *cls,
                                   int64_t capacity_rows, ea_depth_gate_stats *stats) {
  int rc = batch_depth_gate_checks(b, b_T_a, prm, cls, capacity_rows);
  if (rc != EA_OK) return rc;
  BatchView v;
  if ((rc = depth_gate_prepare(b, prm, &v)) != EA_OK) return rc;
  return depth_gate_to_host(b, v, b_T_a, prm, v.total_rows, cls, stats);
}

extern "C" int ea_problem_depth_gate(ea_problem *p, const double b_T_a[16], const ea_depth_gate_params *prm, uint8_t *cls,
                                     int64_t capacity, ea_depth_gate_stats *stats) {
  if (!p || !b_T_a || !prm || !stats) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = depth_gate_params_check(prm);
  if (rc == EA_OK) rc = check_reproject_poses(b_T_a, 1);
  if (rc != EA_OK) return rc;
  if (cls && capacity < p->n) return fail(EA_ERR_INVALID_ARG, "capacity is smaller than ea_problem_num_points");
  if ((rc = require_device()) != EA_OK) return rc;
  ea_batch *b;
  BatchView v;
  if ((rc = problem_call_batch(p, &b, false)) != EA_OK) return rc;  // (depth_gate_prepare builds, behind its own checks)
  if ((rc = depth_gate_prepare(b, prm, &v)) != EA_OK) return rc;
  std::vector<uint8_t> tmp(cls && !p->order.empty() ? (size_t)p->n : 0);  // (tile order: by way of tmp)
  rc = depth_gate_to_host(b, v, b_T_a, prm, p->n, tmp.empty() ? cls : tmp.data(), stats);  // (the head family's rows start at 0)
  if (rc == EA_OK && cls) scatter_to_callers_order(p->order, 1, tmp.data(), cls);
  return rc;
}

// ---- point selection (ea_point_select.h; kernels: ea_point_select_*_kernel) -------------------------------------------------
//
// One segment per problem of the call: its own points, read where the problem holds them -- no descriptor is needed, so the
// batch is not built and a problem needs a DT image only for the extent of the cell step.  The survivors are written out of
// place into arrays sized for the points there are (known without a wait), which replace the problem's after the call's ONE
// synchronisation; the old ones go back to the cache.  The weights keep living behind z (ea_capi_internal.h: w_off).
extern "C" void ea_default_point_selection(ea_point_selection *prm) {
  if (!prm) return;
  std::memset(prm, 0, sizeof(*prm));
  prm->cell_rule = EA_CELL_FIRST;
  prm->stride = 1;
}

namespace {
// the new arrays of one problem until the problem takes them
struct SelectedArrays {
  void *x = nullptr, *y = nullptr, *z = nullptr;
  size_t cap = 0;
  int64_t w_off = 0;
  SelectedArrays() = default;
  SelectedArrays(const SelectedArrays &) = delete;
  SelectedArrays(SelectedArrays &&o) noexcept : x(o.x), y(o.y), z(o.z), cap(o.cap), w_off(o.w_off) { o.x = o.y = o.z = nullptr; }
  ~SelectedArrays() { drop(); }
  void drop() {
    if (x) cached_free(x);
    if (y) cached_free(y);
    if (z) cached_free(z);
    x = y = z = nullptr;
  }
};
}  // namespace

// the layout of reserve_points: [z: cap bytes, rounded up to 256 | w: cap bytes]
static int selected_arrays_take(SelectedArrays &a, int64_t n, size_t esz, int device) {
  a.cap = (size_t)n * esz;
  const size_t z_bytes = (a.cap + 255) & ~(size_t)255;
  HIPCHK(cached_malloc(&a.x, a.cap, device));
  HIPCHK(cached_malloc(&a.y, a.cap, device));
  HIPCHK(cached_malloc(&a.z, z_bytes + a.cap, device));
  a.w_off = (int64_t)(z_bytes / esz);
  return EA_OK;
}

static int batch_select_points(ea_batch *b, const int *sel, int nsel, const ea_point_selection *prm, ea_point_selection_stats *stats) {
  const BatchView v = batch_view(b);
  if (!sel) nsel = v.count;
  if (nsel < 0) return fail(EA_ERR_INVALID_ARG, "nsel must be >= 0");
  std::vector<ea_problem *> probs((size_t)nsel);
  for (int j = 0; j < nsel; ++j) {
    const int i = sel ? sel[j] : j;
    if (i < 0 || i >= v.count) return fail(EA_ERR_INVALID_ARG, "sel: no such problem in the batch");
    probs[(size_t)j] = v.probs[i];
  }
  {
    std::vector<const ea_problem *> sorted(probs.begin(), probs.end());
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
      return fail(EA_ERR_INVALID_ARG, "the same problem twice in one selection: its points can be replaced once per call");
  }
  int rc = check_segment_count((size_t)nsel, "point selection");
  if (rc != EA_OK) return rc;
  // what the problems must be, read off the problems themselves: nothing has touched a device or changed a problem yet
  std::vector<int> ext_h((size_t)nsel, 0), ext_w((size_t)nsel, 0);
  for (int j = 0; j < nsel; ++j) {
    const ea_problem *p = probs[(size_t)j];
    if (!p->order.empty())
      return fail(EA_ERR_STATE, "the points are held in a storage order (tiles): set them under ea_problem_set_point_order(p, 0) to select");
    if (prm->cell_px == 0) continue;
    const bool given = prm->height > 0;
    if (!given && !(p->d_dt && p->H > 0 && p->W > 0))
      return fail(EA_ERR_STATE, "cell_px > 0 needs an extent: height, width or a distance-transform image (ea_problem_set_dt)");
    ext_h[(size_t)j] = given ? prm->height : p->H;
    ext_w[(size_t)j] = given ? prm->width : p->W;
    if (point_selection_cells(prm->cell_px, ext_h[(size_t)j], ext_w[(size_t)j]) > kPointSelectMaxCells)
      return fail(EA_ERR_INVALID_ARG, "more than 2^26 cells");
  }
  if (point_selection_is_identity(prm)) {
    for (int j = 0; stats && j < nsel; ++j) {
      const int64_t n = probs[(size_t)j]->n;
      stats[j] = ea_point_selection_stats{n, 0, n, n, 1};
    }
    return EA_OK;
  }
  int max_n = 0;
  for (const ea_problem *p : probs) max_n = std::max(max_n, (int)p->n);
  if (max_n == 0) {
    for (int j = 0; stats && j < nsel; ++j) stats[j] = ea_point_selection_stats{0, 0, 0, 0, 1};
    return EA_OK;
  }
  if ((rc = require_device()) != EA_OK) return rc;
  HIPCHK(hipSetDevice(v.device));
  const size_t esz = v.dtype == EA_F32 ? 4 : 8;
  const bool nearest = prm->cell_px > 0 && prm->cell_rule == EA_CELL_NEAREST;
  // the work block: [z tables (NEAREST) | index tables | block counts], one of each per segment
  std::vector<size_t> cells((size_t)nsel, 0), blocks((size_t)nsel, 0);
  size_t total_cells = 0, total_blocks = 0;
  for (int j = 0; j < nsel; ++j) {
    const ea_problem *p = probs[(size_t)j];
    if (p->n == 0) continue;
    if (prm->cell_px > 0) cells[(size_t)j] = (size_t)point_selection_cells(prm->cell_px, ext_h[(size_t)j], ext_w[(size_t)j]);
    blocks[(size_t)j] = (size_t)((p->n + kPointSelectThreads - 1) / kPointSelectThreads);
    total_cells += cells[(size_t)j]; total_blocks += blocks[(size_t)j];
  }
  const size_t o_imin = nearest ? total_cells * sizeof(unsigned long long) : 0;
  const size_t table_bytes = o_imin + total_cells * sizeof(unsigned int), o_counts = align16(table_bytes);
  DevBuf work;
  HIPCHK(cached_malloc(&work.p, o_counts + total_blocks * sizeof(int32_t), v.device));
  std::vector<SelectedArrays> fresh((size_t)nsel);
  SegmentBlock blk;
  const size_t bytes = blk.layout((size_t)nsel * sizeof(PointSelectSeg), (size_t)nsel * sizeof(PointSelectOut));
  HIPCHK(blk.take_pinned(bytes, v.device));
  std::memset(blk.pinned, 0, bytes);
  size_t at_cell = 0, at_block = 0;
  for (int j = 0; j < nsel; ++j) {
    const ea_problem *p = probs[(size_t)j];
    PointSelectSeg &sg = blk.records<PointSelectSeg>()[j];
    sg.n = (int32_t)p->n;
    if (p->n == 0) continue;
    SelectedArrays &a = fresh[(size_t)j];
    if ((rc = selected_arrays_take(a, p->n, esz, v.device)) != EA_OK) return rc;
    sg.x = p->d_x; sg.y = p->d_y; sg.z = p->d_z;
    sg.ox = a.x; sg.oy = a.y; sg.oz = a.z;
    sg.weighted = p->weighted ? 1 : 0;
    sg.w_in = p->weighted ? p->w_off : 0; sg.w_out = a.w_off;
    sg.fx = p->cam.fx; sg.fy = p->cam.fy; sg.cx = p->cam.cx; sg.cy = p->cam.cy;
    sg.height = ext_h[(size_t)j]; sg.width = ext_w[(size_t)j];
    if (prm->cell_px > 0) {
      sg.cells_x = select_cells_x(prm->cell_px, sg.width);
      sg.zmin = nearest ? work.as<unsigned long long>() + at_cell : nullptr;
      sg.imin = reinterpret_cast<unsigned int *>(work.as<unsigned char>() + o_imin) + at_cell;
    }
    sg.block_counts = reinterpret_cast<int32_t *>(work.as<unsigned char>() + o_counts) + at_block;
    at_cell += cells[(size_t)j]; at_block += blocks[(size_t)j];
  }
  HIPCHK(blk.take_device(bytes, v.device));
  HIPCHK(blk.up(v.stream));
  PointSelectWork w;
  w.nseg = nsel; w.max_n = max_n; w.cell_px = prm->cell_px; w.nearest = nearest ? 1 : 0; w.outside = prm->outside;
  w.stride = (unsigned int)std::min<int64_t>(prm->stride, 0x7fffffff);
  w.target = (unsigned int)std::min<int64_t>(prm->target, 0x7fffffff);
  w.segs = blk.dev_records<PointSelectSeg>();
  w.out = blk.dev_results<PointSelectOut>();
  w.tables = work.p; w.table_bytes = table_bytes;
  hipError_t e = launch_point_select(v.dtype, w, v.stream);
  if (e == hipSuccess) e = blk.down(v.stream);
  const hipError_t es = hipStreamSynchronize(v.stream);  // (nothing of the call stays in flight when the new arrays are dropped)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(EA_ERR_HIP, std::string("ea_batch_select_points: ") + hipGetErrorString(e));
  // the survivors become the problems' points
  for (int j = 0; j < nsel; ++j) {
    ea_problem *p = probs[(size_t)j];
    const PointSelectOut &o = blk.results<PointSelectOut>()[j];
    ea_point_selection_stats st{p->n, 0, 0, 0, 1};
    if (p->n > 0) {
      st.no_pixel = (int64_t)o.no_pixel;
      st.after_cells = (int64_t)o.after_cells;
      st.stride_used = select_stride_used(st.after_cells, prm->stride, prm->target);
      st.n_after = select_count_after(st.after_cells, st.stride_used);
      SelectedArrays &a = fresh[(size_t)j];
      if (st.n_after == 0) {  // (a problem without points holds no arrays and no weights)
        a.drop();
        (void)reserve_points(p, 0);
      } else {
        if (p->own_points) { cached_free(p->d_x); cached_free(p->d_y); cached_free(p->d_z); }
        p->d_x = a.x; p->d_y = a.y; p->d_z = a.z;
        a.x = a.y = a.z = nullptr;
        p->own_points = true;
        p->pts_cap = a.cap;
        p->w_off = a.w_off;
        p->n = st.n_after;
      }
      p->version++;
    }
    if (stats) stats[j] = st;
  }
  return EA_OK;
}

extern "C" int ea_batch_select_points(ea_batch *b, const int *sel, int nsel, const ea_point_selection *prm,
                                      ea_point_selection_stats *stats) {
  if (!b || !prm) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (const char *why = point_selection_error(prm)) return fail(EA_ERR_INVALID_ARG, why);
  return batch_select_points(b, sel, nsel, prm, stats);
}

extern "C" int ea_problem_select_points(ea_problem *p, const ea_point_selection *prm, ea_point_selection_stats *stats) {
  if (!prm) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (const char *why = point_selection_error(prm)) return fail(EA_ERR_INVALID_ARG, why);
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  ea_batch *b;
  int rc = problem_self_batch(p, &b);
  if (rc != EA_OK) return rc;
  return batch_select_points(b, nullptr, 1, prm, stats);
}

// ---- carrying points between frames (ea_point_merge.h; kernels: ea_point_transform_kernel, ea_point_merge_*_kernel) ---------
//
// Like point selection these calls read the points where the problems hold them and build no batch.  The transform rewrites
// the arrays in place; the merge writes dst's points and the carried ones out of place into arrays sized n_dst + n_src (known
// without a wait), which replace dst's after the call's ONE synchronisation.
extern "C" void ea_default_point_merge(ea_point_merge *prm) {
  if (!prm) return;
  std::memset(prm, 0, sizeof(*prm));
  prm->max_dt = -1.0;
  prm->cell_rule = EA_CELL_FIRST;
  prm->weight_scale = 1.0;
}

static const char *kStorageOrderMessage =
    "the points are held in a storage order (tiles): set them under ea_problem_set_point_order(p, 0) to select";

// the problems sel names, each at most once
static int selected_problems(const BatchView &v, const int *sel, int nsel, const char *twice, std::vector<ea_problem *> *probs) {
  if (nsel < 0) return fail(EA_ERR_INVALID_ARG, "nsel must be >= 0");
  probs->resize((size_t)nsel);
  for (int j = 0; j < nsel; ++j) {
    const int i = sel ? sel[j] : j;
    if (i < 0 || i >= v.count) return fail(EA_ERR_INVALID_ARG, "sel: no such problem in the batch");
    (*probs)[(size_t)j] = v.probs[i];
  }
  std::vector<const ea_problem *> sorted(probs->begin(), probs->end());
  std::sort(sorted.begin(), sorted.end());
  if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(EA_ERR_INVALID_ARG, twice);
  return EA_OK;
}

static int batch_transform_points(ea_batch *b, const int *sel, int nsel, const double *a_T_o) {
  const BatchView v = batch_view(b);
  if (!sel) nsel = v.count;
  std::vector<ea_problem *> probs;
  int rc = selected_problems(v, sel, nsel, "the same problem twice in one transform: chain two calls instead", &probs);
  if (rc != EA_OK) return rc;
  for (int j = 0; j < nsel; ++j)
    if (const char *why = point_transform_error(a_T_o + 16 * (size_t)j)) return fail(EA_ERR_INVALID_ARG, why);
  if ((rc = check_segment_count((size_t)nsel, "point transform")) != EA_OK) return rc;
  int max_n = 0;
  for (const ea_problem *p : probs) {
    if (!p->order.empty()) return fail(EA_ERR_STATE, kStorageOrderMessage);
    max_n = std::max(max_n, (int)p->n);
  }
  if (max_n == 0) return EA_OK;
  if ((rc = require_device()) != EA_OK) return rc;
  HIPCHK(hipSetDevice(v.device));
  for (ea_problem *p : probs)
    if ((rc = own_borrowed_points(p)) != EA_OK) return rc;
  SegmentBlock blk;
  const size_t bytes = blk.layout((size_t)nsel * sizeof(PointTransformSeg), 0);
  HIPCHK(blk.take_pinned(bytes, v.device));
  std::memset(blk.pinned, 0, bytes);
  for (int j = 0; j < nsel; ++j) {
    ea_problem *p = probs[(size_t)j];
    PointTransformSeg &sg = blk.records<PointTransformSeg>()[j];
    sg.x = p->d_x; sg.y = p->d_y; sg.z = p->d_z;
    sg.n = (int32_t)p->n;
    std::memcpy(sg.M, a_T_o + 16 * (size_t)j, sizeof(sg.M));
  }
  HIPCHK(blk.take_device(bytes, v.device));
  hipError_t e = blk.up(v.stream);
  if (e == hipSuccess) e = launch_point_transform(v.dtype, blk.dev_records<PointTransformSeg>(), nsel, max_n, v.stream);
  const hipError_t es = hipStreamSynchronize(v.stream);
  if (e == hipSuccess) e = es;
  for (ea_problem *p : probs)
    if (p->n > 0) p->version++;  // (also after a failure: the points may have been written)
  if (e != hipSuccess) return fail(EA_ERR_HIP, std::string("ea_batch_transform_points: ") + hipGetErrorString(e));
  return EA_OK;
}

extern "C" int ea_batch_transform_points(ea_batch *b, const int *sel, int nsel, const double *a_T_o) {
  if (!b || !a_T_o) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  return batch_transform_points(b, sel, nsel, a_T_o);
}

extern "C" int ea_problem_transform_points(ea_problem *p, const double a_T_o[16]) {
  if (!a_T_o) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (const char *why = point_transform_error(a_T_o)) return fail(EA_ERR_INVALID_ARG, why);
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  ea_batch *b;
  int rc = problem_self_batch(p, &b);
  if (rc != EA_OK) return rc;
  return batch_transform_points(b, nullptr, 1, a_T_o);
}

int ea::batch_merge_arrays(ea_batch *b, const int *sel, int nsel, const MergeSource *src, const double *dst_T_src,
                           const ea_point_merge *prm, ea_point_merge_stats *stats) {
  const BatchView v = batch_view(b);
  if (!sel) nsel = v.count;
  std::vector<ea_problem *> probs;
  int rc = selected_problems(v, sel, nsel, "the same dst twice in one merge: its points can be replaced once per call", &probs);
  if (rc != EA_OK) return rc;
  for (int j = 0; j < nsel; ++j)
    if (const char *why = point_transform_error(dst_T_src + 16 * (size_t)j)) return fail(EA_ERR_INVALID_ARG, why);
  if ((rc = check_segment_count((size_t)nsel, "point merge")) != EA_OK) return rc;
  // what the problems must be, read off the problems themselves: nothing has touched a device or changed a problem yet
  const bool need_pixel = point_merge_needs_pixel(prm), edge = prm->max_dt >= 0.0;
  std::vector<int> ext_h((size_t)nsel, 0), ext_w((size_t)nsel, 0);
  for (int j = 0; j < nsel; ++j) {
    const ea_problem *p = probs[(size_t)j];
    if (!p->order.empty()) return fail(EA_ERR_STATE, kStorageOrderMessage);
    if (p->n + src[j].n >= ((int64_t)1 << 31)) return fail(EA_ERR_INVALID_ARG, "dst and src together hold 2^31 points or more");
    if (!need_pixel) continue;
    const bool given = prm->height > 0, image = p->d_dt && p->H > 0 && p->W > 0;
    if (edge && !image) return fail(EA_ERR_STATE, "max_dt >= 0 needs dst's distance-transform image (ea_problem_set_dt)");
    if (!given && !image)
      return fail(EA_ERR_STATE, "the pixel test needs an extent: height, width or a distance-transform image (ea_problem_set_dt)");
    ext_h[(size_t)j] = given ? prm->height : p->H;
    ext_w[(size_t)j] = given ? prm->width : p->W;
    if (edge && (ext_h[(size_t)j] > p->H || ext_w[(size_t)j] > p->W))
      return fail(EA_ERR_INVALID_ARG, "max_dt >= 0: height x width must lie inside dst's distance-transform image");
    if (prm->cell_px > 0 && point_selection_cells(prm->cell_px, ext_h[(size_t)j], ext_w[(size_t)j]) > kPointSelectMaxCells)
      return fail(EA_ERR_INVALID_ARG, "more than 2^26 cells");
  }
  int max_dst = 0, max_src = 0;
  for (int j = 0; j < nsel; ++j) {
    const ea_problem *p = probs[(size_t)j];
    if (stats) stats[j] = ea_point_merge_stats{p->n, src[j].n, 0, 0, 0, 0, 0, 0, p->n};
    if (src[j].n == 0) continue;  // (nothing to carry: the segment launches nothing)
    max_dst = std::max(max_dst, (int)p->n);
    max_src = std::max(max_src, (int)src[j].n);
  }
  if (max_src == 0) return EA_OK;
  if ((rc = require_device()) != EA_OK) return rc;
  HIPCHK(hipSetDevice(v.device));
  const size_t esz = v.dtype == EA_F32 ? 4 : 8;
  const bool nearest = prm->cell_px > 0 && prm->cell_rule == EA_CELL_NEAREST;
  // the work block: [z tables (NEAREST) | index tables | occupancy bytes || block counts], one of each per segment
  std::vector<size_t> cells((size_t)nsel, 0), blocks((size_t)nsel, 0);
  size_t total_cells = 0, total_blocks = 0;
  for (int j = 0; j < nsel; ++j) {
    if (src[j].n == 0) continue;
    if (prm->cell_px > 0) cells[(size_t)j] = (size_t)point_selection_cells(prm->cell_px, ext_h[(size_t)j], ext_w[(size_t)j]);
    blocks[(size_t)j] = (size_t)((src[j].n + kPointMergeThreads - 1) / kPointMergeThreads);
    total_cells += cells[(size_t)j]; total_blocks += blocks[(size_t)j];
  }
  const size_t o_imin = nearest ? total_cells * sizeof(unsigned long long) : 0, o_occ = o_imin + total_cells * sizeof(unsigned int);
  const size_t table_bytes = o_occ + total_cells, o_counts = align16(table_bytes);
  DevBuf work;
  HIPCHK(cached_malloc(&work.p, o_counts + total_blocks * sizeof(int32_t), v.device));
  std::vector<SelectedArrays> fresh((size_t)nsel);
  SegmentBlock blk;
  const size_t o_scan_segs = align16((size_t)nsel * sizeof(PointMergeSeg)), o_scan_out = (size_t)nsel * sizeof(PointMergeOut);
  const size_t bytes = blk.layout(o_scan_segs + (size_t)nsel * sizeof(PointSelectSeg), o_scan_out + (size_t)nsel * sizeof(PointSelectOut));
  HIPCHK(blk.take_pinned(bytes, v.device));
  std::memset(blk.pinned, 0, bytes);
  PointSelectSeg *scan_segs = reinterpret_cast<PointSelectSeg *>(blk.pinned + o_scan_segs);
  size_t at_cell = 0, at_block = 0;
  for (int j = 0; j < nsel; ++j) {
    const ea_problem *p = probs[(size_t)j];
    const MergeSource &s = src[j];
    PointMergeSeg &sg = blk.records<PointMergeSeg>()[j];
    if (s.n == 0) continue;  // (n_dst = n_src = 0: every pass skips the segment)
    SelectedArrays &a = fresh[(size_t)j];
    if ((rc = selected_arrays_take(a, p->n + s.n, esz, v.device)) != EA_OK) return rc;
    sg.x = p->d_x; sg.y = p->d_y; sg.z = p->d_z;
    sg.sx = s.x; sg.sy = s.y; sg.sz = s.z;
    sg.ox = a.x; sg.oy = a.y; sg.oz = a.z;
    sg.n_dst = (int32_t)p->n; sg.n_src = (int32_t)s.n;
    sg.dst_weighted = p->weighted ? 1 : 0; sg.src_weighted = s.weighted ? 1 : 0;
    sg.out_weighted = merge_weighted(p->weighted, s.weighted, prm->weight_scale) ? 1 : 0;
    sg.w_dst = p->weighted ? p->w_off : 0; sg.w_src = s.weighted ? s.w_off : 0; sg.w_out = a.w_off;
    std::memcpy(sg.M, dst_T_src + 16 * (size_t)j, sizeof(sg.M));
    sg.fx = p->cam.fx; sg.fy = p->cam.fy; sg.cx = p->cam.cx; sg.cy = p->cam.cy;
    sg.height = ext_h[(size_t)j]; sg.width = ext_w[(size_t)j];
    if (edge) { sg.dt = p->d_dt; sg.pitch = p->pitch; }
    if (prm->cell_px > 0) {
      sg.cells_x = select_cells_x(prm->cell_px, sg.width);
      sg.zmin = nearest ? work.as<unsigned long long>() + at_cell : nullptr;
      sg.imin = reinterpret_cast<unsigned int *>(work.as<unsigned char>() + o_imin) + at_cell;
      sg.occ = work.as<unsigned char>() + o_occ + at_cell;
    }
    sg.block_counts = reinterpret_cast<int32_t *>(work.as<unsigned char>() + o_counts) + at_block;
    scan_segs[j].n = sg.n_src;
    scan_segs[j].block_counts = sg.block_counts;
    at_cell += cells[(size_t)j]; at_block += blocks[(size_t)j];
  }
  HIPCHK(blk.take_device(bytes, v.device));
  HIPCHK(blk.up(v.stream));
  PointMergeWork w;
  w.nseg = nsel; w.max_dst = max_dst; w.max_src = max_src;
  w.need_pixel = need_pixel ? 1 : 0; w.margin = prm->margin; w.max_dt = edge ? prm->max_dt : -1.0;
  w.cell_px = prm->cell_px; w.nearest = nearest ? 1 : 0; w.weight_scale = prm->weight_scale;
  w.cap = (unsigned int)std::min<int64_t>(prm->max_carried, 0x7fffffff);
  w.segs = blk.dev_records<PointMergeSeg>();
  w.out = blk.dev_results<PointMergeOut>();
  w.scan_segs = reinterpret_cast<const PointSelectSeg *>(blk.dev + o_scan_segs);
  w.scan_out = reinterpret_cast<PointSelectOut *>(blk.dev + blk.o_results + o_scan_out);
  w.tables = work.p; w.table_bytes = table_bytes;
  hipError_t e = launch_point_merge(v.dtype, w, v.stream);
  if (e == hipSuccess) e = blk.down(v.stream);
  const hipError_t es = hipStreamSynchronize(v.stream);  // (nothing of the call stays in flight when the new arrays are dropped)
  if (e == hipSuccess) e = es;
  if (e != hipSuccess) return fail(EA_ERR_HIP, std::string("ea_batch_merge_points: ") + hipGetErrorString(e));
  // dst's points and the carried ones become dst's points
  const PointSelectOut *scan_out = reinterpret_cast<const PointSelectOut *>(blk.pinned + blk.o_results + o_scan_out);
  for (int j = 0; j < nsel; ++j) {
    ea_problem *p = probs[(size_t)j];
    if (src[j].n == 0) continue;
    const PointMergeOut &o = blk.results<PointMergeOut>()[j];
    ea_point_merge_stats st{p->n, src[j].n, (int64_t)o.no_pixel, (int64_t)o.off_edge, (int64_t)o.occupied, (int64_t)o.lost_cell, 0, 0, 0};
    const int64_t survivors = (int64_t)scan_out[j].after_cells;
    st.carried = merge_carried(survivors, prm->max_carried);
    st.capped = survivors - st.carried;
    st.n_after = st.n_dst + st.carried;
    if (st.carried > 0) {
      SelectedArrays &a = fresh[(size_t)j];
      const bool weighted = merge_weighted(p->weighted, src[j].weighted, prm->weight_scale);
      if (p->own_points) { cached_free(p->d_x); cached_free(p->d_y); cached_free(p->d_z); }
      p->d_x = a.x; p->d_y = a.y; p->d_z = a.z;
      a.x = a.y = a.z = nullptr;
      p->own_points = true;
      p->pts_cap = a.cap;
      p->w_off = a.w_off;
      p->n = st.n_after;
      p->weighted = weighted;
      p->weights_from_depth = false;
      p->version++;
    }
    if (stats) stats[j] = st;
  }
  return EA_OK;
}

extern "C" int ea_batch_merge_points(ea_batch *dst, const int *sel, int nsel, ea_problem *const *src, const double *dst_T_src,
                                     const ea_point_merge *prm, ea_point_merge_stats *stats) {
  if (!prm) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (const char *why = point_merge_error(prm)) return fail(EA_ERR_INVALID_ARG, why);
  if (!dst || !src || !dst_T_src) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  const BatchView v = batch_view(dst);
  if (!sel) nsel = v.count;
  if (nsel < 0) return fail(EA_ERR_INVALID_ARG, "nsel must be >= 0");
  std::vector<MergeSource> from((size_t)nsel);
  for (int j = 0; j < nsel; ++j) {
    const ea_problem *s = src[j];
    if (!s) return fail(EA_ERR_INVALID_ARG, "NULL src problem");
    for (int k = 0; k < nsel; ++k) {
      const int i = sel ? sel[k] : k;
      if (i >= 0 && i < v.count && v.probs[i] == s)
        return fail(EA_ERR_INVALID_ARG, k == j ? "dst == src" : "a src problem is also a dst of the call");
    }
    if (s->dtype != v.dtype || s->device != v.device) return fail(EA_ERR_INVALID_ARG, "dst and src differ in dtype or device");
    if (!s->order.empty()) return fail(EA_ERR_STATE, kStorageOrderMessage);
    from[(size_t)j] = MergeSource{s->d_x, s->d_y, s->d_z, s->n, s->weighted ? s->w_off : 0, s->weighted};
  }
  return batch_merge_arrays(dst, sel, nsel, from.data(), dst_T_src, prm, stats);
}

extern "C" int ea_problem_merge_points(ea_problem *dst, const ea_problem *src, const double dst_T_src[16], const ea_point_merge *prm,
                                       ea_point_merge_stats *stats) {
  if (!prm || !dst_T_src) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (const char *why = point_merge_error(prm)) return fail(EA_ERR_INVALID_ARG, why);
  if (const char *why = point_transform_error(dst_T_src)) return fail(EA_ERR_INVALID_ARG, why);
  if (!dst || !src) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  if (dst == src) return fail(EA_ERR_INVALID_ARG, "dst == src");
  ea_batch *b;
  int rc = problem_self_batch(dst, &b);
  if (rc != EA_OK) return rc;
  ea_problem *from = const_cast<ea_problem *>(src);
  return ea_batch_merge_points(b, nullptr, 1, &from, dst_T_src, prm, stats);
}
