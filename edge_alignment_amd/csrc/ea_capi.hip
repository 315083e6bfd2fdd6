// ea_capi.hip — host driver behind include/ea_hip.h: HBM residency, tile lists, launches,
// the device-resident trust-region loop, and the measurement hooks (frame producers and tracker: ea_frames.hip; the calls that
// run one segment per problem: ea_segments.hip; what the three files share: ea_capi_internal.h).  No CPU compute fallback:
// without a gfx950 device every compute entry point returns EA_ERR_NO_DEVICE.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <utility>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/ea_hip.h"
#include "ea_capi_internal.h"
#include "ea_cov.h"
#include "ea_hip_dev.h"
#include "ea_launch.h"
#include "ea_lm.h"
#include "ea_poses_map.h"
#include "ea_prior.h"
#include "ea_search_rank.h"
#include "ea_spin.h"
#include "ea_starts_map.h"
#include "ea_types.h"

using namespace ea;

static thread_local std::string g_err;

int ea::fail(int code, const std::string &msg) {
  g_err = msg;
  return code;
}

// (ea_launch.h) for ea_comm.hip
extern "C" int ea_internal_fail(int code, const char *msg) { return fail(code, msg ? msg : ""); }

// scope guards for the temporaries of the measurement / test hooks, so that an early HIPCHK return frees them (DevBuf:
// ea_capi_internal.h)
namespace {
struct EventPair {
  hipEvent_t e0 = nullptr, e1 = nullptr;
  ~EventPair() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
  }
};
struct EventList {
  std::vector<hipEvent_t> ev;
  ~EventList() { for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e); }
};
}  // namespace


// ---- resource cache -----------------------------------------------------------------------------------------------
// A fresh problem's first solve used to cost 6 ms against 0.14 ms for the solve itself (scripts/archive/upload_probe.py): three
// hipMalloc for the points, one for the image, four hipMalloc + four hipHostMalloc + a stream for its batch, and the same
// number of frees -- each a driver call of 0.1-1 ms, hipFree also a device synchronisation.  That is what the ceres facade
// pays per ceres::Solve (one ea_problem per ceres::Problem, standalone_edge_align.cpp:256-293).  Freed device blocks,
// pinned host blocks and streams are therefore kept and handed out again: device blocks to any request they fit without
// wasting more than half, pinned blocks to requests of exactly their size and flags, streams to the next batch of the
// device.  Bounded (kCacheMaxBytes per kind, kCacheMaxEntries blocks); ea_release_cached_memory() returns everything
// to the driver.  hipFree used to synchronise the device implicitly; the cache keeps that guarantee explicitly: a recycled
// DEVICE block is handed out only after a device-wide drain that happened AFTER it was freed (one hipDeviceSynchronize --
// microseconds on a device that is idle or only holds the early-exit launches a finished solve left queued -- before the
// first reuse following any free; `stale`), so no launch enqueued on behalf of the previous owner can still touch it.
namespace {
struct CachedBlock { void *p; size_t bytes; int device; unsigned flags; };
struct ResourceCache {
  std::mutex mu;
  std::vector<CachedBlock> dev, pinned;
  std::vector<std::pair<int, hipStream_t>> streams;
  std::unordered_map<void *, CachedBlock> live;  // what is handed out (size / device / flags of a pointer)
  size_t dev_bytes = 0, pinned_bytes = 0;
  std::unordered_map<int, bool> stale;           // device -> a block was freed since the device was last drained
};
ResourceCache &cache() { static ResourceCache *c = new ResourceCache; return *c; }  // (never destroyed: frees at exit race the runtime's teardown)
constexpr size_t kCacheMaxBytes = (size_t)1 << 30;
constexpr size_t kCacheMaxEntries = 256;
void release_cached_memory_locked_free();
}  // namespace

hipError_t ea::cached_malloc(void **out, size_t bytes, int device) {
  *out = nullptr;
  if (bytes == 0) bytes = 256;
  bytes = (bytes + 255) & ~(size_t)255;
  ResourceCache &c = cache();
  {
    std::lock_guard<std::mutex> g(c.mu);
    size_t best = (size_t)-1;
    for (size_t i = 0; i < c.dev.size(); ++i)
      if (c.dev[i].device == device && c.dev[i].bytes >= bytes && c.dev[i].bytes <= 2 * bytes + 4096 &&
          (best == (size_t)-1 || c.dev[i].bytes < c.dev[best].bytes))
        best = i;
    if (best != (size_t)-1) {
      CachedBlock blk = c.dev[best];
      c.dev.erase(c.dev.begin() + (long)best);
      c.dev_bytes -= blk.bytes;
      c.live[blk.p] = blk;
      *out = blk.p;
      bool &stale = c.stale[device];
      if (stale) {
        // launches queued for the block's previous owner (on any stream) finish before the new owner sees it
        const hipError_t es = hipDeviceSynchronize();
        if (es != hipSuccess) return es;
        stale = false;
      }
      return hipSuccess;
    }
  }
  void *p = nullptr;
  hipError_t e = hipMalloc(&p, bytes);
  if (e != hipSuccess) {  // the cache may be what is in the way: give it back and try once more
    (void)hipGetLastError();
    release_cached_memory_locked_free();
    e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
  }
  std::lock_guard<std::mutex> g(c.mu);
  c.live[p] = CachedBlock{p, bytes, device, 0u};
  *out = p;
  return hipSuccess;
}

void ea::cached_free(void *p) {
  if (!p) return;
  ResourceCache &c = cache();
  CachedBlock blk{p, 0, -1, 0u};
  {
    std::lock_guard<std::mutex> g(c.mu);
    auto it = c.live.find(p);
    if (it != c.live.end()) {
      blk = it->second;
      c.live.erase(it);
      if (c.dev_bytes + blk.bytes <= kCacheMaxBytes && c.dev.size() < kCacheMaxEntries) {
        c.dev.push_back(blk);
        c.dev_bytes += blk.bytes;
        c.stale[blk.device] = true;
        return;
      }
    }
  }
  (void)hipFree(p);
}

hipError_t ea::cached_host_malloc(void **out, size_t bytes, unsigned flags, int device) {
  *out = nullptr;
  if (bytes == 0) bytes = 64;
  ResourceCache &c = cache();
  {
    std::lock_guard<std::mutex> g(c.mu);
    for (size_t i = 0; i < c.pinned.size(); ++i)
      if (c.pinned[i].bytes == bytes && c.pinned[i].flags == flags && c.pinned[i].device == device) {
        CachedBlock blk = c.pinned[i];
        c.pinned.erase(c.pinned.begin() + (long)i);
        c.pinned_bytes -= blk.bytes;
        c.live[blk.p] = blk;
        *out = blk.p;
        return hipSuccess;
      }
  }
  void *p = nullptr;
  const hipError_t e = hipHostMalloc(&p, bytes, flags);
  if (e != hipSuccess) return e;
  std::lock_guard<std::mutex> g(c.mu);
  c.live[p] = CachedBlock{p, bytes, device, flags};
  *out = p;
  return hipSuccess;
}

void ea::cached_host_free(void *p) {
  if (!p) return;
  ResourceCache &c = cache();
  {
    std::lock_guard<std::mutex> g(c.mu);
    auto it = c.live.find(p);
    if (it != c.live.end()) {
      const CachedBlock blk = it->second;
      c.live.erase(it);
      if (c.pinned_bytes + blk.bytes <= kCacheMaxBytes / 4 && c.pinned.size() < kCacheMaxEntries) {
        c.pinned.push_back(blk);
        c.pinned_bytes += blk.bytes;
        return;
      }
    }
  }
  (void)hipHostFree(p);
}

hipError_t ea::cached_stream_create(hipStream_t *out, int device) {
  ResourceCache &c = cache();
  {
    std::lock_guard<std::mutex> g(c.mu);
    for (size_t i = 0; i < c.streams.size(); ++i)
      if (c.streams[i].first == device) {
        *out = c.streams[i].second;
        c.streams.erase(c.streams.begin() + (long)i);
        return hipSuccess;
      }
  }
  return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}

void ea::cached_stream_destroy(hipStream_t s, int device) {  // (the caller has synchronised it)
  if (!s) return;
  ResourceCache &c = cache();
  {
    std::lock_guard<std::mutex> g(c.mu);
    if (c.streams.size() < 64) { c.streams.emplace_back(device, s); return; }
  }
  (void)hipStreamDestroy(s);
}

namespace {
void release_cached_memory_locked_free() {
  ResourceCache &c = cache();
  std::vector<CachedBlock> dev, pinned;
  std::vector<std::pair<int, hipStream_t>> streams;
  {
    std::lock_guard<std::mutex> g(c.mu);
    dev.swap(c.dev); pinned.swap(c.pinned); streams.swap(c.streams);
    c.dev_bytes = c.pinned_bytes = 0;
  }
  int cur = -1;
  if (hipGetDevice(&cur) != hipSuccess) cur = -1;
  for (const CachedBlock &b : dev) { (void)hipSetDevice(b.device); (void)hipFree(b.p); }
  for (const CachedBlock &b : pinned) (void)hipHostFree(b.p);
  for (auto &st : streams) { (void)hipSetDevice(st.first); (void)hipStreamDestroy(st.second); }
  if (cur >= 0) (void)hipSetDevice(cur);
  (void)hipGetLastError();
}
}  // namespace

extern "C" int ea_release_cached_memory(void) {
  release_cached_memory_locked_free();
  return EA_OK;
}

// one fold of a pose-batched call: the sequence number its completion raises the pinned flag to, and the poses it covers
struct KposesMark { int seq, start, g; };

constexpr int kPosesWaveExchangeDefault = 1;  // tuning key "poses_wave_exchange"
// tuning key "poses_lane_per_pose" at -1: the smallest K that takes one pose per lane.  Measured on C2 (98 rows, profiles/LOG.md):
// a launch of that kernel has rows x ceil(K / 64) workgroups, two resident per CU, so below ~1000 poses it does not fill the
// chip twice over and the other kernel is faster (K = 512: 0.89x); from 1024 on it is ahead.
constexpr int kPosesLanesFromK = 1024;
struct ea_batch {
  std::vector<ea_problem *> probs;
  std::vector<uint64_t> versions;
  int device = 0, dtype = EA_F64;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  // device
  // descriptors on the device: ONE block [ProblemDesc x nterms | GroupDesc x count], the layout of the staging block, so that a
  // build is one upload (a frame pair that changes its points / image every solve pays it every solve)
  unsigned char *d_desc_block = nullptr;
  ProblemDesc *d_probs = nullptr;       // one per term (problem + its additional terms), groups contiguous
  GroupDesc *d_groups = nullptr;         // one per problem (= pose); behind the terms of the current build
  // descriptors go up from a pinned staging block with asynchronous copies on the batch's stream (a frame pair that
  // changes its points / DT every solve would otherwise pay two blocking copies per solve)
  unsigned char *h_desc = nullptr;
  size_t h_desc_cap = 0;
  hipEvent_t desc_done = nullptr;
  int nterms = 0, terms_cap = 0;
  int any_variant = 0, terms_are_groups = 1;
  int weighted_terms = 0;  // terms of the current build with per-point weights (info key "weighted")
  int ntiles = 0, tiles_cap = 0;  // rows of the partial-sum array (one per workgroup with work)
  int chunk = 256, max_chunks = 0; // points per workgroup; largest per-problem workgroup count
  PoseState *d_poses = nullptr;
  double *d_partials = nullptr;
  EvalOut *d_out = nullptr;
  unsigned char *d_lm_block = nullptr;  // [PoseState x count | LMState x count | LMTrace x count]: poses + states go up
                                        // in ONE copy per solve, states + traces come back in ONE copy
  LMState *d_states = nullptr;
  LMCold *d_cold = nullptr;             // written by the first LM step before anything reads it
  LMTrace *d_traces = nullptr;
  int *d_progress = nullptr;            // device view of h_progress
  // pinned host mirrors
  PoseState *h_poses = nullptr;
  PoseState *dv_h_poses = nullptr;      // the device's view of h_poses: a lone evaluation of a few problems reads its poses from there
  int t_zero_copy = -1;                 // tuning key "zero_copy_poses": 0 = always upload the poses first (A/B)
  EvalOut *h_out = nullptr;
  EvalOut *dv_out = nullptr;            // the device's view of h_out: the synchronous evaluations fold straight into host memory
  // final delivery of a solve: [LMState x count | LMTrace x count] in pinned, device-mapped host memory, written by the
  // step kernel that ends a problem's solve (dv_* = the device's view of the same memory)
  unsigned char *h_deliver = nullptr;
  LMState *hd_states = nullptr, *dv_states = nullptr;
  LMTrace *hd_traces = nullptr, *dv_traces = nullptr;
  unsigned char *h_lm_block = nullptr;
  LMState *h_states = nullptr;
  LMTrace *h_traces = nullptr;
  int *h_progress = nullptr;            // pinned, device-visible: [running x count | evaluations started x count | steps complete x count | done flag]
  unsigned int *d_done_count = nullptr; // workgroups of the last fold of a synchronous evaluation that have delivered (ea_reduce_done_kernel)
  int done_seq = 0;                     // the value the flag takes when the current call's results have all landed
  int t_poll = 1;                       // tuning key "poll_results": 0 = wait for the stream's completion signal instead (A/B)
  // tuning (-1 = heuristic)
  int t_lds_bytes = -1, t_ppt = -1, t_use_lds = -1, t_xcd = -1, t_nt = -1, t_streams = -1, t_variant = 0;
  int t_wide = 0, wide = 0;              // "wide_accumulate": an fp32 kernel sums in fp64 from the lane's sum on (plain functor, L2 path)
  int ppt = 1, nt = 256, lds_bytes = 0, xcd_remap = 1;
  int t_test_fail_build = 0;  // test hook: the next descriptor build fails half-way, as a failed allocation would
  int t_test_stall_ms = 0;  // test hook: hold the stream on a host function for this long at the start of a solve
  int t_buf = -1, buffer_loads = 0;  // raw-buffer addressing of the DT image and the points (needs a < 2 GiB image)
  int t_img32 = -1, img32 = 0;       // fp64 batch whose kernels read the float32 mirror of the DT images ("dt_f32": -1 = when every
                                     // term has an exact mirror, 0 = never)
  std::vector<ea_batch *> parts;  // sub-batches of the concurrent solve (ea_batch_solve)
  bool built = false;
  hipEvent_t bench_e0 = nullptr, bench_e1 = nullptr;
  hipGraphExec_t bench_graph = nullptr;  // K x (evaluation + fold) captured once (ea_batch_bench_capture), replayed by
  int bench_riding_steps = 0;            // length of the last riding-fold sequence (captured or run launch by launch)
  int bench_graph_steps = 0;             // ea_batch_bench_steps(K): the timed region then holds no per-launch host work
  // ea_batch_bench_capture_pipelined: the fold of step k-1 rides in the launch of evaluation k; the evaluations alternate
  // between `bench_ring` = 2 row / result arrays
  int bench_ring = 0;
  double *d_bench_rows = nullptr;   // bench_ring x tiles_cap x kAccSlots
  EvalOut *d_bench_out = nullptr;   // bench_ring x count
  // ea_batch_set_poses / ea_batch_eval_resident_poses: K different poses per problem resident on the device, their K
  // evaluations + folds as one replayed hipGraph (the fold of evaluation k-1 rides in the launch of evaluation k), the K
  // results folded straight into pinned host memory
  int kp_K = 0, kp_cap = 0;                       // poses per problem resident / allocated
  double *h_kqt = nullptr, *d_kqt = nullptr;      // q, t staging: cap x count x 7 doubles (pinned / device)
  PoseState *d_kposes = nullptr;                  // cap x count
  EvalOut *h_kout = nullptr, *dv_kout = nullptr;  // cap x count, pinned + the device's view of it
  // G poses per launch: the descriptor / group tables replicated G times (copy g of a term owns the partial rows and the pose
  // slot of pose g) and the partial rows of G poses
  int kp_G = 0, t_kp_G = 0;   // (t_kp_G > 0: tuning key "poses_per_launch" caps G)
  // the launch shape of the pose-batched evaluation -- a throughput shape (more points per lane than the latency shape one
  // evaluation of the same batch takes) -- and the partial rows / widest term it implies per pose
  int kp_ppt = 1, kp_nt = 256, kp_chunk = 256, kp_ntiles = 0, kp_max_chunks = 0;
  unsigned char *d_kblock = nullptr;  // flat form: [PosesRow x rows | ProblemDesc x nterms | GroupDesc x count], the two below point into it
  ProblemDesc *d_kprobs = nullptr;
  GroupDesc *d_kgroups = nullptr;
  double *d_krows = nullptr;          // flat form: two arrays of kp_rows_cap poses each; grid form: one
  int kp_rows_cap = 0;
  int t_kp_order = -1;                // tuning key "poses_order": 1 = an XCD walks the rows of a pose instead of the poses of a row; -1 = the path's own (flat 0, lanes kPosesLanesOrder)
  int t_kp_xchg = kPosesWaveExchangeDefault, kp_xchg = 0, last_kp_xchg = 0;  // tuning key "poses_wave_exchange"; what kposes_shape made of it; what the last pose-batched launch ran
  // one pose per lane (ea_eval_poses_lanes_kernel): tuning key "poses_lane_per_pose" (-1 = from kPosesLanesFromK poses on, 0 =
  // never, N = from N poses on); what ea_batch_set_poses made of it for its K; what the last pose-batched call ran.  kp_Gc: the
  // launch size of the cost-only kernel, which keeps kposes_group's rule whatever the evaluation runs
  int t_kp_lanes = -1, kp_lanes = 0, last_kp_lanes = 0, kp_Gc = 0;
  std::vector<KposesMark> kp_marks;   // the folds of the last call: sequence number, first pose, poses (lanes path: one per group of the call)
  // the fold inside the lanes launches (ea_poses_map.h): run partials and counters of kl_groups_cap groups, and the pinned
  // flags of a call, one per (group of the call, problem), kl_flags_cap of them
  double *d_kparts = nullptr;
  unsigned int *d_kcount = nullptr;
  int *h_kflags = nullptr, *dv_kflags = nullptr;
  int kl_groups_cap = 0;
  size_t kl_flags_cap = 0;
  // ea_batch_cost_resident_poses: the narrow partials of one launch (kCostPartialBytes per row of a pose), tuning key
  // "cost_form" (0: always the fall-back, the full evaluation with only the cost fetched) and what the last call ran
  unsigned char *d_kcost = nullptr;
  size_t kcost_bytes = 0;
  int t_cost_form = 1, last_cost_form = 0;
  // one launch per LM iteration (ea_lm_iter_kernel): the second buffer of each pair a launch reads / writes -- states and cold
  // systems [LMState x count | LMCold x count] and partial rows -- beside d_states, d_cold, d_partials
  unsigned char *d_iter_alt = nullptr;
  int iter_alt_count = 0;
  double *d_partials_alt = nullptr;
  int tiles_cap_alt = 0;
  int t_fused = -1;             // tuning key "fused_iterations": -1 = whenever the solve qualifies, 0 = never (A/B, tests)
  int last_fused = 0;           // info key "fused_iterations": the last solve of this batch ran one launch per iteration
  bool needs_drain = false;     // a solve gave up on its deadline with launches still queued: synchronise before reuse
  const void *x0 = nullptr, *y0 = nullptr, *z0 = nullptr;  // problem 0's point arrays and count, handed to the evaluation
  int n0 = 0;                                              // kernel in its preloaded arguments
  GroupDesc group0 = {0, 0, 0, 0};  // host copy of d_groups[0]: handed to the step kernel by value
  GroupDesc *d_one_row = nullptr;  // {0, 1, 0, 1}: "one partial row" for the step kernel of ea_solve_sharded_device
  bool poses_uploaded = false;  // d_poses holds caller-supplied poses (ea_batch_bench_steps re-evaluates at them)
  bool poses_staged = false;    // h_poses holds the poses of the last ea_batch_eval, which the kernel read in place (not in d_poses yet)
  // materialised mode (ea_batch_eval_rows*): rows of all terms, in term order; library-owned output arrays on request
  int64_t total_rows = 0, max_n = 0;
  std::vector<int64_t> row_offsets;     // per problem (its terms are adjacent), count + 1 entries
  void *d_rows_r = nullptr, *d_rows_J = nullptr;
  int64_t rows_cap = 0;
  unsigned int *d_rows_invalid = nullptr;
  int t_rows_staged = -1, t_rows_nt = -1;
  // covariance (ea_batch_covariance): descriptors with the loss forced to trivial (apply_loss_function = 0) and the
  // results, written by the device into pinned host memory (dv_cov = the device's view of h_cov)
  unsigned char *h_cdesc = nullptr;
  ProblemDesc *d_cprobs = nullptr;
  int cdesc_cap = 0;
  ea_covariance *h_cov = nullptr, *dv_cov = nullptr;
  // NormalPriors: one PriorDesc per problem right behind the groups in d_desc_block (where the SIDE instantiations of the LM
  // kernels look for them), uploaded with them when any problem has one or holds tangent coordinates constant (PriorDesc::held
  // rides the same table, and the same instantiations apply the mask); any_side = 0: the prior-free instantiations run and
  // d_priors is NULL.  The host copy serves the results folded into host memory and the host-side state machine of
  // ea_solve_sharded.
  // (any_side / d_priors / h_priors: "side table" = whatever rides beside the groups; PriorDesc is its record and also
  // carries the mask -- held is kept twice on purpose: LMState::held is what the solve kernels read with the state they
  // fetch anyway, PriorDesc::held what ea_cov_kernel, which has no LMState, reads)
  PriorDesc *d_priors = nullptr;
  std::vector<PriorDesc> h_priors;
  int any_side = 0;  // ea_batch_solve_starts: K trust-region runs per problem in lock-step.  One device block [q, t x N | LMState x N | live list 0 |
  // alive | n_live pair, counter || live list 1 | PoseState x N | LMCold x N] (N = K x count slots; the part in front of || goes
  // up in one copy from the pinned staging block h_ms_up), the device trace rows when summaries are asked for, and the pinned,
  // device-mapped delivery block [the polled word | LMState x N | LMTrace x N]
  int ms_cap_slots = 0, ms_cap_K = 0;
  bool ms_has_traces = false;
  unsigned char *d_ms = nullptr, *h_ms_up = nullptr, *h_ms_dl = nullptr, *dv_ms_dl = nullptr;
  LMTrace *d_ms_traces = nullptr;
  unsigned ms_tag = 0;           // the tag of the last call's posts (ea_starts_map.h: starts_word)
  int last_starts_form = 0, last_starts_launches = 0;  // info keys "starts_form", "starts_launches"
  int t_starts_events = 0;       // tuning key "starts_events": an event pair around the call's queued launches (measurement)
  int last_starts_iterations = 0;
  int64_t last_starts_device_ns = 0;  // info keys "starts_iterations" (enqueued), "starts_device_ns" (0 without the events)
  // ea_batch_set_frames (ea_frames.hip): the batched producers' device block (count frame workspaces and the slot table) and
  // their pinned staging block (the table on its way up, the point counts on their way down); batch_frames_reserve
  unsigned char *d_frames = nullptr, *h_frames = nullptr;
  size_t frames_bytes = 0, h_frames_bytes = 0;
  int frames_rounds = 0;  // looks at the hysteresis flags of the last batched producer call (ea_batch_set_frames_canny / _ros; else 0)
  int frames_without_edges = 0;  // current frames without any edge in the last ea_batch_set_frames_ros call (else 0)
  int64_t frames_uploaded = 0;   // host-to-device frame copies of the last ea_batch_set_frames_ros_pyramid call led by this batch
  // ea_batch_depth_gate*: the segments and counters of a call, [DepthGateSeg x count | 6 counters x count], on the device and
  // in pinned memory; batch-owned and kept across calls, so that a call takes nothing from the allocator's cache (whose
  // reuse of a freed block drains the device first: a second wait)
  unsigned char *d_gate = nullptr, *h_gate = nullptr;
  size_t gate_bytes = 0;
};

int ea::check_device(int device) {
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess || cnt <= 0)
    return fail(EA_ERR_NO_DEVICE, "no HIP device available (libea_hip has no CPU fallback)");
  if (device < 0 || device >= cnt) return fail(EA_ERR_INVALID_ARG, "device index out of range");
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
    return fail(EA_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
  return EA_OK;
}

extern "C" const char *ea_last_error(void) { return g_err.c_str(); }

extern "C" void *ea_host_alloc(size_t bytes, int device) {
  if (bytes == 0) { fail(EA_ERR_INVALID_ARG, "ea_host_alloc: zero bytes"); return nullptr; }
  if (check_device(device) != EA_OK) return nullptr;
  void *p = nullptr;
  hipError_t e = hipSetDevice(device);
  if (e == hipSuccess) e = hipHostMalloc(&p, bytes, hipHostMallocPortable);
  if (e != hipSuccess) { fail(EA_ERR_ALLOC, std::string("ea_host_alloc: ") + hipGetErrorString(e)); return nullptr; }
  return p;
}

extern "C" void ea_host_free(void *p) {
  if (p) (void)hipHostFree(p);
}
extern "C" const char *ea_version(void) { return "edge_alignment_amd 0.2 (gfx950)"; }

extern "C" int ea_device_count(int *count) {
  if (!count) return fail(EA_ERR_INVALID_ARG, "count is NULL");
  int cnt = 0;
  hipError_t e = hipGetDeviceCount(&cnt);
  if (e != hipSuccess) { *count = 0; return fail(EA_ERR_NO_DEVICE, hipGetErrorString(e)); }
  int n950 = 0;
  for (int i = 0; i < cnt; ++i) {
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, i) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) ++n950;
  }
  *count = n950;
  return EA_OK;
}

extern "C" void ea_default_options(ea_options *o) {
  if (!o) return;
  o->max_num_iterations = 50;
  o->function_tolerance = 1e-6;
  o->gradient_tolerance = 1e-10;
  o->parameter_tolerance = 1e-8;
  o->initial_trust_region_radius = 1e4;
  o->max_trust_region_radius = 1e16;
  o->min_trust_region_radius = 1e-32;
  o->min_relative_decrease = 1e-3;
  o->min_lm_diagonal = 1e-6;
  o->max_lm_diagonal = 1e32;
  o->max_num_consecutive_invalid_steps = 5;
  o->jacobi_scaling = 1;
  o->strategy = EA_STRATEGY_LM;
  o->minimizer_progress_to_stdout = 0;
  o->iterations_per_sync = 0;
  o->solve_timeout_ms = 0.0;
}

// ceres::Solver::Options::IsValid for the fields carried here (solver.cc: OPTION_GE / OPTION_GT / OPTION_LE_OPTION);
// written so that a NaN fails every test.  Ceres ends such a Solve with FAILURE before touching the problem; the C-ABI
// returns EA_ERR_INVALID_ARG and leaves q, t and the summary alone.
int ea::check_options(const ea_options &o) {
  if (!(o.max_num_iterations >= 0)) return fail(EA_ERR_INVALID_ARG, "max_num_iterations < 0");
  if (o.strategy != EA_STRATEGY_LM && o.strategy != EA_STRATEGY_DOGLEG)
    return fail(EA_ERR_INVALID_ARG, "unknown trust-region strategy");
  if (!(o.function_tolerance >= 0.0) || !(o.gradient_tolerance >= 0.0) || !(o.parameter_tolerance >= 0.0))
    return fail(EA_ERR_INVALID_ARG, "tolerances must be >= 0");
  if (!(o.min_trust_region_radius > 0.0) || !(o.initial_trust_region_radius > 0.0) || !(o.max_trust_region_radius > 0.0) ||
      !(o.min_trust_region_radius <= o.initial_trust_region_radius) || !(o.initial_trust_region_radius <= o.max_trust_region_radius))
    return fail(EA_ERR_INVALID_ARG, "need 0 < min_trust_region_radius <= initial_trust_region_radius <= max_trust_region_radius");
  if (!(o.min_relative_decrease >= 0.0)) return fail(EA_ERR_INVALID_ARG, "min_relative_decrease < 0");
  if (!(o.min_lm_diagonal >= 0.0) || !(o.min_lm_diagonal <= o.max_lm_diagonal))
    return fail(EA_ERR_INVALID_ARG, "need 0 <= min_lm_diagonal <= max_lm_diagonal");
  if (!(o.max_num_consecutive_invalid_steps >= 0)) return fail(EA_ERR_INVALID_ARG, "max_num_consecutive_invalid_steps < 0");
  if (o.iterations_per_sync < 0) return fail(EA_ERR_INVALID_ARG, "iterations_per_sync < 0");
  if (o.solve_timeout_ms != o.solve_timeout_ms) return fail(EA_ERR_INVALID_ARG, "solve_timeout_ms is NaN");
  return EA_OK;
}

// ---- problem ------------------------------------------------------------------------------------

extern "C" int ea_problem_create(ea_problem **out, const ea_camera *cam, int dtype, int device) {
  if (!out || !cam) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (dtype != EA_F64 && dtype != EA_F32) return fail(EA_ERR_INVALID_ARG, "dtype must be EA_F64 or EA_F32");
  if (!(std::fabs(cam->fx) <= DBL_MAX) || !(std::fabs(cam->fy) <= DBL_MAX) || !(std::fabs(cam->cx) <= DBL_MAX) ||
      !(std::fabs(cam->cy) <= DBL_MAX) || cam->fx == 0.0 || cam->fy == 0.0)
    return fail(EA_ERR_INVALID_ARG, "camera intrinsics must be finite, focal lengths non-zero");
  int rc = check_device(device);
  if (rc != EA_OK) return rc;
  ea_problem *p = new (std::nothrow) ea_problem();
  if (!p) return fail(EA_ERR_ALLOC, "out of host memory");
  p->device = device;
  p->dtype = dtype;
  p->cam = *cam;
  *out = p;
  return EA_OK;
}

static void free_points(ea_problem *p) {
  if (p->own_points) {
    cached_free(p->d_x); cached_free(p->d_y); cached_free(p->d_z);
  }
  p->d_x = p->d_y = p->d_z = nullptr;
  p->own_points = false;
  p->pts_cap = 0;
  p->n = 0;
  p->order.clear();
  p->order_tile_used = 0;
  p->weighted = p->weights_from_depth = false;  // (the weights belong to the point set)
  p->w_off = 0;
}

// Room for n points in arrays the problem owns: the previous allocation when it is large enough (and not more than
// four times too large), a fresh one otherwise.  Leaves the problem without points (n = 0) and without weights either way.
// The block behind d_z has room for the weights too: [z: pts_cap bytes, rounded up to 256 | w: pts_cap bytes], so that a
// descriptor reaches them through a 32-bit element offset from z (ProblemDesc::w_off).
int ea::reserve_points(ea_problem *p, int64_t n) {
  const size_t esz = p->dtype == EA_F32 ? 4 : 8;
  const size_t need = (size_t)n * esz;
  if (p->own_points && p->pts_cap >= need && p->pts_cap <= 4 * need + 4096) {
    p->n = 0;
    p->order.clear();
    p->order_tile_used = 0;
    p->weighted = p->weights_from_depth = false;
    return EA_OK;
  }
  free_points(p);
  if (n == 0) return EA_OK;
  p->own_points = true;  // (before the allocations: a failure half-way leaves what was allocated to free_points)
  const size_t z_bytes = (need + 255) & ~(size_t)255;
  HIPCHK(cached_malloc(&p->d_x, need, p->device));
  HIPCHK(cached_malloc(&p->d_y, need, p->device));
  HIPCHK(cached_malloc(&p->d_z, z_bytes + need, p->device));
  p->pts_cap = need;
  p->w_off = (int64_t)(z_bytes / esz);
  return EA_OK;
}

// Storage order for large point sets: tiles of T x T pixels of the reference frame (the identity-pose projection),
// tiles in raster order, the caller's order inside a tile.  A wavefront's 64 points then sample a compact patch of
// the DT image instead of a 1-2 row strip across its whole width, and the four stencil-row loads of neighbouring
// points hit the lines the CU's L1 already holds (C5: 12.7 -> 8.1 us per evaluation, scripts/archive/order_sweep.py).
// Sums are taken in storage order; per-point outputs and ea_problem_get_points stay in the caller's order.
constexpr int64_t kAutoOrderPoints = 200000;  // below this a launch is latency-bound and the order does not matter

static void tile_order(const ea_problem *p, const double *xyz, int64_t n, int64_t stride, int tile,
                       std::vector<int32_t> &order) {
  std::vector<uint32_t> key((size_t)n);
  uint32_t max_tx = 0, max_ty = 0;
  const double inv = 1.0 / (double)tile;
  for (int64_t i = 0; i < n; ++i) {
    const double x = xyz[i * stride], y = xyz[i * stride + 1], z = xyz[i * stride + 2];
    double u = p->cam.fx * x / z + p->cam.cx, v = p->cam.fy * y / z + p->cam.cy;
    if (!(u >= 0.0)) u = 0.0;  // also NaN (z = 0)
    if (!(v >= 0.0)) v = 0.0;
    const uint32_t tx = (uint32_t)std::min(u * inv, 4095.0), ty = (uint32_t)std::min(v * inv, 4095.0);
    key[(size_t)i] = (ty << 12) | tx;
    max_tx = std::max(max_tx, tx); max_ty = std::max(max_ty, ty);
  }
  // stable counting sort on (ty, tx)
  const uint32_t nx = max_tx + 1, ny = max_ty + 1;
  std::vector<int64_t> head((size_t)nx * ny + 1, 0);
  for (int64_t i = 0; i < n; ++i) { const uint32_t k = key[(size_t)i]; head[(size_t)(k >> 12) * nx + (k & 4095) + 1]++; }
  for (size_t c = 1; c < head.size(); ++c) head[c] += head[c - 1];
  order.resize((size_t)n);
  for (int64_t i = 0; i < n; ++i) { const uint32_t k = key[(size_t)i]; order[(size_t)head[(size_t)(k >> 12) * nx + (k & 4095)]++] = (int32_t)i; }
}

extern "C" void ea_problem_destroy(ea_problem *p) {
  if (!p) return;
  (void)hipSetDevice(p->device);
  for (ea_problem *tm : p->terms) tm->term_of--;
  if (p->self) ea_batch_destroy(p->self);
  free_points(p);
  if (p->d_dt) cached_free(p->d_dt);
  if (p->d_dt32) cached_free(p->d_dt32);
  if (p->d_now_depth) cached_free(p->d_now_depth);
  if (p->ws) cached_free(p->ws);
  if (p->stage) cached_free(p->stage);
  delete p;
}

extern "C" int64_t ea_problem_num_points(const ea_problem *p) { return p ? p->n : 0; }

extern "C" int ea_problem_set_distortion(ea_problem *p, double k1, double k2, double p1, double p2, double k3) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!(std::fabs(k1) <= DBL_MAX) || !(std::fabs(k2) <= DBL_MAX) || !(std::fabs(p1) <= DBL_MAX) || !(std::fabs(p2) <= DBL_MAX) ||
      !(std::fabs(k3) <= DBL_MAX))
    return fail(EA_ERR_INVALID_ARG, "distortion coefficients must be finite");
  p->dist[0] = k1; p->dist[1] = k2; p->dist[2] = p1; p->dist[3] = p2; p->dist[4] = k3;
  const bool on = k1 != 0.0 || k2 != 0.0 || p1 != 0.0 || p2 != 0.0 || k3 != 0.0;
  p->variant = on ? (p->variant | 1) : (p->variant & ~1);
  p->version++;
  return EA_OK;
}

extern "C" int ea_problem_set_second_camera(ea_problem *p, const double trans_1to2[16], const double trans_1to2_inv[16]) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!trans_1to2 || !trans_1to2_inv) {  // back to the first camera
    for (int i = 0; i < 16; ++i) p->T12[i] = p->T12inv[i] = (i % 5 == 0) ? 1.0 : 0.0;
    p->variant &= ~2;
    p->version++;
    return EA_OK;
  }
  for (int k = 0; k < 2; ++k) {
    const double *m = k ? trans_1to2_inv : trans_1to2;
    if (m[12] != 0.0 || m[13] != 0.0 || m[14] != 0.0 || m[15] != 1.0)
      return fail(EA_ERR_INVALID_ARG, "rig transforms must be affine (last row 0 0 0 1)");
    for (int i = 0; i < 12; ++i)
      if (!(std::fabs(m[i]) <= DBL_MAX)) return fail(EA_ERR_INVALID_ARG, "rig transforms must be finite");
  }
  for (int i = 0; i < 16; ++i) { p->T12[i] = trans_1to2[i]; p->T12inv[i] = trans_1to2_inv[i]; }
  p->variant |= 2;
  p->version++;
  return EA_OK;
}

extern "C" int ea_problem_add_term(ea_problem *p, ea_problem *term) {
  if (!p || !term || p == term) return fail(EA_ERR_INVALID_ARG, "bad argument");
  if (!term->terms.empty()) return fail(EA_ERR_INVALID_ARG, "a term cannot have terms of its own");
  if (p->device != term->device || p->dtype != term->dtype) return fail(EA_ERR_INVALID_ARG, "terms must share device and dtype");
  if (std::find(p->terms.begin(), p->terms.end(), term) != p->terms.end()) return fail(EA_ERR_INVALID_ARG, "term already added");
  if (term->prior.has_q || term->prior.has_t)
    return fail(EA_ERR_INVALID_ARG, "a problem with a normal prior cannot be a term (the prior belongs on the head problem)");
  if (term->held)
    return fail(EA_ERR_INVALID_ARG, "a problem with constant parameters cannot be a term (the mask belongs on the head problem)");
  if (p->auto_factor > 0.0 || term->auto_factor > 0.0)
    return fail(EA_ERR_INVALID_ARG, "a problem with an auto-scaled loss cannot take terms or be one (ea_problem_set_loss_auto_scale)");
  p->terms.push_back(term);
  term->term_of++;
  p->version++;
  return EA_OK;
}

extern "C" int ea_problem_clear_terms(ea_problem *p) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  for (ea_problem *tm : p->terms) tm->term_of--;
  p->terms.clear();
  p->version++;
  return EA_OK;
}

// ceres::NormalPrior(A, b) on block 0 (q, n = 4) or 1 (t, n = 3): H = A^T A is formed here in fp64 and kept with b (ea_prior.h)
extern "C" int ea_problem_set_normal_prior(ea_problem *p, int block, const double *A, int k, const double *b) {
  // (the arguments are checked first, the problem last: every check here needs no device)
  if (block != 0 && block != 1) return fail(EA_ERR_INVALID_ARG, "block must be 0 (quaternion) or 1 (translation)");
  if (k < 0) return fail(EA_ERR_INVALID_ARG, "k must be >= 0");
  const bool clear = !A || k == 0;
  const int n = block == 0 ? 4 : 3;
  if (!clear) {
    if (!b) return fail(EA_ERR_INVALID_ARG, "b must not be NULL when A is given");
    for (int64_t i = 0; i < (int64_t)k * n; ++i)
      if (!(std::fabs(A[i]) <= DBL_MAX)) return fail(EA_ERR_INVALID_ARG, "A must be finite");
    for (int i = 0; i < n; ++i)
      if (!(std::fabs(b[i]) <= DBL_MAX)) return fail(EA_ERR_INVALID_ARG, "b must be finite");
  }
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  if (p->term_of > 0) return fail(EA_ERR_INVALID_ARG, "a problem that is a term cannot carry a normal prior");
  double H[16] = {0};
  if (!clear)
    for (int r = 0; r < k; ++r)
      for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) H[n * i + j] += A[(size_t)r * n + i] * A[(size_t)r * n + j];
  for (int i = 0; i < n * n; ++i)
    if (!(std::fabs(H[i]) <= DBL_MAX)) return fail(EA_ERR_INVALID_ARG, "A^T A overflows");
  PriorDesc &pr = p->prior;
  if (block == 0) {
    for (int i = 0; i < 16; ++i) pr.Hq[i] = H[i];
    for (int i = 0; i < 4; ++i) pr.bq[i] = clear ? 0.0 : b[i];
    pr.has_q = clear ? 0 : 1;
  } else {
    for (int i = 0; i < 9; ++i) pr.Ht[i] = H[i];
    for (int i = 0; i < 3; ++i) pr.bt[i] = clear ? 0.0 : b[i];
    pr.has_t = clear ? 0 : 1;
  }
  p->version++;
  return EA_OK;
}

// Problem::SetParameterBlockConstant / SubsetParameterization: the tangent coordinates a solve does not move and the
// covariance leaves out, in the solver's ordering [delta0 delta1 delta2 | tx ty tz].  Kept on the head problem like the prior.
extern "C" int ea_problem_set_constant_parameters(ea_problem *p, const int tangent_constant[6]) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  if (p->term_of > 0) return fail(EA_ERR_INVALID_ARG, "a problem that is a term cannot carry constant parameters");
  int held = 0;
  if (tangent_constant)
    for (int i = 0; i < 6; ++i) held |= tangent_constant[i] ? 1 << i : 0;
  p->held = held;
  p->version++;
  return EA_OK;
}

extern "C" int ea_problem_get_constant_parameters(const ea_problem *p, int tangent_constant[6]) {
  if (!p || !tangent_constant) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  for (int i = 0; i < 6; ++i) tangent_constant[i] = (p->held >> i) & 1;
  return EA_OK;
}

extern "C" int ea_problem_set_points(ea_problem *p, const double *xyz, int64_t n, int64_t stride) {
  if (!p || (n > 0 && !xyz)) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (n < 0 || n > 0x7fffff00LL) return fail(EA_ERR_INVALID_ARG, "n out of range");
  if (stride < 3) return fail(EA_ERR_INVALID_ARG, "stride_elems must be >= 3");
  HIPCHK(hipSetDevice(p->device));
  p->version++;
  if (n == 0) { free_points(p); return EA_OK; }
  const size_t esz = p->dtype == EA_F32 ? 4 : 8;
  const int tile = p->order_tile < 0 ? (n >= kAutoOrderPoints ? 16 : 0) : p->order_tile;
  if (tile == 0 && stride <= 8) {
    // the caller's order, compact AoS: the array goes up as it is (one copy) and is split into x[], y[], z[] of the
    // problem's dtype on the device -- no host pass over the points, one upload instead of three
    int rc = reserve_points(p, n);
    if (rc != EA_OK) return rc;
    const size_t raw = ((size_t)(n - 1) * (size_t)stride + 3) * sizeof(double);
    void *d_raw = nullptr;
    HIPCHK(cached_malloc(&d_raw, raw, p->device));
    hipError_t e = hipMemcpy(d_raw, xyz, raw, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_aos_to_soa(p->dtype, static_cast<const double *>(d_raw), n, (int)stride, p->d_x, p->d_y, p->d_z, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    cached_free(d_raw);
    if (e != hipSuccess) { free_points(p); return fail(EA_ERR_HIP, std::string("ea_problem_set_points: ") + hipGetErrorString(e)); }
    p->n = n;
    p->order.clear();
    p->order_tile_used = 0;
    return EA_OK;
  }
  std::vector<unsigned char> soa(3 * (size_t)n * esz);
  std::vector<int32_t> order;
  if (tile > 0) tile_order(p, xyz, n, stride, tile, order);
  const int32_t *ord = order.empty() ? nullptr : order.data();
  for (int c = 0; c < 3; ++c) {
    if (p->dtype == EA_F32) {
      float *dst = reinterpret_cast<float *>(soa.data()) + (size_t)c * n;
      for (int64_t i = 0; i < n; ++i) dst[i] = (float)xyz[(ord ? ord[i] : i) * stride + c];
    } else {
      double *dst = reinterpret_cast<double *>(soa.data()) + (size_t)c * n;
      for (int64_t i = 0; i < n; ++i) dst[i] = xyz[(ord ? ord[i] : i) * stride + c];
    }
  }
  {
    int rc = reserve_points(p, n);
    if (rc != EA_OK) return rc;
  }
  HIPCHK(hipMemcpy(p->d_x, soa.data(), n * esz, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p->d_y, soa.data() + (size_t)n * esz, n * esz, hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(p->d_z, soa.data() + 2 * (size_t)n * esz, n * esz, hipMemcpyHostToDevice));
  p->n = n;
  p->order.swap(order);
  p->order_tile_used = tile;
  return EA_OK;
}

extern "C" int ea_problem_get_point_order(const ea_problem *p, int *tile_px) {
  if (!p || !tile_px) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  *tile_px = p->order_tile_used;
  return EA_OK;
}

extern "C" int ea_problem_set_point_order(ea_problem *p, int tile_px) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (tile_px > 1024) return fail(EA_ERR_INVALID_ARG, "tile_px must be <= 1024 (0 = caller's order, < 0 = automatic)");
  p->order_tile = tile_px < 0 ? -1 : tile_px;
  return EA_OK;
}

extern "C" int ea_problem_set_points_device(ea_problem *p, const void *x, const void *y, const void *z, int64_t n) {
  if (!p || (n > 0 && (!x || !y || !z))) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (n < 0 || n > 0x7fffff00LL) return fail(EA_ERR_INVALID_ARG, "n out of range");
  HIPCHK(hipSetDevice(p->device));
  free_points(p);
  p->d_x = const_cast<void *>(x); p->d_y = const_cast<void *>(y); p->d_z = const_cast<void *>(z);
  p->own_points = false;
  p->n = n;
  p->version++;
  return EA_OK;
}

// ---- per-point weights (ceres::ScaledLoss per residual block) --------------------------------------------------------------

// borrowed point arrays (ea_problem_set_points_device) into arrays the problem owns: the weights live behind z.  Copied by a
// kernel: the caller's arrays may belong to another HIP runtime in the process (check_device_pointer), whose pointers this
// runtime's hipMemcpy does not know.
int ea::own_borrowed_points(ea_problem *p) {
  if (p->own_points || p->n == 0) return EA_OK;
  const void *x = p->d_x, *y = p->d_y, *z = p->d_z;
  const int64_t n = p->n;
  p->d_x = p->d_y = p->d_z = nullptr;
  int rc = reserve_points(p, n);
  if (rc == EA_OK) {
    const int same = p->dtype == EA_F64 ? 1 : 0;  // (source elements are the problem dtype)
    hipError_t e = launch_store_weights(p->dtype, same, x, nullptr, n, p->d_x, nullptr);
    if (e == hipSuccess) e = launch_store_weights(p->dtype, same, y, nullptr, n, p->d_y, nullptr);
    if (e == hipSuccess) e = launch_store_weights(p->dtype, same, z, nullptr, n, p->d_z, nullptr);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) rc = fail(EA_ERR_HIP, std::string("copying borrowed points: ") + hipGetErrorString(e));
  }
  if (rc != EA_OK) {  // back to the caller's arrays
    free_points(p);
    p->d_x = const_cast<void *>(x); p->d_y = const_cast<void *>(y); p->d_z = const_cast<void *>(z);
    p->n = n;
    return rc;
  }
  p->n = n;
  p->version++;
  return EA_OK;
}

// n weights in the caller's order at `src` (host doubles, or device values of the problem dtype) into the problem's storage:
// converted and permuted into the points' order by ea_store_weights_kernel
static int store_weights(ea_problem *p, const void *src, bool host_doubles) {
  const int64_t n = p->n;
  DevBuf raw, ord;
  if (host_doubles) {
    HIPCHK(cached_malloc(&raw.p, (size_t)n * sizeof(double), p->device));
    HIPCHK(hipMemcpy(raw.p, src, (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    src = raw.p;
  }
  if (!p->order.empty()) {
    HIPCHK(cached_malloc(&ord.p, (size_t)n * sizeof(int32_t), p->device));
    HIPCHK(hipMemcpy(ord.p, p->order.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice));
  }
  // (the staging above can fail without having touched the problem; only now do borrowed points become owned ones)
  int rc = own_borrowed_points(p);
  if (rc != EA_OK) return rc;
  HIPCHK(launch_store_weights(p->dtype, host_doubles || p->dtype == EA_F64, src, ord.as<int32_t>(), n, weights_ptr(p), nullptr));
  HIPCHK(hipDeviceSynchronize());
  p->weights_from_depth = false;
  if (!p->weighted) { p->weighted = true; p->version++; }  // (new values alone need no rebuild of a batch)
  return EA_OK;
}

extern "C" int ea_problem_set_weights(ea_problem *p, const double *w, int64_t n) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  if (!w) {
    if (p->weighted) { p->weighted = p->weights_from_depth = false; p->version++; }
    return EA_OK;
  }
  if (n != p->n) return fail(EA_ERR_INVALID_ARG, "n must equal the problem's number of points (ea_problem_num_points)");
  const double wmax = p->dtype == EA_F32 ? (double)FLT_MAX : DBL_MAX;
  for (int64_t i = 0; i < n; ++i)
    if (!(w[i] >= 0.0) || !(w[i] <= wmax)) return fail(EA_ERR_INVALID_ARG, "weights must be finite and >= 0");
  if (n == 0) return EA_OK;
  HIPCHK(hipSetDevice(p->device));
  return store_weights(p, w, true);
}

extern "C" int ea_problem_set_weights_device(ea_problem *p, const void *w, int64_t n) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  if (!w) return ea_problem_set_weights(p, nullptr, 0);
  if (n != p->n) return fail(EA_ERR_INVALID_ARG, "n must equal the problem's number of points (ea_problem_num_points)");
  if (n == 0) return EA_OK;
  HIPCHK(hipSetDevice(p->device));
  return store_weights(p, w, false);
}

extern "C" int ea_problem_get_weights(ea_problem *p, double *w, int64_t capacity, int64_t *count) {
  if (!p || !count) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  *count = 0;
  if (!p->weighted || p->n == 0) return EA_OK;
  if (!w) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (capacity < p->n) return fail(EA_ERR_INVALID_ARG, "capacity smaller than the number of points");
  HIPCHK(hipSetDevice(p->device));
  const size_t n = (size_t)p->n, esz = p->dtype == EA_F32 ? 4 : 8;
  std::vector<unsigned char> buf(n * esz);
  HIPCHK(hipMemcpy(buf.data(), weights_ptr(p), n * esz, hipMemcpyDeviceToHost));
  const int32_t *ord = p->order.empty() ? nullptr : p->order.data();
  for (size_t i = 0; i < n; ++i)
    w[ord ? (size_t)ord[i] : i] = p->dtype == EA_F32 ? (double)reinterpret_cast<float *>(buf.data())[i]
                                                     : reinterpret_cast<double *>(buf.data())[i];
  *count = p->n;
  return EA_OK;
}

extern "C" int ea_problem_set_depth_weighting(ea_problem *p, double z_ref, int power) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  if (power < 0 || power > 8) return fail(EA_ERR_INVALID_ARG, "power must be 0 (off) or 1..8");
  if (!(z_ref > 0.0) || !(z_ref <= DBL_MAX)) return fail(EA_ERR_INVALID_ARG, "z_ref must be finite and > 0");
  p->dw_z_ref = z_ref;
  p->dw_power = power;
  if (power == 0 && p->weighted && p->weights_from_depth) { p->weighted = p->weights_from_depth = false; p->version++; }
  return EA_OK;
}

int ea::alloc_dt(ea_problem *p, int W, int H) {
  p->W = W; p->H = H;
  p->pitch = (W + 2 * kImagePad + 3) & ~3;
  const size_t esz = p->dtype == EA_F32 ? 4 : 8;
  const size_t need = (size_t)p->pitch * (size_t)(H + 2 * kImagePad) * esz;
  p->dt32_exact = false;  // (until the call that fills the image says otherwise)
  if (p->dtype == EA_F64) {
    const size_t need32 = need / 2;
    if (!(p->d_dt32 && p->dt32_cap >= need32 && p->dt32_cap <= 4 * need32)) {
      if (p->d_dt32) { cached_free(p->d_dt32); p->d_dt32 = nullptr; p->dt32_cap = 0; }
      HIPCHK(cached_malloc(reinterpret_cast<void **>(&p->d_dt32), need32, p->device));
      p->dt32_cap = need32;
    }
  }
  if (p->d_dt && p->dt_cap >= need && p->dt_cap <= 4 * need) return EA_OK;  // same-size frame: keep the allocation
  if (p->d_dt) { cached_free(p->d_dt); p->d_dt = nullptr; p->dt_cap = 0; }
  HIPCHK(cached_malloc(&p->d_dt, need, p->device));
  p->dt_cap = need;
  return EA_OK;
}

// a device word for the "mirror is not exact" flag of the two upload paths, zeroed; freed by the caller
static int inexact_flag(ea_problem *p, int **flag) {
  *flag = nullptr;
  if (p->dtype != EA_F64) return EA_OK;
  HIPCHK(cached_malloc(reinterpret_cast<void **>(flag), sizeof(int), p->device));
  HIPCHK(hipMemsetAsync(*flag, 0, sizeof(int), nullptr));
  return EA_OK;
}

extern "C" int ea_problem_set_dt(ea_problem *p, const double *data, int grid_rows, int grid_cols) {
  if (!p || !data) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (grid_rows < 1 || grid_cols < 1 || grid_rows > 32768 || grid_cols > 32768)
    return fail(EA_ERR_INVALID_ARG, "grid extent out of range");
  HIPCHK(hipSetDevice(p->device));
  // Grid2D rows index u, cols index v (ref: standalone_edge_align.cpp:258, utils.h:77).
  const int W = grid_rows, H = grid_cols;
  int rc = alloc_dt(p, W, H);
  if (rc != EA_OK) return rc;
  // The grid goes up as it is (one contiguous copy) and is transposed, bordered and converted on the device: the host loop
  // this replaces read the caller's array with a stride of one grid row per element (0.28 -> 0.1x ms per 640 x 480 frame).
  const size_t raw = (size_t)W * (size_t)H * sizeof(double);
  void *d_raw = nullptr;
  int *d_inexact = nullptr;
  if ((rc = inexact_flag(p, &d_inexact)) != EA_OK) return rc;
  hipError_t e = cached_malloc(&d_raw, raw, p->device);
  if (e == hipSuccess) e = hipMemcpy(d_raw, data, raw, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = launch_grid_to_image(p->dtype, static_cast<const double *>(d_raw), W, H, p->d_dt, p->pitch, p->d_dt32, d_inexact, nullptr);
  int inexact = 1;
  if (e == hipSuccess && d_inexact) e = hipMemcpy(&inexact, d_inexact, sizeof(int), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  cached_free(d_raw);
  cached_free(d_inexact);
  if (e != hipSuccess) return fail(EA_ERR_HIP, std::string("ea_problem_set_dt: ") + hipGetErrorString(e));
  // every grid the reference builds comes out of a CV_32F distance transform (utils.cpp:79-82, cv2eigen at
  // standalone_edge_align.cpp:205-206): its doubles are floats, and the fp64 kernels may read the float mirror
  p->dt32_exact = d_inexact != nullptr && inexact == 0;
  p->version++;
  return EA_OK;
}

extern "C" int ea_problem_set_dt_image_device(ea_problem *p, const void *image, int height, int width) {
  if (!p || !image) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (height < 1 || width < 1 || height > 32768 || width > 32768)
    return fail(EA_ERR_INVALID_ARG, "image extent out of range");
  HIPCHK(hipSetDevice(p->device));
  int rc = alloc_dt(p, width, height);
  if (rc != EA_OK) return rc;
  int *d_inexact = nullptr;
  if ((rc = inexact_flag(p, &d_inexact)) != EA_OK) return rc;
  hipError_t e = launch_pad_image(p->dtype, image, height, width, p->d_dt, p->pitch, p->d_dt32, d_inexact, nullptr);
  int inexact = 1;
  if (e == hipSuccess && d_inexact) e = hipMemcpy(&inexact, d_inexact, sizeof(int), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  cached_free(d_inexact);
  if (e != hipSuccess) return fail(EA_ERR_HIP, std::string("ea_problem_set_dt_image_device: ") + hipGetErrorString(e));
  p->dt32_exact = d_inexact != nullptr && inexact == 0;
  p->version++;
  return EA_OK;
}

extern "C" int ea_problem_set_loss(ea_problem *p, int kind, double a) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (kind < EA_LOSS_TRIVIAL || kind > EA_LOSS_HUBER) return fail(EA_ERR_INVALID_ARG, "unknown loss kind");
  if (kind != EA_LOSS_TRIVIAL && !(a > 0.0)) return fail(EA_ERR_INVALID_ARG, "loss scale must be > 0");
  p->loss_kind = kind;
  p->loss_a = a;
  p->version++;
  return EA_OK;
}

extern "C" int ea_problem_get_loss(const ea_problem *p, int *kind, double *a) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (kind) *kind = p->loss_kind;
  if (a) *a = p->loss_a;
  return EA_OK;
}

// A loss scale taken from the data at the start of every solve (ea_batch_solve: auto_scale_losses); the arguments are
// checked first, the problem last: every check here needs no device
extern "C" int ea_problem_set_loss_auto_scale(ea_problem *p, double factor, double prob, double a_min) {
  if (!(std::fabs(factor) <= DBL_MAX) || factor < 0.0) return fail(EA_ERR_INVALID_ARG, "factor must be finite and >= 0 (0 = off)");
  if (!select_prob_ok(prob)) return fail(EA_ERR_INVALID_ARG, "prob must be in [0, 1]");
  if (!(a_min > 0.0) || !(a_min <= DBL_MAX)) return fail(EA_ERR_INVALID_ARG, "a_min must be finite and > 0");
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  if (factor > 0.0 && (p->term_of > 0 || !p->terms.empty()))
    return fail(EA_ERR_INVALID_ARG, "a problem that has terms or is a term cannot carry an auto-scaled loss");
  p->auto_factor = factor; p->auto_prob = prob; p->auto_a_min = a_min;
  return EA_OK;  // (no version bump: the descriptors do not change until a solve sets the loss)
}

extern "C" int ea_problem_get_loss_auto_scale(const ea_problem *p, double *factor, double *prob, double *a_min) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (factor) *factor = p->auto_factor;
  if (prob) *prob = p->auto_prob;
  if (a_min) *a_min = p->auto_a_min;
  return EA_OK;
}

extern "C" int ea_problem_set_flavour(ea_problem *p, double z_guard, double z_eps, int rot_transposed) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!(z_guard >= 0.0) || !(z_guard <= DBL_MAX) || !(std::fabs(z_eps) <= DBL_MAX))
    return fail(EA_ERR_INVALID_ARG, "z_guard must be >= 0, z_guard and z_eps finite");
  p->z_guard = z_guard; p->z_eps = z_eps; p->rot_transposed = rot_transposed ? 1 : 0;
  p->version++;
  return EA_OK;
}

// ---- batch --------------------------------------------------------------------------------------

static void bench_ring_free(ea_batch *b) {
  (void)hipFree(b->d_bench_rows); (void)hipFree(b->d_bench_out);
  b->d_bench_rows = nullptr; b->d_bench_out = nullptr; b->bench_ring = 0; b->bench_riding_steps = 0;
}

static void kposes_free_tables(ea_batch *b);
static bool kposes_flat(const ea_batch *b);

static void kposes_free(ea_batch *b) {
  kposes_free_tables(b);
  cached_free(b->d_kqt); cached_free(b->d_kposes);
  cached_host_free(b->h_kqt); cached_host_free(b->h_kout);
  b->d_kqt = nullptr; b->d_kposes = nullptr; b->h_kqt = nullptr; b->h_kout = nullptr; b->dv_kout = nullptr;
  b->kp_K = b->kp_cap = 0;
}

static void starts_free(ea_batch *b) {
  cached_free(b->d_ms); cached_free(b->d_ms_traces);
  cached_host_free(b->h_ms_up); cached_host_free(b->h_ms_dl);
  b->d_ms = nullptr; b->d_ms_traces = nullptr; b->h_ms_up = nullptr; b->h_ms_dl = nullptr; b->dv_ms_dl = nullptr;
  b->ms_cap_slots = b->ms_cap_K = 0; b->ms_has_traces = false;
}

static void batch_free_device(ea_batch *b) {
  kposes_free(b);
  starts_free(b);
  cached_free(b->d_frames); cached_host_free(b->h_frames);
  b->d_frames = b->h_frames = nullptr; b->frames_bytes = b->h_frames_bytes = 0;
  cached_free(b->d_gate); cached_host_free(b->h_gate);
  b->d_gate = b->h_gate = nullptr; b->gate_bytes = 0;
  cached_free(b->d_cprobs); cached_host_free(b->h_cdesc); cached_host_free(b->h_cov);
  b->d_cprobs = nullptr; b->h_cdesc = nullptr; b->cdesc_cap = 0; b->h_cov = nullptr; b->dv_cov = nullptr;
  (void)hipFree(b->d_rows_r); (void)hipFree(b->d_rows_J); (void)hipFree(b->d_rows_invalid);
  b->d_rows_r = b->d_rows_J = nullptr; b->d_rows_invalid = nullptr; b->rows_cap = 0;
  if (b->bench_graph) { (void)hipGraphExecDestroy(b->bench_graph); b->bench_graph = nullptr; b->bench_graph_steps = 0; b->bench_riding_steps = 0; }
  bench_ring_free(b);
  if (b->bench_e0) { (void)hipEventDestroy(b->bench_e0); b->bench_e0 = nullptr; }
  if (b->bench_e1) { (void)hipEventDestroy(b->bench_e1); b->bench_e1 = nullptr; }
  (void)hipFree(b->d_one_row); b->d_one_row = nullptr;
  cached_free(b->d_desc_block); cached_free(b->d_lm_block); cached_free(b->d_cold);
  b->d_desc_block = nullptr;
  cached_free(b->d_iter_alt); cached_free(b->d_partials_alt);
  b->d_iter_alt = nullptr; b->d_partials_alt = nullptr; b->iter_alt_count = 0; b->tiles_cap_alt = 0;
  cached_free(b->d_partials); cached_free(b->d_out); cached_free(b->d_done_count);
  b->d_done_count = nullptr;
  cached_host_free(b->h_lm_block); cached_host_free(b->h_out);
  cached_host_free(b->h_progress); cached_host_free(b->h_deliver);
  if (b->h_desc) cached_host_free(b->h_desc);
  if (b->desc_done) (void)hipEventDestroy(b->desc_done);
  b->h_desc = nullptr; b->h_desc_cap = 0; b->desc_done = nullptr;
  b->d_probs = nullptr; b->d_groups = nullptr; b->d_poses = nullptr; b->d_partials = nullptr; b->d_traces = nullptr; b->d_cold = nullptr; b->d_lm_block = nullptr;
  b->d_out = nullptr; b->d_states = nullptr; b->d_progress = nullptr;
  b->h_poses = nullptr; b->h_out = nullptr; b->dv_out = nullptr; b->h_states = nullptr; b->h_traces = nullptr; b->h_progress = nullptr;
  b->h_lm_block = nullptr; b->h_deliver = nullptr;
}

extern "C" int ea_batch_create(ea_batch **out, ea_problem *const *problems, int count) {
  if (!out || !problems || count < 1) return fail(EA_ERR_INVALID_ARG, "need at least one problem");
  for (int i = 0; i < count; ++i) {
    if (!problems[i]) return fail(EA_ERR_INVALID_ARG, "NULL problem in batch");
    if (problems[i]->device != problems[0]->device || problems[i]->dtype != problems[0]->dtype)
      return fail(EA_ERR_INVALID_ARG, "all problems of a batch must share device and dtype");
  }
  ea_batch *b = new (std::nothrow) ea_batch();
  if (!b) return fail(EA_ERR_ALLOC, "out of host memory");
  b->probs.assign(problems, problems + count);
  b->versions.assign(count, 0);
  b->device = problems[0]->device;
  b->dtype = problems[0]->dtype;
  hipError_t e = hipSetDevice(b->device);
  if (e == hipSuccess) e = cached_stream_create(&b->stream, b->device);
  if (e != hipSuccess) { delete b; return fail(EA_ERR_HIP, hipGetErrorString(e)); }
  b->own_stream = true;
  const size_t c = (size_t)count;
  const size_t lm_bytes = c * (sizeof(LMState) + sizeof(LMTrace) + sizeof(PoseState));
  e = cached_malloc(reinterpret_cast<void **>(&b->d_lm_block), lm_bytes, b->device);
  if (e == hipSuccess) e = cached_malloc(reinterpret_cast<void **>(&b->d_out), c * sizeof(EvalOut), b->device);
  if (e == hipSuccess) e = cached_malloc(reinterpret_cast<void **>(&b->d_cold), c * sizeof(LMCold), b->device);
  if (e == hipSuccess) e = cached_host_malloc(reinterpret_cast<void **>(&b->h_lm_block), lm_bytes, hipHostMallocDefault, b->device);
  if (e == hipSuccess) e = cached_host_malloc(reinterpret_cast<void **>(&b->h_out), c * sizeof(EvalOut), hipHostMallocMapped, b->device);
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&b->dv_out), b->h_out, 0);
  if (e == hipSuccess) e = cached_host_malloc(reinterpret_cast<void **>(&b->h_progress), (3 * c + 1) * sizeof(int), hipHostMallocMapped, b->device);
  if (e == hipSuccess) e = cached_malloc(reinterpret_cast<void **>(&b->d_done_count), 256, b->device);
  if (e == hipSuccess) e = hipMemsetAsync(b->d_done_count, 0, 256, b->stream);
  if (e == hipSuccess) b->h_progress[3 * c] = 0;
  if (e == hipSuccess) e = hipHostGetDevicePointer(reinterpret_cast<void **>(&b->d_progress), b->h_progress, 0);
  if (e == hipSuccess) e = cached_host_malloc(reinterpret_cast<void **>(&b->h_deliver), c * (sizeof(LMState) + sizeof(LMTrace)), hipHostMallocMapped, b->device);
  if (e == hipSuccess) {
    unsigned char *dv = nullptr;
    e = hipHostGetDevicePointer(reinterpret_cast<void **>(&dv), b->h_deliver, 0);
    b->hd_states = reinterpret_cast<LMState *>(b->h_deliver);
    b->hd_traces = reinterpret_cast<LMTrace *>(b->h_deliver + c * sizeof(LMState));
    b->dv_states = reinterpret_cast<LMState *>(dv);
    b->dv_traces = reinterpret_cast<LMTrace *>(dv + c * sizeof(LMState));
  }
  if (e == hipSuccess) {
    static_assert(sizeof(PoseState) % 8 == 0 && sizeof(LMState) % 8 == 0, "8-byte aligned sub-blocks");
    b->d_poses = reinterpret_cast<PoseState *>(b->d_lm_block);
    b->d_states = reinterpret_cast<LMState *>(b->d_lm_block + c * sizeof(PoseState));
    b->d_traces = reinterpret_cast<LMTrace *>(b->d_lm_block + c * (sizeof(PoseState) + sizeof(LMState)));
    b->h_poses = reinterpret_cast<PoseState *>(b->h_lm_block);
    if (hipHostGetDevicePointer(reinterpret_cast<void **>(&b->dv_h_poses), b->h_poses, 0) != hipSuccess) { b->dv_h_poses = nullptr; (void)hipGetLastError(); }
    b->h_states = reinterpret_cast<LMState *>(b->h_lm_block + c * sizeof(PoseState));
    b->h_traces = reinterpret_cast<LMTrace *>(b->h_lm_block + c * (sizeof(PoseState) + sizeof(LMState)));
  }
  if (e == hipSuccess) {  // traces and states are read back row by row: never hand out uninitialised memory
    // (on the batch's own stream: a null-stream memset is not ordered with this non-blocking stream and could land
    // after the first solve's upload -- states wiped to "not running", the host waiting for a flag nobody lowers)
    e = hipMemsetAsync(b->d_lm_block, 0, lm_bytes, b->stream);
    std::memset(b->h_lm_block, 0, lm_bytes);
    std::memset(b->h_deliver, 0, c * (sizeof(LMState) + sizeof(LMTrace)));
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(b->stream);
    batch_free_device(b);
    cached_stream_destroy(b->stream, b->device);
    delete b;
    return fail(EA_ERR_ALLOC, std::string("batch allocation: ") + hipGetErrorString(e));
  }
  *out = b;
  return EA_OK;
}

extern "C" void ea_batch_destroy(ea_batch *b) {
  if (!b) return;
  for (ea_batch *c : b->parts) ea_batch_destroy(c);
  b->parts.clear();
  (void)hipSetDevice(b->device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
  batch_free_device(b);
  if (b->own_stream && b->stream) cached_stream_destroy(b->stream, b->device);  // (synchronised above)
  for (ea_problem *p : b->probs)
    if (p && p->self == b) p->self = nullptr;
  delete b;
}

extern "C" int ea_batch_count(const ea_batch *b) { return b ? (int)b->probs.size() : 0; }
extern "C" void *ea_internal_batch_stream(ea_batch *b, int *device) {
  if (device) *device = b ? b->device : -1;
  return b ? (void *)b->stream : nullptr;
}

int ea::batch_frames_reserve(ea_batch *b, size_t device_bytes, size_t pinned_bytes, unsigned char **device_block,
                             unsigned char **pinned_block) {
  if (b->frames_bytes < device_bytes) {
    cached_free(b->d_frames);
    b->d_frames = nullptr; b->frames_bytes = 0;
    if (cached_malloc(reinterpret_cast<void **>(&b->d_frames), device_bytes, b->device) != hipSuccess) {
      (void)hipGetLastError();
      return fail(EA_ERR_ALLOC, "ea_batch_set_frames: no device memory for the frames' workspace");
    }
    b->frames_bytes = device_bytes;
  }
  if (b->h_frames_bytes < pinned_bytes) {
    cached_host_free(b->h_frames);
    b->h_frames = nullptr; b->h_frames_bytes = 0;
    if (cached_host_malloc(reinterpret_cast<void **>(&b->h_frames), pinned_bytes, hipHostMallocDefault, b->device) != hipSuccess) {
      (void)hipGetLastError();
      return fail(EA_ERR_ALLOC, "ea_batch_set_frames: no pinned memory for the frame table");
    }
    b->h_frames_bytes = pinned_bytes;
  }
  *device_block = b->d_frames;
  *pinned_block = b->h_frames;
  return EA_OK;
}

void ea::batch_frames_set_rounds(ea_batch *b, int rounds) { b->frames_rounds = rounds; }
void ea::batch_frames_set_without_edges(ea_batch *b, int frames) { b->frames_without_edges = frames; }
void ea::batch_frames_set_uploaded(ea_batch *b, int64_t copies) { b->frames_uploaded = copies; }

// (re)build descriptors and the tile list when any problem changed
static void fill_desc(const ea_problem *p, ProblemDesc &d) {
  std::memset(&d, 0, sizeof(d));
  d.x = p->d_x; d.y = p->d_y; d.z = p->d_z; d.dt = p->d_dt;
  d.dt32 = (p->dtype == EA_F64 && p->dt32_exact) ? p->d_dt32 : nullptr;
  d.n = (int32_t)p->n; d.W = p->W; d.H = p->H; d.pitch = p->pitch;
  d.fx = p->cam.fx; d.fy = p->cam.fy; d.cx = p->cam.cx; d.cy = p->cam.cy;
  d.loss_a = p->loss_a; d.z_guard = p->z_guard; d.z_eps = p->z_eps;
  d.fxf = (float)d.fx; d.fyf = (float)d.fy; d.cxf = (float)d.cx; d.cyf = (float)d.cy;
  d.loss_inv_b = 1.0 / (d.loss_a * d.loss_a); d.loss_inv_bf = (float)d.loss_inv_b;
  d.loss_af = (float)d.loss_a; d.z_guardf = (float)d.z_guard; d.z_epsf = (float)d.z_eps;
  d.loss_kind = p->loss_kind; d.rot_transposed = p->rot_transposed;
  d.variant = term_variant(p);
  d.w_off = p->weighted ? (int32_t)p->w_off : 0;
  for (int i = 0; i < 5; ++i) { d.dist[i] = p->dist[i]; d.distf[i] = (float)p->dist[i]; }
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) {
      d.A[3 * r + c] = p->T12[4 * r + c]; d.Ai[3 * r + c] = p->T12inv[4 * r + c];
      d.Af[3 * r + c] = (float)d.A[3 * r + c]; d.Aif[3 * r + c] = (float)d.Ai[3 * r + c];
    }
    d.d[r] = p->T12[4 * r + 3]; d.di[r] = p->T12inv[4 * r + 3];
    d.df[r] = (float)d.d[r]; d.dif[r] = (float)d.di[r];
  }
}

// (re)build descriptors when any problem (or one of its terms) changed
static int batch_build(ea_batch *b) {
  // every entry point that launches or allocates passes through here first: the calling thread's current device is the
  // batch's from now on (a process driving several GPUs may have switched between calls)
  HIPCHK(hipSetDevice(b->device));
  if (b->needs_drain) {  // launches of an abandoned solve may still be queued on (or stuck in) the stream
    HIPCHK(hipStreamSynchronize(b->stream));
    b->needs_drain = false;
  }
  uint64_t sig = 0;
  bool dirty = !b->built;
  for (size_t i = 0; i < b->probs.size(); ++i) {
    uint64_t v = b->probs[i]->version;
    for (ea_problem *tm : b->probs[i]->terms) v = v * 1000003u + tm->version + 17;
    if (b->versions[i] != v) dirty = true;
    sig += v;
  }
  (void)sig;
  if (!dirty) return EA_OK;
  b->built = false;  // until the last allocation and upload below has succeeded
  if (b->bench_graph) { (void)hipGraphExecDestroy(b->bench_graph); b->bench_graph = nullptr; b->bench_graph_steps = 0; b->bench_riding_steps = 0; }
  bench_ring_free(b);  // (sized by the row count of the old build)
  b->kp_K = 0;         // (resident pose states and the replicated tables were built for the old descriptors)
  b->kp_G = 0;
  // terms of a problem follow it; all share its pose
  std::vector<const ea_problem *> terms;
  std::vector<int> term_group;
  int64_t total = 0, max_n = 0;
  int any_variant = 0, weighted_terms = 0;
  for (size_t i = 0; i < b->probs.size(); ++i) {
    std::vector<const ea_problem *> fam;
    fam.push_back(b->probs[i]);
    for (ea_problem *tm : b->probs[i]->terms) fam.push_back(tm);
    for (const ea_problem *p : fam) {
      if (p->device != b->device || p->dtype != b->dtype) return fail(EA_ERR_INVALID_ARG, "terms must share device and dtype");
      if (!p->d_dt) return fail(EA_ERR_STATE, "distance-transform image not set (ea_problem_set_dt)");
      if (p->n > 0 && !p->d_x) return fail(EA_ERR_STATE, "edge points not set (ea_problem_set_points)");
      if (p->rot_transposed != b->probs[i]->rot_transposed) return fail(EA_ERR_INVALID_ARG, "terms of one problem must agree on rot_transposed");
      total += p->n;
      max_n = std::max<int64_t>(max_n, p->n);
      any_variant |= term_variant(p);
      weighted_terms += p->weighted ? 1 : 0;
      terms.push_back(p);
      term_group.push_back((int)i);
    }
  }
  any_variant |= b->t_variant;  // a part of a larger batch runs the kernel form the whole batch runs
  b->any_variant = any_variant;
  b->weighted_terms = weighted_terms;
  b->terms_are_groups = terms.size() == b->probs.size() ? 1 : 0;
  // Launch shape, measured on MI355X (profiles/r01_sweep*.txt, r02_single_shape_sweep.txt, r02_batch_shape_sweep.txt): what
  // counts is the (evaluate, fold) step and the LM iteration, i.e. the kernel AND the number of partial rows behind it.
  // Small problems are latency-bound: one point per lane and as many waves as possible.  From ~1e5 points two points
  // per lane cost the kernel nothing and halve the rows; larger clouds take 1024-thread workgroups (fp32: 2-4 points per
  // lane on top): the kernel time hardly moves, the rows drop to a few hundred.
  int nt_auto = 256, ppt_auto = 1;
  if (terms.size() == 1) {
    if (b->dtype == EA_F32) {
      if (max_n >= 800000) { nt_auto = 1024; ppt_auto = 4; }
      else if (max_n >= 300000) { nt_auto = 1024; ppt_auto = 2; }
      else if (max_n >= 150000) { nt_auto = 1024; ppt_auto = 1; }   // 2e5: step 6.3 us, against 6.7 at 256 x 4
      else if (max_n >= 80000) ppt_auto = 2;                        // 1e5: step 5.7 us / solve 159 us, against 6.3 / 177
    } else {
      // fp64 runs ONE 1024-thread workgroup per CU (128-VGPR budget): that shape pays when its workgroups fill whole
      // rounds of the 256 CUs (3.4e5 points = 1.33 rounds: 8.8 us against 6.0 us at 256 x 2)
      const int64_t wg1024 = (max_n + 1023) / 1024, rounds = (wg1024 + 255) / 256;
      if (max_n >= 150000 && (rounds == 1 || wg1024 * 4 >= rounds * 256 * 3)) nt_auto = 1024;
      else if (max_n >= 80000) ppt_auto = 2;
    }
  } else if (b->dtype == EA_F32) {
    if (max_n >= 800000) { nt_auto = 1024; ppt_auto = 4; }
    else if (max_n >= 300000) { nt_auto = 1024; ppt_auto = 2; }
    else if (max_n >= 150000) { nt_auto = 256; ppt_auto = 4; }
    else {
      // batches of small problems: one point per lane (latency-bound up to ~32 pairs; in raster order two points per lane
      // cost 4-6 % at every size) -- except large batches stored tile by tile, where two points per lane halve the
      // butterfly per point and still read neighbouring texels: 64 x 50k 23.5 -> 21.4 us, 128 x 50k 47.7 -> 41.3 us
      // (0.63 -> 0.69 / 0.71 of the HBM roofline; profiles/r02_batch_shape_sweep.txt)
      bool all_tiled = true;
      for (const ea_problem *p : terms) all_tiled = all_tiled && p->order_tile_used > 0;
      ppt_auto = (all_tiled && total >= 2400000) ? 2 : 1;
    }
  } else {
    ppt_auto = total >= 80000 ? 2 : 1;  // same kernel time at 1e5 points, half the rows for the LM step to fold
  }
  if (terms.size() == 1 && b->t_fused != 0 && !any_variant) {
    // A single problem whose evaluation fits one workgroup per CU can run one launch per LM iteration (ea_lm_iter_kernel:
    // 256-thread workgroups, at most 255 chunks + the writer), which beats every pair-form shape measured
    // (profiles/r03_ab_fused_shapes.txt: fp64 7e4 points 13.1 -> 11.9 us per iteration, fp32 2e5 points 12.6 -> 12.0): take
    // the fewest points per lane that fit.
    const int max_ppt = b->dtype == EA_F32 ? 4 : 2;
    for (int pp = 1; pp <= max_ppt; pp *= 2)
      if ((max_n + 256 * pp - 1) / (256 * pp) <= 255) { nt_auto = 256; ppt_auto = pp; break; }
  }
  int nt = (b->t_nt == 1024 || b->t_nt == 256) ? b->t_nt : nt_auto;
  int ppt = b->t_ppt;
  if (ppt != 1 && ppt != 2 && ppt != 4) ppt = ppt_auto;
  // the variant kernel is built for this shape only -- first, so that a request for 1024 threads, which it cannot honour,
  // does not cost an fp64 batch its second point per lane through the rule below
  if (any_variant) { nt = 256; ppt = std::min(ppt, 2); }
  if (nt == 1024 && b->dtype == EA_F64) ppt = 1;  // 128-VGPR budget at 16 waves/CU
  if (b->dtype == EA_F64 && ppt > 2) ppt = 2;
  // raw-buffer addressing (32-bit byte offsets into the image): on unless an image reaches 2 GiB
  int buffer_loads = b->t_buf >= 0 ? (b->t_buf ? 1 : 0) : 1;
  for (const ea_problem *p : terms)
    if ((size_t)p->pitch * (size_t)(p->H + 2 * kImagePad) * (b->dtype == EA_F32 ? 4 : 8) >= ((size_t)1 << 31)) buffer_loads = 0;
  b->buffer_loads = buffer_loads;
  b->ppt = ppt;
  b->nt = nt;
  const int64_t chunk = (int64_t)nt * ppt;
  b->chunk = (int)chunk;
  std::vector<ProblemDesc> descs(terms.size());
  std::vector<GroupDesc> groups(b->probs.size());
  int rows = 0, max_chunks = 0;
  int64_t row_begin = 0;
  std::vector<int64_t> row_offsets(b->probs.size() + 1, 0);
  for (size_t k = 0; k < terms.size(); ++k) {
    const ea_problem *p = terms[k];
    ProblemDesc &d = descs[k];
    fill_desc(p, d);
    d.group = term_group[k];
    d.row_begin = row_begin;
    if (k == 0 || term_group[k - 1] != term_group[k]) row_offsets[(size_t)term_group[k]] = row_begin;
    row_begin += p->n;
    const int nchunks = (int)((p->n + chunk - 1) / chunk);
    d.tile_begin = rows;
    rows += nchunks;
    d.tile_end = rows;
    max_chunks = std::max(max_chunks, nchunks);
    GroupDesc &g = groups[term_group[k]];
    if (k == 0 || term_group[k - 1] != term_group[k]) { g.tile_begin = d.tile_begin; g.term_begin = (int)k; }
    g.tile_end = d.tile_end;
    g.term_end = (int)k + 1;
  }
  b->nterms = (int)terms.size();
  b->group0 = groups.empty() ? GroupDesc{0, 0, 0, 0} : groups[0];
  if (!descs.empty()) { b->x0 = descs[0].x; b->y0 = descs[0].y; b->z0 = descs[0].z; b->n0 = descs[0].n; }
  else { b->x0 = b->y0 = b->z0 = nullptr; b->n0 = 0; }
  b->ntiles = rows;
  b->max_chunks = max_chunks;
  row_offsets[b->probs.size()] = row_begin;
  b->row_offsets = row_offsets;
  b->total_rows = row_begin;
  b->max_n = max_n;
  if (b->nterms > b->terms_cap || !b->d_desc_block) {
    cached_free(b->d_desc_block);
    b->d_desc_block = nullptr; b->d_probs = nullptr; b->d_groups = nullptr;
    b->terms_cap = b->nterms + 8;
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_desc_block),
                         (size_t)b->terms_cap * sizeof(ProblemDesc) + b->probs.size() * (sizeof(GroupDesc) + sizeof(PriorDesc)),
                         b->device));
  }
  static_assert(sizeof(ProblemDesc) % alignof(GroupDesc) == 0, "the groups sit right behind the terms");
  b->d_probs = reinterpret_cast<ProblemDesc *>(b->d_desc_block);
  b->d_groups = reinterpret_cast<GroupDesc *>(b->d_desc_block + (size_t)b->nterms * sizeof(ProblemDesc));
  b->h_priors.resize(b->probs.size());
  b->any_side = 0;
  for (size_t i = 0; i < b->probs.size(); ++i) {
    b->h_priors[i] = b->probs[i]->prior;
    b->h_priors[i].held = b->probs[i]->held;  // (the table's other passenger: constant tangent coordinates)
    b->any_side |= (b->h_priors[i].has_q || b->h_priors[i].has_t || b->h_priors[i].held) ? 1 : 0;
  }
  static_assert(sizeof(GroupDesc) % alignof(PriorDesc) == 0, "the priors sit right behind the groups");
  b->d_priors = b->any_side ? reinterpret_cast<PriorDesc *>(b->d_groups + b->probs.size()) : nullptr;
  if (b->t_test_fail_build) {  // (tests/test_gpu_robustness.py: a build that fails here must leave the batch dirty)
    b->t_test_fail_build = 0;
    return fail(EA_ERR_ALLOC, "batch build: injected allocation failure (test hook)");
  }
  if (b->ntiles > b->tiles_cap) {
    cached_free(b->d_partials);
    b->d_partials = nullptr;
    b->tiles_cap = b->ntiles + b->ntiles / 4 + 16;
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_partials), (size_t)b->tiles_cap * kAccSlots * sizeof(double), b->device));
    // (stream-ordered on the batch's own stream: a null-stream memset is not ordered with a non-blocking stream and may
    // land after the first evaluation has written its rows)
    HIPCHK(hipMemsetAsync(b->d_partials, 0, (size_t)b->tiles_cap * kAccSlots * sizeof(double), b->stream));
  }
  {
    const size_t pb = descs.size() * sizeof(ProblemDesc), gb = groups.size() * sizeof(GroupDesc);
    const size_t rb = b->any_side ? b->h_priors.size() * sizeof(PriorDesc) : 0;
    if (!b->desc_done) HIPCHK(hipEventCreateWithFlags(&b->desc_done, hipEventDisableTiming));
    else HIPCHK(hipEventSynchronize(b->desc_done));  // the staging block is free again (it always is by now)
    if (b->h_desc_cap < pb + gb + rb) {
      if (b->h_desc) cached_host_free(b->h_desc);
      b->h_desc = nullptr;
      b->h_desc_cap = ((pb + gb + rb) * 2 + 1024 + 4095) & ~(size_t)4095;  // (whole pages: batches of equal shape find each other's block)
      HIPCHK(cached_host_malloc(reinterpret_cast<void **>(&b->h_desc), b->h_desc_cap, hipHostMallocDefault, b->device));
    }
    std::memcpy(b->h_desc, descs.data(), pb);
    std::memcpy(b->h_desc + pb, groups.data(), gb);
    if (rb) std::memcpy(b->h_desc + pb + gb, b->h_priors.data(), rb);
    HIPCHK(hipMemcpyAsync(b->d_desc_block, b->h_desc, pb + gb + rb, hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipEventRecord(b->desc_done, b->stream));
  }
  // LDS staging of the DT footprint is available but off by default: on MI355X the unaligned 16-byte
  // row loads served by the XCD's L2 beat it at every size measured (profiles/LOG.md section 5)
  int use_lds = b->t_use_lds < 0 ? 0 : b->t_use_lds;
  int lds = b->t_lds_bytes >= 0 ? b->t_lds_bytes : (b->dtype == EA_F32 ? 32768 : 49152);
  if (lds > 61440) lds = 61440;
  b->lds_bytes = (use_lds && !any_variant) ? lds : 0;
  b->wide = (b->t_wide > 0 && b->dtype == EA_F32 && !any_variant && b->lds_bytes == 0) ? 1 : 0;
  {
    bool all32 = b->dtype == EA_F64 && !any_variant && b->lds_bytes == 0 && b->t_img32 != 0 && !terms.empty();
    for (const ea_problem *p : terms) all32 = all32 && p->dt32_exact && p->d_dt32;
    b->img32 = all32 ? 1 : 0;
  }
  b->xcd_remap = b->t_xcd < 0 ? 1 : (b->t_xcd ? 1 : 0);
  // only now is the batch consistent with its problems: a failure above leaves it dirty, so the next call rebuilds
  // instead of launching on freed or missing buffers
  for (size_t i = 0; i < b->probs.size(); ++i) {
    uint64_t v = b->probs[i]->version;
    for (ea_problem *tm : b->probs[i]->terms) v = v * 1000003u + tm->version + 17;
    b->versions[i] = v;
  }
  b->built = true;
  return EA_OK;
}

static void host_pose_state(const ea_problem *p, const double *q, const double *t, PoseState *ps) {
  double x[7] = {q[0], q[1], q[2], q[3], t[0], t[1], t[2]};
  make_pose_state(x, p->rot_transposed, 1, ps);
}

// what the batch's build fixed about its evaluation launches; kposes: in the shape of the pose-batched evaluation (kposes_shape)
static EvalLaunch eval_launch(const ea_batch *b, bool kposes = false) {
  EvalLaunch s;
  s.dtype = b->dtype; s.variant = b->any_variant; s.weighted = b->weighted_terms > 0 ? 1 : 0;
  s.ppt = kposes ? b->kp_ppt : b->ppt; s.nt = kposes ? b->kp_nt : b->nt;
  s.chunk = kposes ? b->kp_chunk : b->chunk; s.max_chunks = kposes ? b->kp_max_chunks : b->max_chunks;
  s.xcd_remap = b->xcd_remap; s.lds_bytes = b->lds_bytes; s.wide = b->wide; s.terms_are_groups = b->terms_are_groups;
  s.buffer_loads = b->buffer_loads; s.img32 = b->img32;
  s.x0 = b->x0; s.y0 = b->y0; s.z0 = b->z0; s.n0 = b->n0;
  return s;
}

static int batch_launch_eval(ea_batch *b, const PoseState *poses = nullptr) {
  HIPCHK(launch_eval_fused(eval_launch(b), b->d_probs, b->nterms, poses ? poses : b->d_poses, b->d_partials, b->stream));
  return EA_OK;
}

int ea::batch_upload_poses(ea_batch *b, const double *q, const double *t, const PoseState **d_poses) {
  const int count = (int)b->probs.size();
  for (int i = 0; i < count; ++i) host_pose_state(b->probs[i], q + 4 * i, t + 3 * i, &b->h_poses[i]);
  HIPCHK(hipMemcpyAsync(b->d_poses, b->h_poses, count * sizeof(PoseState), hipMemcpyHostToDevice, b->stream));
  b->poses_uploaded = true;
  b->poses_staged = false;
  if (d_poses) *d_poses = b->d_poses;
  return EA_OK;
}

// ---- what ea_frames.hip and ea_segments.hip see of a batch (ea_capi_internal.h; batch_frames_*: further up) ------------------

BatchView ea::batch_view(ea_batch *b) {
  BatchView v;
  v.device = b->device; v.dtype = b->dtype; v.stream = b->stream; v.probs = b->probs.data(); v.count = (int)b->probs.size();
  return v;
}

int ea::batch_built(ea_batch *b, BatchView *v) {
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  *v = batch_view(b);
  v->nterms = b->nterms; v->d_probs = b->d_probs; v->total_rows = b->total_rows;
  // (batch_build's staging block: the descriptors and groups of the current build)
  v->h_desc = reinterpret_cast<const ProblemDesc *>(b->h_desc);
  v->h_groups = reinterpret_cast<const GroupDesc *>(b->h_desc + (size_t)b->nterms * sizeof(ProblemDesc));
  return EA_OK;
}

int ea::batch_gate_reserve(ea_batch *b, size_t bytes, unsigned char **device_block, unsigned char **pinned_block) {
  if (b->gate_bytes < bytes) {
    cached_free(b->d_gate); cached_host_free(b->h_gate);
    b->d_gate = b->h_gate = nullptr; b->gate_bytes = 0;
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_gate), bytes, b->device));
    HIPCHK(cached_host_malloc(reinterpret_cast<void **>(&b->h_gate), bytes, hipHostMallocDefault, b->device));
    b->gate_bytes = bytes;
  }
  *device_block = b->d_gate;
  *pinned_block = b->h_gate;
  return EA_OK;
}

// the measurement hooks re-evaluate at "the poses of the last evaluation": bring them to the device if that evaluation read them
// from host memory
static int ensure_poses_on_device(ea_batch *b) {
  if (b->poses_uploaded) return EA_OK;
  if (!b->poses_staged) return fail(EA_ERR_STATE, "no poses uploaded yet (ea_batch_bench_eval or ea_batch_eval first)");
  HIPCHK(hipMemcpyAsync(b->d_poses, b->h_poses, b->probs.size() * sizeof(PoseState), hipMemcpyHostToDevice, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  b->poses_uploaded = true;
  b->poses_staged = false;
  return EA_OK;
}

// the 32 accumulator slots of every problem (pinned host copy) -> the caller's cost / 6x6 JtJ / Jtr / invalid count
static void unpack_eval_out(const EvalOut *src, int count, double *cost, double *JtJ, double *Jtr, int64_t *n_invalid) {
  for (int i = 0; i < count; ++i) {
    const double *acc = src[i].acc;
    if (cost) cost[i] = acc[kAccCost];
    if (JtJ) {
      int k = 0;
      for (int a = 0; a < 6; ++a)
        for (int c = a; c < 6; ++c) {
          JtJ[36 * i + 6 * a + c] = acc[kAccJtJ + k];
          JtJ[36 * i + 6 * c + a] = acc[kAccJtJ + k];
          ++k;
        }
    }
    if (Jtr) for (int a = 0; a < 6; ++a) Jtr[6 * i + a] = acc[kAccJtr + a];
    if (n_invalid) n_invalid[i] = (int64_t)llround(acc[kAccInvalid]);
  }
}
static void unpack_eval_out(const ea_batch *b, int count, double *cost, double *JtJ, double *Jtr, int64_t *n_invalid) {
  unpack_eval_out(b->h_out, count, cost, JtJ, Jtr, n_invalid);
}

// The last fold of a synchronous evaluation raises a flag in pinned host memory once every result has landed there
// (ea_reduce_done_kernel); the host polls it instead of waiting for the stream's completion signal, which arrives ~10 us
// later.  The poll is bounded: should the flag not show up (it always has), the stream is synchronised the classic way --
// the results are complete then, and a device fault surfaces as the error it is.
static hipError_t launch_last_fold(ea_batch *b, const GroupDesc *groups, int count, const double *rows, EvalOut *out) {
  const size_t c = b->probs.size();
  b->done_seq = b->done_seq == 0x7fffffff ? 1 : b->done_seq + 1;
  return launch_reduce_done(groups, count, rows, out, b->d_done_count, b->d_progress + 3 * c, b->done_seq, b->stream);
}

static int wait_results(ea_batch *b) {
  const size_t c = b->probs.size();
  if (!b->t_poll) {
    HIPCHK(hipStreamSynchronize(b->stream));
    return EA_OK;
  }
  SpinWait wait(2000.0);
  while (__atomic_load_n(&b->h_progress[3 * c], __ATOMIC_ACQUIRE) != b->done_seq) {
    if (wait.poll()) {
      HIPCHK(hipStreamSynchronize(b->stream));
      return EA_OK;
    }
  }
  return EA_OK;
}

// Whole-problem results land in pinned host memory: the priors' terms are added there, at the pose of each result (n results,
// result j belonging to problem j % count, its pose at qt(j) = 7 doubles q | t).  The fold kernels stay as they are.
template <typename PoseFn>
static void add_priors_host(const ea_batch *b, EvalOut *out, size_t n, PoseFn qt) {
  if (!b->any_side) return;
  const size_t count = b->probs.size();
  for (size_t j = 0; j < n; ++j) {
    const PriorDesc &pr = b->h_priors[j % count];
    if (!pr.has_q && !pr.has_t) continue;
    double x[7];
    qt(j, x);
    prior_add(pr, x, out[j].acc);
  }
}

extern "C" int ea_batch_eval(ea_batch *b, const double *q, const double *t, double *cost, double *JtJ,
                             double *Jtr, int64_t *n_invalid) {
  if (!b || !q || !t) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  const int count = (int)b->probs.size();
  if (count <= 4 && b->dv_h_poses && b->t_zero_copy != 0) {
    // A lone evaluation of a few problems: the pose constants stay where the host wrote them (pinned memory the device can
    // read) and every workgroup fetches its ~100 bytes from there -- one PCIe round trip inside the kernel's head instead of a
    // DMA transfer in front of the launch (26 -> 24 us per call, profiles/r03_ab_zero_copy.txt).  The call is synchronous: nobody touches h_poses before the
    // results are back.  (d_poses keeps whatever an earlier call uploaded.)
    for (int i = 0; i < count; ++i) host_pose_state(b->probs[i], q + 4 * i, t + 3 * i, &b->h_poses[i]);
    b->poses_uploaded = false;
    b->poses_staged = true;
    rc = batch_launch_eval(b, b->dv_h_poses);
  } else {
    rc = batch_upload_poses(b, q, t);
    if (rc != EA_OK) return rc;
    rc = batch_launch_eval(b);
  }
  if (rc != EA_OK) return rc;
  // the fold writes its 256 bytes per problem straight into pinned host memory: no device-to-host copy behind it (-6 us
  // of a 31 us call); the kernel's end makes them visible
  HIPCHK(launch_last_fold(b, b->d_groups, count, b->d_partials, b->dv_out));
  if ((rc = wait_results(b)) != EA_OK) return rc;
  add_priors_host(b, b->h_out, (size_t)count, [&](size_t j, double x[7]) {
    for (int k = 0; k < 4; ++k) x[k] = q[4 * j + k];
    for (int k = 0; k < 3; ++k) x[4 + k] = t[3 * j + k];
  });
  unpack_eval_out(b, count, cost, JtJ, Jtr, n_invalid);
  return EA_OK;
}

// ---- K evaluations at K different poses (ea_batch_set_poses / ea_batch_eval_resident_poses / ea_batch_eval_poses) ------
// What a caller that drives its own optimiser -- or probes a cost surface, or runs a line search -- asks of the evaluator:
// ceres::Problem::Evaluate once per pose (src/SolveEA.cpp:241 is the reference's one call of it).  One evaluation through
// ea_batch_eval is a launch pair and a synchronisation (~30 us on a 5e4-point pair, 3 us of which are the kernel, run by
// 196 workgroups on a 256-CU chip).  K independent evaluations do not have to queue up behind each other: the POSE is one
// more batch dimension.  A launch evaluates G poses of the batch: `rows` chunks per pose (all terms together, one partial row
// each) x G poses = one flat list of work items, dealt evenly over the 8 XCDs (ea_poses_map.h; a per-pose deal cannot be
// even when `rows` does not divide by 8 -- C2's 98 chunks left one XCD half idle), each XCD walking the poses of its own
// run of chunks back to back.  The kernel (ea_eval_poses_kernel) derives pose, term and chunk from the item: it reads the
// batch's own descriptors -- a copy behind a small row table, built once per build of the batch -- and pose slot
// pose * count + group, and writes partial row pose * rows + row.  Nothing is replicated per pose, so a larger K costs
// ea_batch_set_poses rows and result slots only.  K poses are n = ceil(K / G) launches of ceil(K / n) poses behind one
// synchronisation.  The fold of launch i -- one 256-lane workgroup per (pose, problem), straight into pinned host memory
// -- rides in FRONT of launch i + 1 (two row arrays alternate), only the last launch's is a launch of its own, in the
// same workgroups and summation order: a result does not depend on the launch its pose fell into.  Every fold raises a
// pinned flag to its own sequence number, and the host unpacks the results of launch i while launch i + 1 runs.  (The sums
// of pose k are those ea_batch_eval returns at pose k up to rounding: the pose path cuts the points into chunks of its
// own, kposes_shape.)  Every (point, pose) pair runs the whole per-point arithmetic; nothing is shared between poses but
// the bytes of the points and the image, which the later poses find in the caches.
// (From 1024 poses on an fp64 batch takes ea_eval_poses_lanes_kernel, which folds inside its launches: kposes_lanes below.)
// Variant functors, LDS staging, wide_accumulate and terms that share a pose keep the form this one replaced: descriptor
// and group tables replicated G times, a (chunks, G x terms) grid of ea_eval_fused_kernel's body under the name
// ea_eval_poses_grid_kernel, and a stand-alone 1024-lane fold behind every launch.
// (Round 3 first chained K launches with the fold of evaluation k-1 riding in launch k -- 3.3 us per C2 evaluation, one
// small launch at a time; G poses per launch fill the chip.)

// G: poses per launch -- enough workgroups to fill the chip several times over (~32k), within the grid's y limit and 64 MB
// of partial rows (both arrays of the flat form together)
// Launch shape.  One evaluation of a batch is shaped for latency (one point per lane on frame-sized problems: as many
// wavefronts as possible, few partial rows for the LM step to fold); a launch of G poses is throughput-bound, where more
// points per lane amortise the wavefront butterfly and 256-lane workgroups keep the occupancy
// (profiles/r03_ab_poses_shape.txt: C2 fp64 0.69 -> 0.58 us per evaluation at two points per lane, fp32 0.33 -> 0.27; C5
// fp32 5.65 -> 4.50 at 256 x 4 instead of 1024 x 4).  Explicit tuning ("points_per_thread", "threads") wins.
static bool kposes_flat(const ea_batch *b);
static void kposes_shape(ea_batch *b) {
  int nt = 256, ppt = b->dtype == EA_F64 ? 2 : (b->max_n >= 200000 ? 4 : 2);
  if (b->lds_bytes > 0 || b->wide) { nt = b->nt; ppt = b->ppt; }          // (those forms keep the shape they were tuned at)
  if (b->t_nt == 1024 || b->t_nt == 256) nt = b->t_nt;
  if (b->t_ppt == 1 || b->t_ppt == 2 || b->t_ppt == 4) ppt = b->t_ppt;
  if (b->any_variant) { nt = 256; ppt = std::min(ppt, 2); }  // (first, as in batch_build)
  if (nt == 1024 && b->dtype == EA_F64) ppt = 1;
  if (b->dtype == EA_F64 && ppt > 2) ppt = 2;
  b->kp_nt = nt; b->kp_ppt = ppt; b->kp_chunk = nt * ppt;
  // the wave-exchange reduction (ea_wave_exchange.h): the fp64, 256-lane launches of ea_eval_poses_kernel / ea_eval_starts_kernel
  b->kp_xchg = b->t_kp_xchg && b->dtype == EA_F64 && nt == 256 && kposes_flat(b);
  const ProblemDesc *hd = reinterpret_cast<const ProblemDesc *>(b->h_desc);
  int rows = 0, widest = 0;
  for (int j = 0; j < b->nterms; ++j) {
    const int nchunks = (int)(((int64_t)hd[j].n + b->kp_chunk - 1) / b->kp_chunk);
    rows += nchunks; widest = std::max(widest, nchunks);
  }
  b->kp_ntiles = rows; b->kp_max_chunks = widest;
}

static int64_t kposes_rows_bound(const ea_batch *b) {  // poses whose rows fit in 64 MB (both arrays of the flat form together)
  const int64_t wgs = std::max<int64_t>(1, (int64_t)b->kp_ntiles);
  return ((int64_t)64 << 20) / ((kposes_flat(b) ? 2 : 1) * wgs * kAccSlots * (int64_t)sizeof(double));
}
static int kposes_group(const ea_batch *b, int K) {
  const int64_t wgs = std::max<int64_t>(1, (int64_t)b->kp_ntiles);
  int64_t g = (32768 + wgs - 1) / wgs;
  g = std::min<int64_t>(g, 65535 / std::max(1, b->nterms));
  g = std::min<int64_t>(g, kposes_rows_bound(b));
  if (b->t_kp_G > 0) g = std::min<int64_t>(g, b->t_kp_G);
  return (int)std::max<int64_t>(1, std::min<int64_t>(g, K));
}

// One pose per lane (ea_eval_poses_lanes_kernel).  Whether a call of K poses takes it follows from the batch and K alone --
// never from G or the split into launches, so that any split lands on the same bits: a flat fp64 batch at the 256 x 2 pose
// shape whose rows leave room for one full group of 64 poses (kposes_rows_bound, the two-array bound of the flat form: the
// eligibility is what it was), and K at or above the threshold.
// Rows.  The path keeps ONE row array, lane-minor -- [group][row][slot][64 lanes], 16 KB per (group, row) -- because nothing
// alternates: the rows of a launch are folded inside that launch.  Its G is "as many whole groups as 64 MB hold of rows and
// run partials together, one group at least" (C2: (98 rows + 7 partials) x 16 KB = 1.6 MB per group, 39 groups = 2496
// poses; at the eligibility's limit of 2048 rows one group, as before), launches of G with the remainder last
// (poses_lanes_group_size / poses_lanes_launch_size); C2's K = 2000 is one launch.  "poses_per_launch" caps it; below 64 the
// launches have one partly filled group each -- slow, the same bits.
// Fold by tickets (ea_poses_map.h; lanes_tickets in ea_kernels.hip).  No workgroup waits for another.  An item stores its row
// and adds one to the counter of its (group, problem, run), a run being kPosesRun = 16 consecutive rows of the problem
// counted from its first; the workgroup that completes the run's count sums the run's rows in row order into a run partial
// and adds one to the counter of (group, problem); the workgroup that completes THAT count sums the run partials in run
// order, writes the group's 64 results of the problem into pinned memory and raises the pinned flag of (group of the call,
// problem) to the call's sequence number.  16 rows: one workgroup reads another's rows at 60 - 120 GB/s, so a run
// (256 KB) costs its last arrival 2 - 4 us and C2's 7 partials the problem's last arrival another 1 - 2 -- a whole group
// (1.5 MB) in one workgroup would leave 12 - 23 us behind the last item of the call.  The counters are zeroed by a memset
// node ahead of every launch.  A pose's sums are ((rows of run 0 in order) + (rows of run 1 in order) + ...): they depend
// on the pose and the problem's row count, not on the lane, the company in the group, the split into launches, the item
// order or the order of arrival.  A problem without a point has no item: the host writes its zero results and raises its
// flags itself (kposes_collect_lanes).
// Item order: pose-major by default (kPosesLanesOrder), the rows of a group adjacent in the list, so that groups complete
// one after the other and the host unpacks a group while the kernel works on the later ones; "poses_order" overrides.
constexpr int kPosesLanesOrder = 1;
static bool kposes_lanes(const ea_batch *b, int K) {
  if (!kposes_flat(b) || b->dtype != EA_F64 || b->kp_nt != 256 || b->kp_ppt != 2) return false;
  if (kposes_rows_bound(b) < kPosesLanes) return false;
  const int from = b->t_kp_lanes < 0 ? kPosesLanesFromK : b->t_kp_lanes;
  return from > 0 && K >= from;
}
static int kposes_group_lanes(const ea_batch *b, int K) {
  const int rows = std::max(1, b->kp_ntiles);
  const int64_t per_group = ((int64_t)rows + poses_lanes_run_slots(rows, (int)b->probs.size())) * kPosesLanesBlock * (int64_t)sizeof(double);
  int64_t g = std::min<int64_t>(std::max<int64_t>(1, ((int64_t)64 << 20) / per_group) * kPosesLanes, (int64_t)1 << 20);
  if (b->t_kp_G > 0) g = std::min<int64_t>(g, b->t_kp_G);
  return std::min(poses_lanes_group_size((int)g), K);
}
// the pose capacity kposes_tables is asked for so that its two arrays together hold the lanes path's one: whole groups of G
static int kposes_lanes_rows_cap(int G) { return (poses_lanes_groups(G) * kPosesLanes + 1) / 2; }
// poses per launch of the evaluation of the K resident poses (the last launch takes the remainder)
static int kposes_per(const ea_batch *b, int K) {
  return b->kp_lanes ? poses_lanes_launch_size(K, b->kp_G) : poses_launch_size(K, b->kp_G);
}

// a batch ea_eval_poses_kernel covers: the plain functor on the L2 path, one term per problem (any dtype, addressing and
// image type); the others keep the (chunks, G x terms) grid over replicated tables and a stand-alone fold per launch
static bool kposes_flat(const ea_batch *b) { return !b->any_variant && b->lds_bytes == 0 && !b->wide && b->terms_are_groups; }

static void kposes_free_tables(ea_batch *b) {
  if (b->d_kblock) cached_free(b->d_kblock);
  else { cached_free(b->d_kprobs); cached_free(b->d_kgroups); }
  cached_free(b->d_krows); cached_free(b->d_kcost); cached_free(b->d_kparts); cached_free(b->d_kcount);
  cached_host_free(b->h_kflags);
  b->d_kblock = nullptr; b->d_kprobs = nullptr; b->d_kgroups = nullptr; b->d_krows = nullptr; b->d_kcost = nullptr;
  b->d_kparts = nullptr; b->d_kcount = nullptr; b->h_kflags = nullptr; b->dv_kflags = nullptr;
  b->kp_G = 0; b->kp_rows_cap = 0; b->kcost_bytes = 0; b->kl_groups_cap = 0; b->kl_flags_cap = 0;
}

// What the pose-batched launches read beside the batch's own tables, and the partial rows of G poses; the tables are rebuilt
// when the batch was (kp_G = 0), the rows grow with G.
//   flat form: ONE block [PosesRow x rows | ProblemDesc x nterms | GroupDesc x count] -- the row table (ea_poses_map.h), a
//     copy of the descriptors right behind it (the kernel finds the table at probs - rows) and the group table in the pose
//     path's own chunking -- built once per build of the batch, whatever G; two row arrays of G poses each, which the
//     launches of a call alternate between (the riders of launch i + 1 read what launch i wrote).  The lanes path uses the
//     same allocation as ONE lane-minor array of whole groups (kposes_lanes_rows_cap) and has run partials, counters and
//     flags of its own (kposes_lanes_reserve).
//   grid form: the descriptor / group tables replicated G times and one row array of G poses.
static int kposes_tables(ea_batch *b, int G) {
  const bool fresh = b->kp_G == 0, flat = kposes_flat(b);
  if (!fresh && G <= b->kp_rows_cap) { b->kp_G = G; return EA_OK; }
  HIPCHK(hipStreamSynchronize(b->stream));
  const size_t nterms = (size_t)b->nterms, count = b->probs.size(), rows = (size_t)b->kp_ntiles;
  if (fresh || !flat) kposes_free_tables(b);
  else { cached_free(b->d_krows); b->d_krows = nullptr; b->kp_rows_cap = 0; }
  const ProblemDesc *hd = reinterpret_cast<const ProblemDesc *>(b->h_desc);                          // (batch_build's staging block)
  const GroupDesc *hg = reinterpret_cast<const GroupDesc *>(b->h_desc + nterms * sizeof(ProblemDesc));
  // the partial rows of one pose in the pose path's own chunking (kposes_shape)
  std::vector<int32_t> row0(nterms + 1, 0);
  for (size_t j = 0; j < nterms; ++j) row0[j + 1] = row0[j] + (int32_t)(((int64_t)hd[j].n + b->kp_chunk - 1) / b->kp_chunk);
  const size_t row_bytes = std::max<size_t>(1, (flat ? 2 : 1) * (size_t)G * rows) * kAccSlots * sizeof(double);
  if (flat && !b->d_kblock) {
    const size_t tb = rows * sizeof(PosesRow), pb = nterms * sizeof(ProblemDesc), gb = count * sizeof(GroupDesc);
    static_assert(sizeof(PosesRow) == 16 && alignof(ProblemDesc) <= 16, "the descriptors sit right behind the row table");
    std::vector<unsigned char> blk(tb + pb + gb);
    PosesRow *tab = reinterpret_cast<PosesRow *>(blk.data());
    ProblemDesc *descs = reinterpret_cast<ProblemDesc *>(blk.data() + tb);
    GroupDesc *groups = reinterpret_cast<GroupDesc *>(blk.data() + tb + pb);
    for (size_t j = 0; j < nterms; ++j) {
      for (int32_t r = row0[j]; r < row0[j + 1]; ++r) tab[r] = PosesRow{(int32_t)j, row0[j], (int32_t)count, 0};
      descs[j] = hd[j];
      descs[j].tile_begin = row0[j]; descs[j].tile_end = row0[j + 1];
    }
    for (size_t i = 0; i < count; ++i) {
      groups[i] = hg[i];
      groups[i].tile_begin = row0[(size_t)hg[i].term_begin]; groups[i].tile_end = row0[(size_t)hg[i].term_end];
    }
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_kblock), std::max<size_t>(16, blk.size()), b->device));
    b->d_kprobs = reinterpret_cast<ProblemDesc *>(b->d_kblock + tb);
    b->d_kgroups = reinterpret_cast<GroupDesc *>(b->d_kblock + tb + pb);
    if (!blk.empty()) HIPCHK(hipMemcpyAsync(b->d_kblock, blk.data(), blk.size(), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));  // (the host vector goes out of scope)
  } else if (!flat) {
    std::vector<ProblemDesc> descs((size_t)G * nterms);
    std::vector<GroupDesc> groups((size_t)G * count);
    for (int g = 0; g < G; ++g) {
      for (size_t j = 0; j < nterms; ++j) {
        ProblemDesc d = hd[j];
        d.tile_begin = row0[j] + (int32_t)(g * rows); d.tile_end = row0[j + 1] + (int32_t)(g * rows);
        d.group += (int32_t)(g * count);
        descs[(size_t)g * nterms + j] = d;
      }
      for (size_t i = 0; i < count; ++i) {
        GroupDesc gd = hg[i];
        gd.tile_begin = row0[(size_t)hg[i].term_begin] + (int32_t)(g * rows); gd.tile_end = row0[(size_t)hg[i].term_end] + (int32_t)(g * rows);
        gd.term_begin += (int32_t)(g * nterms); gd.term_end += (int32_t)(g * nterms);
        groups[(size_t)g * count + i] = gd;
      }
    }
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_kprobs), std::max<size_t>(1, descs.size()) * sizeof(ProblemDesc), b->device));
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_kgroups), groups.size() * sizeof(GroupDesc), b->device));
    if (!descs.empty()) HIPCHK(hipMemcpyAsync(b->d_kprobs, descs.data(), descs.size() * sizeof(ProblemDesc), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipMemcpyAsync(b->d_kgroups, groups.data(), groups.size() * sizeof(GroupDesc), hipMemcpyHostToDevice, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));  // (the host vectors go out of scope)
  }
  HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_krows), row_bytes, b->device));
  HIPCHK(hipMemsetAsync(b->d_krows, 0, row_bytes, b->stream));
  b->kp_rows_cap = G;
  b->kp_G = G;
  return EA_OK;
}

// run partials and counters for launches of G poses, flags for a call of K (the lanes path)
static int kposes_lanes_reserve(ea_batch *b, int G, int K) {
  const int count = (int)b->probs.size(), rows = b->kp_ntiles, groups = poses_lanes_groups(G);
  if (groups > b->kl_groups_cap) {
    HIPCHK(hipStreamSynchronize(b->stream));
    cached_free(b->d_kparts); cached_free(b->d_kcount);
    b->d_kparts = nullptr; b->d_kcount = nullptr; b->kl_groups_cap = 0;
    const size_t pb = std::max<size_t>(1, (size_t)groups * (size_t)poses_lanes_run_slots(rows, count)) * kPosesLanesBlock * sizeof(double);
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_kparts), pb, b->device));
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_kcount), std::max<size_t>(4, poses_lanes_counters(groups, rows, count)) * sizeof(unsigned int), b->device));
    b->kl_groups_cap = groups;
  }
  const size_t nflags = (size_t)poses_lanes_call_groups(K, G) * (size_t)count;
  if (nflags > b->kl_flags_cap) {
    HIPCHK(hipStreamSynchronize(b->stream));
    cached_host_free(b->h_kflags);
    b->h_kflags = nullptr; b->dv_kflags = nullptr; b->kl_flags_cap = 0;
    HIPCHK(cached_host_malloc(reinterpret_cast<void **>(&b->h_kflags), nflags * sizeof(int), hipHostMallocMapped, b->device));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->dv_kflags), b->h_kflags, 0));
    std::memset(b->h_kflags, 0, nflags * sizeof(int));  // (no sequence number is 0)
    b->kl_flags_cap = nflags;
  }
  return EA_OK;
}

static int kposes_reserve(ea_batch *b, int K) {
  const size_t count = b->probs.size();
  if (K <= b->kp_cap) return EA_OK;
  HIPCHK(hipStreamSynchronize(b->stream));  // (launches still reading the old arrays)
  kposes_free(b);
  const int cap = std::max(K, 8);
  const size_t n = (size_t)cap * count;
  HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_kqt), n * 7 * sizeof(double), b->device));
  HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_kposes), n * sizeof(PoseState), b->device));
  HIPCHK(cached_host_malloc(reinterpret_cast<void **>(&b->h_kqt), n * 7 * sizeof(double), hipHostMallocDefault, b->device));
  HIPCHK(cached_host_malloc(reinterpret_cast<void **>(&b->h_kout), n * sizeof(EvalOut), hipHostMallocMapped, b->device));
  HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->dv_kout), b->h_kout, 0));
  std::memset(b->h_kout, 0, n * sizeof(EvalOut));  // (a cost-only call fills two slots of a result; the priors add to all)
  b->kp_cap = cap;
  return EA_OK;
}

extern "C" int ea_batch_set_poses(ea_batch *b, int K, const double *q, const double *t) {
  if (!b || !q || !t) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (K < 1 || K > (1 << 20)) return fail(EA_ERR_INVALID_ARG, "K out of range");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  b->kp_K = 0;
  if ((rc = kposes_reserve(b, K)) != EA_OK) return rc;
  if (b->kp_G == 0) kposes_shape(b);   // (once per build of the batch)
  // (the cost-only kernel keeps its own launch size: the rows hold the larger of the two)
  const int lanes = kposes_lanes(b, K), Gc = kposes_group(b, K), G = lanes ? kposes_group_lanes(b, K) : Gc;
  if ((rc = kposes_tables(b, lanes ? std::max(kposes_lanes_rows_cap(G), Gc) : std::max(G, Gc))) != EA_OK) return rc;
  if (lanes && (rc = kposes_lanes_reserve(b, G, K)) != EA_OK) return rc;
  b->kp_G = G; b->kp_Gc = Gc; b->kp_lanes = lanes;
  const size_t n = (size_t)K * b->probs.size();
  // (the previous upload out of the same staging block has been consumed: every call below ends with its pose kernel
  // enqueued behind the copy, and the evaluations that follow are synchronised before they return)
  HIPCHK(hipStreamSynchronize(b->stream));
  for (size_t i = 0; i < n; ++i) {
    double *d = b->h_kqt + 7 * i;
    d[0] = q[4 * i]; d[1] = q[4 * i + 1]; d[2] = q[4 * i + 2]; d[3] = q[4 * i + 3];
    d[4] = t[3 * i]; d[5] = t[3 * i + 1]; d[6] = t[3 * i + 2];
  }
  HIPCHK(hipMemcpyAsync(b->d_kqt, b->h_kqt, n * 7 * sizeof(double), hipMemcpyHostToDevice, b->stream));
  HIPCHK(launch_make_poses(b->d_kqt, (int)n, (int)b->probs.size(), b->d_probs, b->d_groups, b->d_kposes, b->stream));
  b->kp_K = K;
  return EA_OK;
}

static int next_done_seq(ea_batch *b) { return b->done_seq = b->done_seq == 0x7fffffff ? 1 : b->done_seq + 1; }
// the pinned flag only ever moves forward through the sequence numbers of a call: "has reached", not "equals" -- the host may
// look after a later launch of the same call has raised it again
static bool seq_reached(int flag, int seq) { return (unsigned)flag - (unsigned)seq < 0x40000000u; }

// The K evaluations of the resident poses on the batch's stream, results into dv_kout[k * count + i]: launches of
// ceil(K / n) poses, n = ceil(K / G) (the last one takes the remainder).  Flat form: the fold of launch i rides in front of
// launch i + 1, the last launch's is a stand-alone launch of the same workgroups; every fold raises the pinned flag to a
// sequence number of its own (consecutive within the call; b->kp_marks keeps them for the caller that unpacks as it goes).
// Grid form: an evaluation + fold pair per launch, the last fold raises the flag (flag_last).
static int enqueue_resident_poses(ea_batch *b, int K, bool folds = true, bool flag_last = false) {
  const int count = (int)b->probs.size(), per = kposes_per(b, K), rows = b->kp_ntiles;
  b->kp_marks.clear();
  b->last_kp_xchg = 0; b->last_kp_lanes = 0;
  if (!kposes_flat(b)) {
    for (int start = 0; start < K; start += per) {
      const int g = std::min(per, K - start);
      HIPCHK(launch_eval_poses_grid(eval_launch(b, /*kposes=*/true), b->d_kprobs, g * b->nterms, b->d_kposes + (size_t)start * count,
                                    b->d_krows, b->stream));
      if (!folds) continue;
      if (flag_last && start + g >= K) HIPCHK(launch_last_fold(b, b->d_kgroups, g * count, b->d_krows, b->dv_kout + (size_t)start * count));
      else HIPCHK(launch_reduce(b->d_kgroups, g * count, b->d_krows, b->dv_kout + (size_t)start * count, b->stream));
    }
    return EA_OK;
  }
  if (b->done_seq > 0x7fffffff - (K + per - 1) / per - 2) b->done_seq = 0;  // (a call's sequence numbers do not straddle the wrap)
  const EvalLaunch shape = eval_launch(b, /*kposes=*/true);
  PosesLaunch pl;
  const bool lanes = b->kp_lanes != 0;
  pl.rows = rows; pl.order = b->t_kp_order < 0 ? (lanes ? kPosesLanesOrder : 0) : b->t_kp_order; pl.single = b->nterms == 1; pl.exchange = b->kp_xchg;
  b->last_kp_xchg = rows > 0 && !lanes ? b->kp_xchg : 0;
  b->last_kp_lanes = rows > 0 && lanes;
  PosesFold owed;  // the fold the launches so far still owe (n = 0: none)
  owed.count = count; owed.rows_per_pose = rows; owed.groups = b->d_kgroups;
  owed.counter = b->d_done_count; owed.host_flag = b->d_progress + 3 * (size_t)count;
  auto owe = [&](int start, int g, const double *from) {
    owed.n = g * count; owed.rows = from; owed.out = b->dv_kout + (size_t)start * count; owed.seq = next_done_seq(b);
    b->kp_marks.push_back({owed.seq, start, g});
  };
  if (rows == 0) {  // not a single point in the batch: nothing to evaluate, K x count zero results owed
    if (folds) { owe(0, K, b->d_krows); HIPCHK(launch_poses_fold(b->kp_nt, owed, b->stream)); }
    return EA_OK;
  }
  if (lanes) {  // one row array, the fold inside each launch; one sequence number for the call, a mark per group of the call
    PosesTickets tk;
    tk.on = folds; tk.count = count; tk.seq = folds ? next_done_seq(b) : 0;
    tk.partials = b->d_kparts; tk.counters = b->d_kcount; tk.flags = b->dv_kflags;
    for (int start = 0; start < K; start += per) {
      pl.g = std::min(per, K - start);
      tk.out = b->dv_kout + (size_t)start * count;
      HIPCHK(launch_eval_poses_lanes(shape, pl, b->d_kprobs, b->d_kposes + (size_t)start * count, b->d_krows, tk, b->stream));
      if (folds)
        for (int p0 = 0; p0 < pl.g; p0 += kPosesLanes) b->kp_marks.push_back({tk.seq, start + p0, std::min(kPosesLanes, pl.g - p0)});
      tk.group0 += poses_lanes_groups(pl.g);
    }
    return EA_OK;
  }
  int i = 0;
  for (int start = 0; start < K; start += per, ++i) {
    double *into = b->d_krows + (size_t)(i & 1) * (size_t)b->kp_rows_cap * (size_t)rows * kAccSlots;
    pl.g = std::min(per, K - start);
    HIPCHK(launch_eval_poses(shape, pl, b->d_kprobs, b->d_kposes + (size_t)start * count, into, owed, b->stream));
    if (folds) owe(start, pl.g, into);
  }
  if (folds) HIPCHK(launch_poses_fold(b->kp_nt, owed, b->stream));
  return EA_OK;
}

// results [first, first + n) of the last call (n a multiple of the problem count): priors added at each result's own pose,
// then out into the caller's arrays
static void kposes_unpack(ea_batch *b, size_t first, size_t n, double *cost, double *JtJ, double *Jtr, int64_t *n_invalid) {
  add_priors_host(b, b->h_kout + first, n, [&](size_t j, double x[7]) {  // (h_kqt: the staging block of ea_batch_set_poses)
    for (int k = 0; k < 7; ++k) x[k] = b->h_kqt[7 * (first + j) + k];
  });
  if (cost || JtJ || Jtr || n_invalid)
    unpack_eval_out(b->h_kout + first, (int)n, cost ? cost + first : nullptr, JtJ ? JtJ + 36 * first : nullptr,
                    Jtr ? Jtr + 6 * first : nullptr, n_invalid ? n_invalid + first : nullptr);
}

// The results of the launches enqueue_resident_poses / enqueue_resident_cost put on the stream, out of pinned memory.  The
// results of launch i are unpacked as soon as its fold has raised the flag -- launch i + 1 is still running then -- so that
// only the last launch's remain behind the final wait.  The poll is bounded like wait_results: should a flag not show up,
// the stream is synchronised (everything is complete then, and a device error surfaces as the error it is).
// The lanes path: mark m is group m of the call, complete when the flags of its `count` problems have reached the call's
// sequence number.  The groups are looked at round after round and each is unpacked as soon as it is complete, whatever the
// order they finish in, while the kernel works on the others; what remains behind the last wait is the last group.  That
// last wait is the stream's completion signal where "poll_results" is 0, as in the other path.  A problem without a point
// has no work item: its zero results and its flags are written here.
static int kposes_collect_lanes(ea_batch *b, double *cost, double *JtJ, double *Jtr, int64_t *n_invalid) {
  const size_t count = b->probs.size();
  const ProblemDesc *hd = reinterpret_cast<const ProblemDesc *>(b->h_desc);
  for (size_t i = 0; i < count; ++i) {
    if (hd[i].n > 0) continue;
    for (size_t m = 0; m < b->kp_marks.size(); ++m) {
      const KposesMark &mk = b->kp_marks[m];
      for (int p = 0; p < mk.g; ++p) std::memset(b->h_kout + (size_t)(mk.start + p) * count + i, 0, sizeof(EvalOut));
      __atomic_store_n(&b->h_kflags[poses_lanes_flag((int)m, (int)i, (int)count)], mk.seq, __ATOMIC_RELEASE);
    }
  }
  std::vector<int> pending(b->kp_marks.size());
  for (size_t m = 0; m < pending.size(); ++m) pending[m] = (int)m;
  bool drained = false;
  SpinWait wait(2000.0);
  while (!pending.empty()) {
    if (!drained && pending.size() == 1 && !b->t_poll) {
      HIPCHK(hipStreamSynchronize(b->stream));
      drained = true;
    }
    size_t kept = 0;
    for (size_t j = 0; j < pending.size(); ++j) {
      const int m = pending[j];
      const KposesMark &mk = b->kp_marks[(size_t)m];
      bool ready = true;
      for (size_t i = 0; i < count && ready && !drained; ++i)
        ready = seq_reached(__atomic_load_n(&b->h_kflags[poses_lanes_flag(m, (int)i, (int)count)], __ATOMIC_ACQUIRE), mk.seq);
      if (ready) kposes_unpack(b, (size_t)mk.start * count, (size_t)mk.g * count, cost, JtJ, Jtr, n_invalid);
      else pending[kept++] = m;
    }
    if (kept < pending.size()) wait.progress();
    else if (wait.poll()) {
      HIPCHK(hipStreamSynchronize(b->stream));
      drained = true;
    }
    pending.resize(kept);
  }
  return EA_OK;
}

static int kposes_collect(ea_batch *b, int K, double *cost, double *JtJ, double *Jtr, int64_t *n_invalid) {
  int rc;
  if (b->last_kp_lanes) return kposes_collect_lanes(b, cost, JtJ, Jtr, n_invalid);
  const size_t count = b->probs.size();
  size_t done = 0;
  bool drained = false;
  for (size_t m = 0; m + 1 < b->kp_marks.size() && !drained; ++m) {
    const KposesMark &mk = b->kp_marks[m];
    SpinWait wait(2000.0);
    while (!seq_reached(__atomic_load_n(&b->h_progress[3 * count], __ATOMIC_ACQUIRE), mk.seq)) {
      if (wait.poll()) {
        HIPCHK(hipStreamSynchronize(b->stream));
        drained = true;
        break;
      }
    }
    if (drained) break;
    kposes_unpack(b, done, (size_t)mk.g * count, cost, JtJ, Jtr, n_invalid);
    done += (size_t)mk.g * count;
  }
  if (!drained && (rc = wait_results(b)) != EA_OK) return rc;
  kposes_unpack(b, done, (size_t)K * count - done, cost, JtJ, Jtr, n_invalid);
  return EA_OK;
}

extern "C" int ea_batch_eval_resident_poses(ea_batch *b, double *cost, double *JtJ, double *Jtr, int64_t *n_invalid) {
  if (!b) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  const int K = b->kp_K;
  if (K < 1 || b->kp_G < 1) return fail(EA_ERR_STATE, "no poses resident (ea_batch_set_poses first; a change of the batch's problems drops them)");
  if ((rc = enqueue_resident_poses(b, K, true, true)) != EA_OK) return rc;
  return kposes_collect(b, K, cost, JtJ, Jtr, n_invalid);
}

// ---- cost-only evaluation of the resident poses (ea_batch_cost_resident_poses / ea_batch_cost_poses) --------------------
// Everything around the kernel is the evaluation path's: the resident poses, G and the even split of K over launches, the
// pose path's tables and launch shape, one synchronisation, results unpacked launch by launch, priors added on the host at
// each result's own pose (the cost slot of prior_add).  The kernel pair is ea_cost_poses_kernel -- the same work items, one
// 16-byte partial {cost, failed functors} per workgroup -- and ea_cost_fold_kernel as a launch of its own behind every
// evaluation launch (one array of narrow partials; nothing rides), which writes the two values into the cost and invalid
// slots of the result in pinned memory and raises the flag to the launch's sequence number.  A result is a fixed-order sum
// over (chunk, lane, wave) and the rows of its pose: it does not depend on G, the split or the item order.
static int enqueue_resident_cost(ea_batch *b, int K) {
  const int count = (int)b->probs.size(), per = poses_launch_size(K, b->kp_Gc), rows = b->kp_ntiles;
  b->kp_marks.clear();
  b->last_kp_xchg = 0; b->last_kp_lanes = 0;
  if (b->done_seq > 0x7fffffff - (K + per - 1) / per - 2) b->done_seq = 0;  // (a call's sequence numbers do not straddle the wrap)
  const size_t need = std::max<size_t>(1, (size_t)per * (size_t)rows) * kCostPartialBytes;
  if (need > b->kcost_bytes) {
    HIPCHK(hipStreamSynchronize(b->stream));
    cached_free(b->d_kcost);
    b->d_kcost = nullptr; b->kcost_bytes = 0;
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_kcost), need, b->device));
    b->kcost_bytes = need;
  }
  PosesFold f;
  f.count = count; f.rows_per_pose = rows; f.groups = b->d_kgroups; f.rows = reinterpret_cast<const double *>(b->d_kcost);
  f.counter = b->d_done_count; f.host_flag = b->d_progress + 3 * (size_t)count;
  auto fold = [&](int start, int g) -> hipError_t {
    f.n = g * count; f.out = b->dv_kout + (size_t)start * count; f.seq = next_done_seq(b);
    b->kp_marks.push_back({f.seq, start, g});
    return launch_cost_fold(f, b->stream);
  };
  if (rows == 0) {  // not a single point in the batch: K x count zero results
    HIPCHK(fold(0, K));
    return EA_OK;
  }
  const EvalLaunch shape = eval_launch(b, /*kposes=*/true);
  PosesLaunch pl;
  pl.rows = rows; pl.order = std::max(0, b->t_kp_order); pl.single = b->nterms == 1;
  for (int start = 0; start < K; start += per) {
    pl.g = std::min(per, K - start);
    HIPCHK(launch_cost_poses(shape, pl, b->d_kprobs, b->d_kposes + (size_t)start * count, b->d_kcost, b->stream));
    HIPCHK(fold(start, pl.g));
  }
  return EA_OK;
}

// the batches the cost kernel serves: what ea_eval_poses_kernel covers, in 256-lane workgroups
static bool kposes_cost_form(const ea_batch *b) { return b->t_cost_form != 0 && kposes_flat(b) && b->kp_nt == 256; }

extern "C" int ea_batch_cost_resident_poses(ea_batch *b, double *cost, int64_t *n_invalid) {
  if (!b) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  const int K = b->kp_K;
  if (K < 1 || b->kp_G < 1) return fail(EA_ERR_STATE, "no poses resident (ea_batch_set_poses first; a change of the batch's problems drops them)");
  if (!kposes_cost_form(b)) {  // the full evaluation, only the cost and the count fetched
    b->last_cost_form = 0;
    return ea_batch_eval_resident_poses(b, cost, nullptr, nullptr, n_invalid);
  }
  b->last_cost_form = 1;
  if ((rc = enqueue_resident_cost(b, K)) != EA_OK) return rc;
  return kposes_collect(b, K, cost, nullptr, nullptr, n_invalid);
}

extern "C" int ea_batch_cost_poses(ea_batch *b, int K, const double *q, const double *t, double *cost, int64_t *n_invalid) {
  int rc = ea_batch_set_poses(b, K, q, t);
  if (rc != EA_OK) return rc;
  return ea_batch_cost_resident_poses(b, cost, n_invalid);
}

// (ea_hip_dev.h) `reps` runs of the resident poses' launches between one event pair on the batch's stream: milliseconds
// per run, the device's own view of the K evaluations; evaluations_only: without the fold launches -- on the lanes path
// without tickets and folds inside the launch -- (what bench.py divides by the number of evaluation launches for the
// dominant kernel's duration); launches (nullable) = evaluation launches per run
extern "C" int ea_batch_bench_resident_poses(ea_batch *b, int reps, int evaluations_only, double *ms_per_run, int *launches) {
  if (!b || !ms_per_run || reps < 1) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = ea_batch_eval_resident_poses(b, nullptr, nullptr, nullptr, nullptr);
  if (rc != EA_OK) return rc;
  EventPair evp;
  HIPCHK(hipEventCreate(&evp.e0));
  HIPCHK(hipEventCreate(&evp.e1));
  // (the stream is held while the runs are enqueued: the launches execute back to back from the queue)
  HIPCHK(hipLaunchHostFunc(b->stream, [](void *) { std::this_thread::sleep_for(std::chrono::milliseconds(2)); }, nullptr));
  HIPCHK(hipEventRecord(evp.e0, b->stream));
  for (int i = 0; i < reps; ++i) if ((rc = enqueue_resident_poses(b, b->kp_K, !evaluations_only)) != EA_OK) return rc;
  HIPCHK(hipEventRecord(evp.e1, b->stream));
  HIPCHK(hipEventSynchronize(evp.e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, evp.e0, evp.e1));
  *ms_per_run = (double)ms / reps;
  if (launches) { const int per = kposes_per(b, b->kp_K); *launches = (b->kp_K + per - 1) / per; }
  return EA_OK;
}

// (ea_hip_dev.h) The floor of the launch mechanism the sequences above run on: a hipGraph of `nodes` kernel nodes, each an
// EMPTY kernel of grid x block threads, replayed between one event pair -- milliseconds per node.  What a launch of any
// size costs when it does nothing; a kernel's duration cannot go below it, so (algorithmic bytes / floor) bounds the
// roofline fraction a small launch can reach.
extern "C" int ea_bench_graph_floor(int device, int nodes, int grid, int block, double *ms_per_node) {
  if (!ms_per_node || nodes < 1 || grid < 1 || block < 1 || block > 1024) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = check_device(device);
  if (rc != EA_OK) return rc;
  HIPCHK(hipSetDevice(device));
  hipStream_t st = nullptr;
  HIPCHK(cached_stream_create(&st, device));
  hipGraph_t graph = nullptr;
  hipGraphExec_t exec = nullptr;
  EventPair evp;
  hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
  for (int i = 0; i < nodes && e == hipSuccess; ++i) e = launch_empty(grid, block, st);
  const hipError_t ee = hipStreamEndCapture(st, &graph);
  if (e == hipSuccess) e = ee;
  if (e == hipSuccess) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
  if (graph) (void)hipGraphDestroy(graph);
  double best = 1e30;
  if (e == hipSuccess) e = hipEventCreate(&evp.e0);
  if (e == hipSuccess) e = hipEventCreate(&evp.e1);
  for (int r = 0; r < 5 && e == hipSuccess; ++r) {  // (first replay uploads the graph; best of the rest)
    e = hipEventRecord(evp.e0, st);
    if (e == hipSuccess) e = hipGraphLaunch(exec, st);
    if (e == hipSuccess) e = hipEventRecord(evp.e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(evp.e1);
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, evp.e0, evp.e1);
    if (r > 0 && e == hipSuccess) best = std::min(best, (double)ms / nodes);
  }
  if (exec) (void)hipGraphExecDestroy(exec);
  (void)hipStreamSynchronize(st);
  cached_stream_destroy(st, device);
  if (e != hipSuccess) return fail(EA_ERR_HIP, std::string("graph floor: ") + hipGetErrorString(e));
  *ms_per_node = best;
  return EA_OK;
}

extern "C" int ea_batch_eval_poses(ea_batch *b, int K, const double *q, const double *t, double *cost, double *JtJ, double *Jtr,
                                   int64_t *n_invalid) {
  int rc = ea_batch_set_poses(b, K, q, t);
  if (rc != EA_OK) return rc;
  return ea_batch_eval_resident_poses(b, cost, JtJ, Jtr, n_invalid);
}

static void fill_summary(const LMState &s, const LMTrace &tr, int64_t npts, double ms, ea_summary *out) {
  std::memset(out, 0, sizeof(*out));
  out->termination = s.termination;
  out->why = s.why;
  out->num_iterations = s.iteration;
  out->num_successful_steps = s.num_successful;
  out->num_unsuccessful_steps = s.num_unsuccessful;
  const bool no_start = s.why == EA_WHY_INITIAL_EVAL_FAILED;  // no trace row exists: costs as Ceres leaves them (-1)
  out->initial_cost = no_start ? -1.0 : tr.it_cost[0];
  out->final_cost = no_start ? -1.0 : s.cost;
  out->num_point_evals = (int64_t)s.num_evals * npts;
  out->total_time_ms = ms;
  const int ni = no_start ? 0 : std::min(s.iteration + 1, (int)EA_MAX_TRACE);
  for (int i = 0; i < ni; ++i) {
    out->it_cost[i] = tr.it_cost[i];
    out->it_cost_change[i] = tr.it_cost_change[i];
    out->it_gradient_max_norm[i] = tr.it_gradient_max_norm[i];
    out->it_step_norm[i] = tr.it_step_norm[i];
    out->it_relative_decrease[i] = tr.it_relative_decrease[i];
    out->it_radius[i] = tr.it_radius[i];
    out->it_successful[i] = tr.it_successful[i];
  }
}

// ---- solve: the trust-region loop of every problem of a batch, on the device ---------------------------------------
//
// One run = one batch on its own stream.  The loop runs on the device: each (evaluate, LM step) pair reads the pose
// the previous step published.  The step kernel reports progress into pinned host memory; the host only keeps a few
// pairs queued ahead of it and stops enqueueing when every problem has terminated (pairs that are already queued
// find `active == 0` and return at once).
struct SolveRun {
  ea_batch *b = nullptr;
  int first = 0;  // index of the run's first problem in the caller's arrays
  int count = 0, enq = 0, budget = 0, ahead = 2;
  int seen = 0;   // evaluations the device had completed at the last look (progress = this moved, or a pair went out)
  unsigned spins = 0;
  bool done = false, fetch = false, moved = false;
  bool fused = false;  // one launch per iteration (ea_lm_iter_kernel) instead of (evaluate, step) pairs
};

static double resolve_timeout_ms(const ea_options &o) { return o.solve_timeout_ms == 0.0 ? 5000.0 : o.solve_timeout_ms; }

// the caller's options (NULL: the defaults), validated
static int resolve_options(const ea_options *opt_in, ea_options *o) {
  if (opt_in) *o = *opt_in; else ea_default_options(o);
  return check_options(*o);
}

// Value-initialised: a field LMOptions gains and this mapping forgets is zero in every driver, not stack garbage in one.
static LMOptions lm_options(const ea_options &o) {
  LMOptions lo{};
  lo.max_num_iterations = o.max_num_iterations;
  lo.function_tolerance = o.function_tolerance;
  lo.gradient_tolerance = o.gradient_tolerance;
  lo.parameter_tolerance = o.parameter_tolerance;
  lo.initial_trust_region_radius = o.initial_trust_region_radius;
  lo.max_trust_region_radius = o.max_trust_region_radius;
  lo.min_trust_region_radius = o.min_trust_region_radius;
  lo.min_relative_decrease = o.min_relative_decrease;
  lo.min_lm_diagonal = o.min_lm_diagonal;
  lo.max_lm_diagonal = o.max_lm_diagonal;
  lo.max_num_consecutive_invalid_steps = o.max_num_consecutive_invalid_steps;
  lo.jacobi_scaling = o.jacobi_scaling;
  lo.strategy = o.strategy;
  return lo;
}

static int solve_start(SolveRun &r, const ea_options &o, const LMOptions &lo, const double *q, const double *t) {
  ea_batch *b = r.b;
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  const int count = r.count = (int)b->probs.size();
  for (int i = 0; i < count; ++i) {
    lm_init(&b->h_states[i], &lo, q + 4 * i, t + 3 * i, b->probs[i]->rot_transposed, b->probs[i]->held);
    host_pose_state(b->probs[i], q + 4 * i, t + 3 * i, &b->h_poses[i]);
    b->h_progress[i] = 1;          // running
    b->h_progress[count + i] = 0;  // evaluations whose step kernel has started
    b->h_progress[2 * count + i] = 0;  // step kernels complete (posted on request: the point-sharded solve)
  }
  if (b->t_test_stall_ms > 0)  // (tests/test_gpu_robustness.py: a device that shows no progress must trip the deadline)
    HIPCHK(hipLaunchHostFunc(b->stream, [](void *ms) { std::this_thread::sleep_for(std::chrono::milliseconds((intptr_t)ms)); },
                             (void *)(intptr_t)b->t_test_stall_ms));
  HIPCHK(hipMemcpyAsync(b->d_lm_block, b->h_lm_block, (size_t)count * (sizeof(PoseState) + sizeof(LMState)),
                        hipMemcpyHostToDevice, b->stream));
  b->poses_staged = false;  // (h_poses now holds the start poses, d_poses gets them with this copy)
  // One launch per iteration when every workgroup of the evaluation can run the LM step itself for free: one
  // plain residual family per problem in 256-thread workgroups on the L2 path, and the whole grid (chunks + the writer,
  // rounded to the XCDs) resident at once -- the kernel holds one workgroup per CU (ea_lm_iter_kernel).
  {
    const int gx = b->xcd_remap ? 8 * ((b->max_chunks + 1 + 7) / 8) : b->max_chunks + 1;
    r.fused = b->t_fused != 0 && b->nt == 256 && !b->any_variant && b->lds_bytes == 0 && !b->wide &&
              b->terms_are_groups && b->max_chunks > 0 && (int64_t)gx * count <= 256;
    if (r.fused) {
      if (b->iter_alt_count < count) {
        cached_free(b->d_iter_alt);
        b->d_iter_alt = nullptr; b->iter_alt_count = 0;
        HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_iter_alt), (size_t)count * (sizeof(LMState) + sizeof(LMCold)), b->device));
        b->iter_alt_count = count;
      }
      if (b->tiles_cap_alt < b->tiles_cap) {
        cached_free(b->d_partials_alt);
        b->d_partials_alt = nullptr; b->tiles_cap_alt = 0;
        HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_partials_alt), (size_t)b->tiles_cap * kAccSlots * sizeof(double), b->device));
        b->tiles_cap_alt = b->tiles_cap;
      }
    }
    b->last_fused = r.fused ? 1 : 0;
  }
  r.ahead = o.iterations_per_sync > 0 ? o.iterations_per_sync : 2;  // measured: 2 beats 1, 3, 4, 6 by 1-3 %
  r.budget = o.max_num_iterations + 2;  // every pair consumes at least one iteration
  r.enq = 0; r.spins = 0; r.seen = 0; r.done = false; r.fetch = false; r.moved = true;
  return EA_OK;
}

// the batch's LM state for a launch of the step / iteration kernel: `first` = the row range problem 0 folds
static LMLaunch lm_launch(const ea_batch *b, const LMOptions &lo, const GroupDesc &first, int post_done) {
  LMLaunch lm;
  lm.poses = b->d_poses; lm.states = b->d_states; lm.cold = b->d_cold; lm.traces = b->d_traces;
  lm.opt = &lo; lm.progress = b->d_progress;
  lm.host_states = b->dv_states; lm.host_traces = b->dv_traces;  // (final delivery into pinned host memory)
  lm.first = first; lm.post_done = post_done; lm.side = b->any_side;
  return lm;
}

// One launch of ea_lm_iter_kernel: launch j = enq + 1 steps on what launch j - 1 left in the buffers of parity (j - 1) and
// evaluates into those of parity j (launch 0 is a plain evaluation into parity 0, the caller's).  `count` problems fold
// the rows of `fold`; *evaluated (nullable): the rows this launch writes.
static int solve_launch_iter(SolveRun &r, const LMOptions &lo, int count, const GroupDesc &fold, int post_done,
                             double **evaluated = nullptr) {
  ea_batch *b = r.b;
  LMState *st[2] = {b->d_states, reinterpret_cast<LMState *>(b->d_iter_alt)};
  LMCold *cold[2] = {b->d_cold, reinterpret_cast<LMCold *>(b->d_iter_alt + (size_t)b->iter_alt_count * sizeof(LMState))};
  double *rows[2] = {b->d_partials, b->d_partials_alt};
  const int in = r.enq & 1, out = in ^ 1;
  LMIterPairs io;
  io.rows_in = rows[in]; io.rows_out = rows[out]; io.st_in = st[in]; io.st_out = st[out]; io.cold_in = cold[in]; io.cold_out = cold[out];
  HIPCHK(launch_lm_iter(eval_launch(b), b->d_probs, count, b->d_groups, lm_launch(b, lo, fold, post_done), io, b->stream));
  if (evaluated) *evaluated = rows[out];
  return EA_OK;
}

// one look at the run's progress words; enqueues the next (evaluate, step) pair when the device is less than
// `ahead` pairs ahead of the host
static int solve_pump(SolveRun &r, const LMOptions &lo) {
  ea_batch *b = r.b;
  const int count = r.count;
  bool any = false;
  int done = 0;
  for (int i = 0; i < count; ++i) {
    any = any || (__atomic_load_n(&b->h_progress[i], __ATOMIC_ACQUIRE) != 0);
    done = std::max(done, __atomic_load_n(&b->h_progress[count + i], __ATOMIC_ACQUIRE));
  }
  if (!any) { r.done = true; r.moved = true; return EA_OK; }
  if (done != r.seen) { r.seen = done; r.moved = true; }
  if (r.enq < r.budget && r.enq - done < r.ahead) {
    if (r.fused) {
      if (r.enq == 0) {  // launch 0: the plain evaluation at the start pose
        int rc = batch_launch_eval(b);
        if (rc != EA_OK) return rc;
      }
      int rc = solve_launch_iter(r, lo, count, b->group0, /*post_done=*/0);
      if (rc != EA_OK) return rc;
    } else {
      int rc = batch_launch_eval(b);
      if (rc != EA_OK) return rc;
      HIPCHK(launch_lm_step(b->d_groups, count, b->d_partials, lm_launch(b, lo, b->group0, /*post_done=*/0), b->stream));
    }
    ++r.enq;
    r.spins = 0;
    r.moved = true;
  } else if (r.enq >= r.budget) {
    HIPCHK(hipStreamSynchronize(b->stream));
    for (int i = 0; i < count; ++i)
      r.fetch = r.fetch || (__atomic_load_n(&b->h_progress[i], __ATOMIC_ACQUIRE) != 0);
    r.done = true;
  } else if ((++r.spins & 0x3fff) == 0) {
    // nothing to enqueue and no progress for a while: make sure the stream is still healthy
    hipError_t qe = hipStreamQuery(b->stream);
    if (qe != hipSuccess && qe != hipErrorNotReady) return fail(EA_ERR_HIP, hipGetErrorString(qe));
  }
  return EA_OK;
}

// The step kernel that ended a problem's solve has already delivered its final state and trace rows into pinned
// host memory, in front of the flag polled above: no copy, and no wait for the launches queued ahead (they find
// every problem finished and drain behind our back; the next use of the stream is ordered after them anyway).
// Only a solve cut short by the launch budget has to be fetched the classic way.
static int solve_collect(SolveRun &r, const ea_options &o, bool want_traces) {
  ea_batch *b = r.b;
  const int count = r.count;
  if (r.fetch) {
    HIPCHK(hipMemcpyAsync(b->h_states, b->d_states, (size_t)count * (sizeof(LMState) + sizeof(LMTrace)),
                          hipMemcpyDeviceToHost, b->stream));
    if (r.fused && (r.enq & 1))  // a solve cut short is still running: every launch wrote, the last one into the other buffer
      HIPCHK(hipMemcpyAsync(b->h_states, b->d_iter_alt, (size_t)count * sizeof(LMState), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
    if (r.fused)  // a problem that ended earlier stopped alternating buffers: its final state is the delivered one
      for (int i = 0; i < count; ++i)
        if (__atomic_load_n(&b->h_progress[i], __ATOMIC_ACQUIRE) == 0) b->h_states[i] = b->hd_states[i];
    return EA_OK;
  }
  std::memcpy(b->h_states, b->hd_states, (size_t)count * sizeof(LMState));
  if (want_traces || o.minimizer_progress_to_stdout) {
    for (int i = 0; i < count; ++i) {
      // rows 0 .. iteration were delivered; the rest of the pinned block is stale
      const int ni = std::min(b->hd_states[i].iteration + 1, (int)kTrace);
      LMTrace &d = b->h_traces[i];
      const LMTrace &sr = b->hd_traces[i];
      std::memcpy(d.it_cost, sr.it_cost, ni * sizeof(double));
      std::memcpy(d.it_cost_change, sr.it_cost_change, ni * sizeof(double));
      std::memcpy(d.it_gradient_max_norm, sr.it_gradient_max_norm, ni * sizeof(double));
      std::memcpy(d.it_step_norm, sr.it_step_norm, ni * sizeof(double));
      std::memcpy(d.it_relative_decrease, sr.it_relative_decrease, ni * sizeof(double));
      std::memcpy(d.it_radius, sr.it_radius, ni * sizeof(double));
      std::memcpy(d.it_successful, sr.it_successful, ni * sizeof(int));
    }
  }
  return EA_OK;
}

static void solve_report(const SolveRun &r, const ea_options &o, double ms, double *q, double *t, ea_summary *summaries) {
  const ea_batch *b = r.b;
  for (int i = 0; i < r.count; ++i) {
    const LMState &s = b->h_states[i];
    for (int k = 0; k < 4; ++k) q[4 * i + k] = s.x[k];
    for (int k = 0; k < 3; ++k) t[3 * i + k] = s.x[4 + k];
    const LMTrace &tr = b->h_traces[i];
    int64_t npts = b->probs[i]->n;
    for (ea_problem *tm : b->probs[i]->terms) npts += tm->n;
    if (summaries) fill_summary(s, tr, npts, ms, &summaries[i]);
    if (o.minimizer_progress_to_stdout) {
      std::printf("problem %d\niter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius\n", r.first + i);
      const int ni = s.why == EA_WHY_INITIAL_EVAL_FAILED ? 0 : std::min(s.iteration + 1, (int)kTrace);
      for (int it = 0; it < ni; ++it)
        std::printf("%4d  %.6e  % .2e    %.2e   %.2e  % .2e  %.2e\n", it, tr.it_cost[it], tr.it_cost_change[it],
                    tr.it_gradient_max_norm[it], tr.it_step_norm[it], tr.it_relative_decrease[it], tr.it_radius[it]);
    }
  }
}

// The end of every on-device solve: the runs' results (solve_collect), the wall time since the entry point began, then
// poses, summaries and the printed trace (solve_report).
static int solve_finish(SolveRun *runs, size_t nruns, const ea_options &o, std::chrono::steady_clock::time_point t0, double *q,
                        double *t, ea_summary *summaries) {
  for (size_t k = 0; k < nruns; ++k) {
    int rc = solve_collect(runs[k], o, summaries != nullptr);
    if (rc != EA_OK) return rc;
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  for (size_t k = 0; k < nruns; ++k) {
    const SolveRun &r = runs[k];
    solve_report(r, o, ms, q + 4 * r.first, t + 3 * r.first, summaries ? summaries + r.first : nullptr);
  }
  return EA_OK;
}

// Look-ahead rule of the point-sharded solves that keep the exchange on the stream.  The host keeps `ahead` iterations
// queued; iteration i + ahead is enqueued once iteration i is COMPLETE (the step kernel posts that behind its flag) unless
// the solve had finished by iteration i.  The decision depends on (i, the iteration the solve finished at) only --
// quantities every rank agrees on, whenever its host happens to look -- so every rank enqueues exactly (finishing
// iteration + ahead) iterations and the collectives match up without the ranks talking about it.  The device never waits
// for the host: the next iteration is in the queue while this one runs.  (Round 2 enqueued rounds of four behind an event
// wait: the device idled while the host looked and enqueued, 5.1e4 against 8.1e4 iterations/s unsharded on one rank.)
// enqueue_iteration() puts one iteration (launches + collective) on the stream; *finished: the solve was seen finished,
// its result delivered -- else it was cut short by the launch budget and has to be fetched (r.fetch).
template <typename Enqueue>
static int solve_lookahead(SolveRun &r, const ea_options &o, Enqueue &enqueue_iteration, bool *finished) {
  ea_batch *b = r.b;
  const double timeout_ms = resolve_timeout_ms(o);
  int rc;
  *finished = false;
  for (int k = 0; k < r.ahead && r.enq < r.budget; ++k) {
    if ((rc = enqueue_iteration()) != EA_OK) return rc;
    ++r.enq;
  }
  for (int i = 0; i < r.enq; ++i) {
    SpinWait wait(timeout_ms);
    int seen = -1;
    while (__atomic_load_n(&b->h_progress[2], __ATOMIC_ACQUIRE) < i + 1) {
      const int started = __atomic_load_n(&b->h_progress[1], __ATOMIC_ACQUIRE);
      if (started != seen) { seen = started; wait.progress(); }
      else if (wait.poll()) {
        b->needs_drain = true;
        return fail(EA_ERR_HIP, "sharded solve deadline: no progress on the device (is every rank taking part in the collective?)");
      }
    }
    // the flag as iteration i left it; the final state was delivered in front of it
    if (__atomic_load_n(&b->h_progress[0], __ATOMIC_ACQUIRE) == 0 && b->hd_states[0].num_evals <= i + 1) { *finished = true; break; }
    if (r.enq < r.budget) {
      if ((rc = enqueue_iteration()) != EA_OK) return rc;
      ++r.enq;
    }
  }
  r.fetch = !*finished;
  r.done = true;
  return EA_OK;
}

// Sub-batches for the concurrent solve: contiguous slices of the parent's problems, each with its own stream and
// buffers, created on first use and kept.
static int batch_parts(ea_batch *b, int parts) {
  if ((int)b->parts.size() == parts) return EA_OK;
  for (ea_batch *c : b->parts) ea_batch_destroy(c);
  b->parts.clear();
  const int count = (int)b->probs.size();
  for (int k = 0; k < parts; ++k) {
    const int lo = (int)((int64_t)count * k / parts), hi = (int)((int64_t)count * (k + 1) / parts);
    ea_batch *c = nullptr;
    int rc = ea_batch_create(&c, b->probs.data() + lo, hi - lo);
    if (rc != EA_OK) return rc;
    b->parts.push_back(c);
  }
  return EA_OK;
}

// auto_scale: the public call; 0 for the multi-start fall-back, whose starts run with the problem's current loss
static int batch_solve(ea_batch *b, const ea_options *opt_in, double *q, double *t, ea_summary *summaries, bool auto_scale) {
  if (!b || !q || !t) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  static_assert(EA_MAX_TRACE == kTrace, "trace length mismatch");
  const auto t0 = std::chrono::steady_clock::now();
  ea_options o;
  if (int vrc = resolve_options(opt_in, &o)) return vrc;
  if (auto_scale)
    if (int arc = auto_scale_losses(b, q, t)) return arc;
  const LMOptions lo = lm_options(o);
  const int count = (int)b->probs.size();
  // Concurrent halves: a batch of many problems is solved as two sub-batches on two streams, pumped by this one
  // thread.  Inside a batch the evaluation (all CUs busy) and the LM step (one workgroup per problem, pure latency)
  // alternate; with two streams one half's step runs under the other half's evaluation
  // (32 x C2: 0.38 -> 0.32 ms fp32, 0.57 -> 0.46 ms fp64; scripts/archive/split_batch_probe.py).  Every problem's arithmetic
  // is what it is in the one-stream solve of the same batch (same launch shape, same chunks, same order of summation).
  int parts = b->t_streams > 0 ? b->t_streams : (count >= 16 ? 2 : 1);
  parts = std::max(1, std::min(parts, std::min(count, 8)));
  std::vector<SolveRun> runs((size_t)parts);
  if (parts == 1) {
    runs[0].b = b;
  } else {
    // the parts take the launch shape the whole batch resolves to (the heuristics look at the batch's totals), so that
    // every problem is cut into the same chunks, and summed in the same order, as in the one-stream solve
    int rc = batch_build(b);
    if (rc != EA_OK) return rc;
    rc = batch_parts(b, parts);
    if (rc != EA_OK) return rc;
    int first = 0;
    for (int k = 0; k < parts; ++k) {
      ea_batch *c = b->parts[(size_t)k];
      const int use_lds = b->lds_bytes > 0 ? 1 : 0;
      if (c->t_lds_bytes != b->t_lds_bytes || c->t_ppt != b->ppt || c->t_use_lds != use_lds || c->t_xcd != b->xcd_remap ||
          c->t_nt != b->nt || c->t_variant != b->any_variant || c->t_buf != b->buffer_loads || c->t_wide != b->t_wide ||
          c->t_img32 != (b->img32 ? -1 : 0) || c->t_fused != b->t_fused) {
        c->t_lds_bytes = b->t_lds_bytes; c->t_ppt = b->ppt; c->t_use_lds = use_lds; c->t_xcd = b->xcd_remap; c->t_nt = b->nt;
        c->t_variant = b->any_variant; c->t_buf = b->buffer_loads; c->t_wide = b->t_wide; c->t_img32 = b->img32 ? -1 : 0;
        c->t_fused = b->t_fused;  // (solve_start reads the part's own: "fused_iterations" = 0 holds for the parts too)
        c->built = false;
      }
      runs[(size_t)k].b = c;
      runs[(size_t)k].first = first;
      first += (int)c->probs.size();
    }
  }
  for (SolveRun &r : runs) {
    int rc = solve_start(r, o, lo, q + 4 * r.first, t + 3 * r.first);
    if (rc != EA_OK) return rc;
  }
  if (parts > 1) {  // info key "fused_iterations" of the batch the caller holds: every part ran one launch per iteration
    b->last_fused = 1;
    for (const SolveRun &r : runs) b->last_fused &= r.fused ? 1 : 0;
  }
  // The host polls pinned progress words; a deadline bounds the wait: if the device shows no progress (no evaluation
  // completed, nothing to enqueue) for solve_timeout_ms, give up with an error instead of spinning for ever on a kernel
  // that never lowers its flag.  The batches are marked for a drain before their next use.
  SpinWait wait(resolve_timeout_ms(o));
  for (;;) {
    bool all_done = true, moved = false;
    for (SolveRun &r : runs) {
      if (r.done) continue;
      r.moved = false;
      int rc = solve_pump(r, lo);
      if (rc != EA_OK) return rc;
      moved = moved || r.moved;
      all_done = all_done && r.done;
    }
    if (all_done) break;
    if (moved) wait.progress();
    else if (wait.poll()) {
      for (SolveRun &r : runs) r.b->needs_drain = true;
      b->needs_drain = true;
      char msg[160];
      std::snprintf(msg, sizeof msg, "solve deadline: no progress on the device for %.0f ms (ea_options.solve_timeout_ms)", wait.timeout_ms());
      return fail(EA_ERR_HIP, msg);
    }
  }
  return solve_finish(runs.data(), runs.size(), o, t0, q, t, summaries);
}

extern "C" int ea_batch_solve(ea_batch *b, const ea_options *opt_in, double *q, double *t, ea_summary *summaries) {
  return batch_solve(b, opt_in, q, t, summaries, true);
}

extern "C" int ea_batch_bench_eval(ea_batch *b, const double *q, const double *t, int warmup, int steps,
                                   double *ms_total, double *ms_eval_kernel) {
  if (!b || !q || !t || steps < 1 || warmup < 0) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  const int count = (int)b->probs.size();
  rc = batch_upload_poses(b, q, t);
  if (rc != EA_OK) return rc;
  EventPair evp;
  HIPCHK(hipEventCreate(&evp.e0));
  HIPCHK(hipEventCreate(&evp.e1));
  const hipEvent_t e0 = evp.e0, e1 = evp.e1;
  auto one_step = [&]() -> int {
    int r = batch_launch_eval(b);
    if (r != EA_OK) return r;
    HIPCHK(launch_reduce(b->d_groups, count, b->d_partials, b->d_out, b->stream));
    return EA_OK;
  };
  for (int i = 0; i < warmup; ++i) if ((rc = one_step()) != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipEventRecord(e0, b->stream));
  for (int i = 0; i < steps; ++i) if ((rc = one_step()) != EA_OK) return rc;
  HIPCHK(hipEventRecord(e1, b->stream));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  if (ms_total) *ms_total = ms;
  if (ms_eval_kernel) {
    // second pass over the same steps: an event pair around every launch of the per-point kernel
    const int m = std::min(steps, 64);
    EventList evl;
    evl.ev.assign(2 * (size_t)m, nullptr);
    std::vector<hipEvent_t> &ev = evl.ev;
    for (auto &e : ev) HIPCHK(hipEventCreate(&e));
    for (int i = 0; i < m; ++i) {
      HIPCHK(hipEventRecord(ev[2 * i], b->stream));
      if ((rc = batch_launch_eval(b)) != EA_OK) return rc;
      HIPCHK(hipEventRecord(ev[2 * i + 1], b->stream));
      HIPCHK(launch_reduce(b->d_groups, count, b->d_partials, b->d_out, b->stream));
    }
    HIPCHK(hipStreamSynchronize(b->stream));
    double sum = 0.0;
    for (int i = 0; i < m; ++i) {
      float k = 0.f;
      HIPCHK(hipEventElapsedTime(&k, ev[2 * i], ev[2 * i + 1]));
      sum += k;
    }
    *ms_eval_kernel = sum / m;
  }
  return EA_OK;
}

// Capture `steps` x (evaluation + fold) into a hipGraph (untimed set-up).  A step is two dependent launches of ~3 us
// each; enqueued one by one the host needs ~3.1 us per launch and the stream never runs ahead of it
// (profiles/r02_bench_bracket.txt) -- replayed from a graph the same launches execute back to back from the queue.
extern "C" int ea_batch_bench_capture(ea_batch *b, int steps) {
  if (!b || steps < 1) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  if (int prc = ensure_poses_on_device(b)) return prc;
  if (b->bench_graph) { (void)hipGraphExecDestroy(b->bench_graph); b->bench_graph = nullptr; b->bench_graph_steps = 0; b->bench_riding_steps = 0; }
  const int count = (int)b->probs.size();
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal));
  hipError_t e = hipSuccess;
  for (int i = 0; i < steps && e == hipSuccess; ++i) {
    if (batch_launch_eval(b) != EA_OK) { e = hipErrorUnknown; break; }
    e = launch_reduce(b->d_groups, count, b->d_partials, b->d_out, b->stream);
  }
  hipGraph_t graph = nullptr;
  const hipError_t ee = hipStreamEndCapture(b->stream, &graph);
  if (e != hipSuccess || ee != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    return fail(EA_ERR_HIP, std::string("graph capture: ") + hipGetErrorString(e != hipSuccess ? e : ee));
  }
  e = hipGraphInstantiate(&b->bench_graph, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) { b->bench_graph = nullptr; return fail(EA_ERR_HIP, std::string("graph instantiate: ") + hipGetErrorString(e)); }
  b->bench_graph_steps = steps;
  HIPCHK(hipGraphLaunch(b->bench_graph, b->stream));  // one untimed replay: uploads the executable graph
  HIPCHK(hipStreamSynchronize(b->stream));
  return EA_OK;
}

static int bench_ring_ensure(ea_batch *b) {
  const int count = (int)b->probs.size();
  const size_t row_doubles = (size_t)b->tiles_cap * kAccSlots;
  if (b->bench_ring == 2) return EA_OK;
  HIPCHK(hipStreamSynchronize(b->stream));
  bench_ring_free(b);
  HIPCHK(hipMalloc(&b->d_bench_rows, row_doubles * sizeof(double) * 2));
  hipError_t ea = hipMalloc(&b->d_bench_out, sizeof(EvalOut) * (size_t)count * 2);
  if (ea != hipSuccess) { bench_ring_free(b); return fail(EA_ERR_ALLOC, "bench row buffers: allocation failed"); }
  b->bench_ring = 2;
  HIPCHK(hipMemsetAsync(b->d_bench_rows, 0, row_doubles * sizeof(double) * 2, b->stream));
  HIPCHK(hipMemsetAsync(b->d_bench_out, 0, sizeof(EvalOut) * (size_t)count * 2, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  return EA_OK;
}

// K steps as K launches + 1 on the batch's stream: evaluation k with the fold of step k-1 riding in it, rows alternating
// between the two arrays of the ring, a stand-alone fold of the last step's rows into the batch's result array.
static hipError_t enqueue_riding_steps(ea_batch *b, int steps) {
  const int count = (int)b->probs.size();
  const size_t row_doubles = (size_t)b->tiles_cap * kAccSlots;
  double *const own_rows = b->d_partials;
  hipError_t e = hipSuccess;
  for (int i = 0; i < steps && e == hipSuccess; ++i) {
    double *rows = b->d_bench_rows + row_doubles * (size_t)(i & 1);
    if (i == 0) {
      b->d_partials = rows;
      const int lr = batch_launch_eval(b);
      b->d_partials = own_rows;
      if (lr != EA_OK) e = hipErrorUnknown;
    } else {
      const int prev = (i - 1) & 1;
      RidingFold fold;
      fold.groups = b->d_groups; fold.prev_rows = b->d_bench_rows + row_doubles * (size_t)prev; fold.prev_out = b->d_bench_out + (size_t)count * (size_t)prev;
      e = launch_eval_fold(eval_launch(b), b->d_probs, b->nterms, b->d_poses, rows, fold, b->stream);
    }
  }
  if (e == hipSuccess)
    e = launch_reduce_nt(b->nt, b->d_groups, count, b->d_bench_rows + row_doubles * (size_t)((steps - 1) & 1), b->d_out, b->stream);
  return e;
}

// The same K steps with the fold off the evaluations' critical path.  A step is two dependent launches, and the second
// one (one workgroup per problem) leaves the chip idle behind a kernel boundary; the next evaluation does not need its
// result -- the K evaluations of the timed region are independent passes at the resident poses.  Here the fold of step
// k-1 RIDES in the launch of evaluation k (ea_eval_fold_kernel: one extra workgroup per problem), the evaluations
// alternating between two row arrays; a stand-alone fold closes the sequence.  K steps = K launches + 1, every step
// still runs its evaluation and its fold in full, the evaluation kernels still execute one after the other.  The folds
// sum in the order of a workgroup of the evaluation's size (equal to ea_batch_eval's 1024-thread fold up to rounding).
// (A two-branch graph with the folds on a side stream was measured first: the cross-branch edges of a replayed graph
// cost more than the fold -- 9-19 us per step against 5.5 serial, profiles/r02_ab_pipeline.txt.)
extern "C" int ea_batch_bench_capture_pipelined(ea_batch *b, int steps) {
  if (!b || steps < 1) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  if (int prc = ensure_poses_on_device(b)) return prc;
  if (b->any_variant || !b->terms_are_groups || b->lds_bytes > 0 || b->wide)
    return fail(EA_ERR_STATE, "the pipelined form covers plain single-family problems on the L2 path");
  if (b->bench_graph) { (void)hipGraphExecDestroy(b->bench_graph); b->bench_graph = nullptr; b->bench_graph_steps = 0; b->bench_riding_steps = 0; }
  if ((rc = bench_ring_ensure(b)) != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipStreamBeginCapture(b->stream, hipStreamCaptureModeThreadLocal));
  hipError_t e = enqueue_riding_steps(b, steps);
  hipGraph_t graph = nullptr;
  const hipError_t ee = hipStreamEndCapture(b->stream, &graph);
  if (e != hipSuccess || ee != hipSuccess || !graph) {
    if (graph) (void)hipGraphDestroy(graph);
    return fail(EA_ERR_HIP, std::string("graph capture (pipelined): ") + hipGetErrorString(e != hipSuccess ? e : ee));
  }
  e = hipGraphInstantiate(&b->bench_graph, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e != hipSuccess) { b->bench_graph = nullptr; return fail(EA_ERR_HIP, std::string("graph instantiate: ") + hipGetErrorString(e)); }
  b->bench_graph_steps = steps;
  b->bench_riding_steps = steps;
  HIPCHK(hipGraphLaunch(b->bench_graph, b->stream));  // one untimed replay: uploads the executable graph
  HIPCHK(hipStreamSynchronize(b->stream));
  return EA_OK;
}

// The same K launches + 1 enqueued launch by launch instead of replayed from a graph: the first evaluation starts while
// the host is still enqueueing the others (a graph replay hands over all K + 1 packets before the first one runs), which
// is what a short sequence wants -- see profiles/r02_riding_eager_vs_graph.txt.  host_us as in ea_batch_bench_steps.
extern "C" int ea_batch_bench_steps_riding(ea_batch *b, int steps, double *host_us) {
  if (!b || steps < 1) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  if (int prc = ensure_poses_on_device(b)) return prc;
  if (b->any_variant || !b->terms_are_groups || b->lds_bytes > 0 || b->wide)
    return fail(EA_ERR_STATE, "the pipelined form covers plain single-family problems on the L2 path");
  if ((rc = bench_ring_ensure(b)) != EA_OK) return rc;
  if (host_us && (!b->bench_e0 || !b->bench_e1)) {
    HIPCHK(hipEventCreate(&b->bench_e0));
    HIPCHK(hipEventCreate(&b->bench_e1));
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (host_us) HIPCHK(hipEventRecord(b->bench_e0, b->stream));
  const hipError_t e = enqueue_riding_steps(b, steps);
  if (e != hipSuccess) return fail(EA_ERR_HIP, std::string("riding steps: ") + hipGetErrorString(e));
  b->bench_riding_steps = steps;
  if (host_us) HIPCHK(hipEventRecord(b->bench_e1, b->stream));
  const auto t1 = std::chrono::steady_clock::now();
  HIPCHK(hipStreamSynchronize(b->stream));
  if (host_us) {
    host_us[0] = std::chrono::duration<double, std::micro>(t1 - t0).count();
    host_us[1] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count();
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, b->bench_e0, b->bench_e1));
    host_us[2] = ms;
  }
  return EA_OK;
}

// The last-but-one step's result of a pipelined sequence (result slot (steps - 2) & 1): with ea_batch_bench_result this
// covers both a riding fold and the closing stand-alone fold.
extern "C" int ea_batch_bench_result_riding(ea_batch *b, double *cost, double *JtJ, double *Jtr, int64_t *n_invalid) {
  if (!b) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!b->built || b->bench_ring != 2 || b->bench_riding_steps < 2)
    return fail(EA_ERR_STATE, "no pipelined sequence of at least two steps captured or run");
  const int count = (int)b->probs.size();
  HIPCHK(hipMemcpyAsync(b->h_out, b->d_bench_out + (size_t)count * (size_t)((b->bench_riding_steps - 2) & 1), count * sizeof(EvalOut),
                        hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  unpack_eval_out(b, count, cost, JtJ, Jtr, n_invalid);
  return EA_OK;
}

// What the last step of the last ea_batch_bench_steps left in the batch's result array (cost, JtJ, Jtr per problem, the
// layout of ea_batch_eval): lets a caller check that the timed launches computed what ea_batch_eval computes.
extern "C" int ea_batch_bench_result(ea_batch *b, double *cost, double *JtJ, double *Jtr, int64_t *n_invalid) {
  if (!b) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!b->built || !(b->poses_uploaded || b->poses_staged)) return fail(EA_ERR_STATE, "nothing evaluated yet");
  const int count = (int)b->probs.size();
  HIPCHK(hipMemcpyAsync(b->h_out, b->d_out, count * sizeof(EvalOut), hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  unpack_eval_out(b, count, cost, JtJ, Jtr, n_invalid);
  return EA_OK;
}

extern "C" int ea_batch_bench_steps(ea_batch *b, int steps, double *host_us) {
  if (!b || steps < 1) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  if (int prc = ensure_poses_on_device(b)) return prc;
  const int count = (int)b->probs.size();
  // host_us != NULL: also an event pair around the region on the stream ([2] = milliseconds between them): the device's
  // own view of the K steps, from which bench.py takes the evaluation kernel's share of a step
  if (host_us && (!b->bench_e0 || !b->bench_e1)) {
    HIPCHK(hipEventCreate(&b->bench_e0));
    HIPCHK(hipEventCreate(&b->bench_e1));
  }
  const auto t0 = std::chrono::steady_clock::now();
  if (host_us) HIPCHK(hipEventRecord(b->bench_e0, b->stream));
  if (b->bench_graph && b->bench_graph_steps == steps) {
    HIPCHK(hipGraphLaunch(b->bench_graph, b->stream));
  } else {
    for (int i = 0; i < steps; ++i) {
      if ((rc = batch_launch_eval(b)) != EA_OK) return rc;
      HIPCHK(launch_reduce(b->d_groups, count, b->d_partials, b->d_out, b->stream));
    }
  }
  if (host_us) HIPCHK(hipEventRecord(b->bench_e1, b->stream));
  const auto t1 = std::chrono::steady_clock::now();
  HIPCHK(hipStreamSynchronize(b->stream));
  if (host_us) {
    host_us[0] = std::chrono::duration<double, std::micro>(t1 - t0).count();
    host_us[1] = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t1).count();
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, b->bench_e0, b->bench_e1));
    host_us[2] = ms;
  }
  return EA_OK;
}

// Average duration of the per-point kernel when `launches` of them are queued back to back between one event pair:
// the command processor dispatches launch i+1 while launch i executes, so the figure is the kernel's execution
// window (what rocprofv3 --kernel-trace reports), not execution + dispatch as an event pair around a lone launch.
extern "C" int ea_batch_bench_kernel(ea_batch *b, const double *q, const double *t, int warmup, int launches,
                                     double *ms_per_launch) {
  if (!b || !q || !t || !ms_per_launch || launches < 1 || warmup < 0) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  rc = batch_upload_poses(b, q, t);
  if (rc != EA_OK) return rc;
  EventPair evp;
  HIPCHK(hipEventCreate(&evp.e0));
  HIPCHK(hipEventCreate(&evp.e1));
  const hipEvent_t e0 = evp.e0, e1 = evp.e1;
  for (int i = 0; i < warmup; ++i) if ((rc = batch_launch_eval(b)) != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  // hold the stream on a host function while the whole run is enqueued: the launches then execute from the queue,
  // back to back, however fast this thread happens to enqueue them
  HIPCHK(hipLaunchHostFunc(b->stream, [](void *) { std::this_thread::sleep_for(std::chrono::milliseconds(3)); }, nullptr));
  HIPCHK(hipEventRecord(e0, b->stream));
  for (int i = 0; i < launches; ++i) if ((rc = batch_launch_eval(b)) != EA_OK) return rc;
  HIPCHK(hipEventRecord(e1, b->stream));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  *ms_per_launch = (double)ms / launches;
  return EA_OK;
}

// the same measurement for the fold kernel of ea_batch_eval (ea_reduce_kernel over the rows the last evaluation left)
extern "C" int ea_batch_bench_fold(ea_batch *b, int warmup, int launches, double *ms_per_launch) {
  if (!b || !ms_per_launch || launches < 1 || warmup < 0) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  const int count = (int)b->probs.size();
  EventPair evp;
  HIPCHK(hipEventCreate(&evp.e0));
  HIPCHK(hipEventCreate(&evp.e1));
  const hipEvent_t e0 = evp.e0, e1 = evp.e1;
  for (int i = 0; i < warmup; ++i) HIPCHK(launch_reduce(b->d_groups, count, b->d_partials, b->d_out, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipLaunchHostFunc(b->stream, [](void *) { std::this_thread::sleep_for(std::chrono::milliseconds(3)); }, nullptr));
  HIPCHK(hipEventRecord(e0, b->stream));
  for (int i = 0; i < launches; ++i) HIPCHK(launch_reduce(b->d_groups, count, b->d_partials, b->d_out, b->stream));
  HIPCHK(hipEventRecord(e1, b->stream));
  HIPCHK(hipEventSynchronize(e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, e0, e1));
  *ms_per_launch = (double)ms / launches;
  return EA_OK;
}

// ---- materialised mode (the "EAResidue batch Evaluate" view) ------------------------------------------------
// Residual and 1x6 row of every point of every term, in the batch's dtype, into device arrays: the caller's or the
// library's own.  Rows of problem i are [offsets[i], offsets[i+1]) (ea_batch_row_offsets), terms of a problem adjacent,
// points in their storage order (ea_problem_get_points).

static int rows_own_buffers(ea_batch *b) {
  if (b->rows_cap >= b->total_rows && b->d_rows_r) return EA_OK;
  (void)hipFree(b->d_rows_r); (void)hipFree(b->d_rows_J);
  b->d_rows_r = b->d_rows_J = nullptr; b->rows_cap = 0;
  const size_t es = b->dtype == EA_F32 ? 4 : 8;
  const int64_t cap = std::max<int64_t>(b->total_rows, 1);
  HIPCHK(hipMalloc(&b->d_rows_r, (size_t)cap * es));
  hipError_t e = hipMalloc(&b->d_rows_J, (size_t)cap * 6 * es);
  if (e != hipSuccess) { (void)hipFree(b->d_rows_r); b->d_rows_r = nullptr; return fail(EA_ERR_ALLOC, "row arrays: allocation failed"); }
  b->rows_cap = cap;
  return EA_OK;
}

// a caller's device pointer: non-NULL, 16-byte aligned, and -- where this runtime knows the allocation -- device memory of
// the batch's GPU.  (Memory of another HIP runtime in the same process, e.g. the storage of a PyTorch-ROCm tensor, is
// unknown to this runtime's pointer query although kernels can address it: such pointers are taken on trust; the calls that
// refuse them ask device_memory_of, ea_segments.hip.)
int ea::check_device_pointer(int device, const void *ptr, const char *what) {
  if (!ptr) return fail(EA_ERR_INVALID_ARG, std::string(what) + " is NULL");
  if (reinterpret_cast<uintptr_t>(ptr) % 16 != 0) return fail(EA_ERR_INVALID_ARG, std::string(what) + " must be 16-byte aligned");
  hipPointerAttribute_t at;
  const hipError_t e = hipPointerGetAttributes(&at, ptr);
  if (e != hipSuccess) { (void)hipGetLastError(); return EA_OK; }
  if (at.type == hipMemoryTypeHost) return fail(EA_ERR_INVALID_ARG, std::string(what) + " is host memory (device memory expected)");
  if ((at.type == hipMemoryTypeDevice) && at.device != device)
    return fail(EA_ERR_INVALID_ARG, std::string(what) + " lives on another device than the batch");
  return EA_OK;
}

static int rows_launch(ea_batch *b, int corrected, int layout, int staged, int nontemporal, void *r_dev, void *J_dev) {
  RowsLaunch s;
  s.dtype = b->dtype; s.variant = b->any_variant; s.buffer_loads = b->buffer_loads; s.img32 = b->img32;
  s.layout = layout; s.staged = staged; s.corrected = corrected ? 1 : 0; s.nontemporal = nontemporal;
  s.max_n = b->max_n; s.total_rows = b->total_rows;
  HIPCHK(launch_eval_rows(s, b->d_probs, b->nterms, b->d_poses, r_dev, J_dev, b->d_rows_invalid, b->stream));
  return EA_OK;
}

static int rows_prepare(ea_batch *b, const double *q, const double *t, int layout, void **r_dev, void **J_dev, int64_t capacity_rows) {
  if (!b || !q || !t) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (layout != 0 && layout != 1) return fail(EA_ERR_INVALID_ARG, "layout: 0 = J row-major [rows][6], 1 = column-major [6][rows]");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  if ((*r_dev == nullptr) != (*J_dev == nullptr)) return fail(EA_ERR_INVALID_ARG, "r_dev and J_dev: both or neither");
  if (*r_dev) {
    if (capacity_rows < b->total_rows) return fail(EA_ERR_INVALID_ARG, "capacity_rows is smaller than the batch's row count (ea_batch_row_offsets)");
    if ((rc = check_device_pointer(b->device, *r_dev, "r_dev")) != EA_OK) return rc;
    if ((rc = check_device_pointer(b->device, *J_dev, "J_dev")) != EA_OK) return rc;
  } else {
    if ((rc = rows_own_buffers(b)) != EA_OK) return rc;
    *r_dev = b->d_rows_r; *J_dev = b->d_rows_J;
  }
  if (!b->d_rows_invalid) HIPCHK(hipMalloc(&b->d_rows_invalid, sizeof(unsigned int)));
  return batch_upload_poses(b, q, t);
}

extern "C" int ea_batch_row_offsets(ea_batch *b, int64_t *offsets) {
  if (!b || !offsets) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  for (size_t i = 0; i < b->row_offsets.size(); ++i) offsets[i] = b->row_offsets[i];
  return EA_OK;
}

extern "C" int ea_batch_eval_rows_device(ea_batch *b, const double *q, const double *t, int corrected, int layout, void *r_dev,
                                         void *J_dev, int64_t capacity_rows, int64_t *n_invalid) {
  int rc = rows_prepare(b, q, t, layout, &r_dev, &J_dev, capacity_rows);
  if (rc != EA_OK) return rc;
  HIPCHK(hipMemsetAsync(b->d_rows_invalid, 0, sizeof(unsigned int), b->stream));
  const int staged = b->t_rows_staged < 0 ? 1 : (b->t_rows_staged ? 1 : 0), nt = b->t_rows_nt < 0 ? 0 : (b->t_rows_nt ? 1 : 0);
  if ((rc = rows_launch(b, corrected, layout, staged, nt, r_dev, J_dev)) != EA_OK) return rc;
  unsigned int bad = 0;
  HIPCHK(hipMemcpyAsync(&bad, b->d_rows_invalid, sizeof(bad), hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));  // the rows are complete (and visible to any other stream) when this returns
  if (n_invalid) *n_invalid = (int64_t)bad;
  return EA_OK;
}

// the same into host arrays of the batch's dtype (library-owned device arrays + one copy each)
extern "C" int ea_batch_eval_rows(ea_batch *b, const double *q, const double *t, int corrected, int layout, void *r_host,
                                  void *J_host, int64_t capacity_rows, int64_t *n_invalid) {
  if (!b) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (!r_host && !J_host) return fail(EA_ERR_INVALID_ARG, "r_host and J_host are both NULL");
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  if (capacity_rows < b->total_rows) return fail(EA_ERR_INVALID_ARG, "capacity_rows is smaller than the batch's row count (ea_batch_row_offsets)");
  rc = ea_batch_eval_rows_device(b, q, t, corrected, layout, nullptr, nullptr, 0, n_invalid);
  if (rc != EA_OK) return rc;
  const size_t es = b->dtype == EA_F32 ? 4 : 8;
  if (b->total_rows > 0) {
    if (r_host) HIPCHK(hipMemcpy(r_host, b->d_rows_r, (size_t)b->total_rows * es, hipMemcpyDeviceToHost));
    if (J_host) HIPCHK(hipMemcpy(J_host, b->d_rows_J, (size_t)b->total_rows * 6 * es, hipMemcpyDeviceToHost));
  }
  return EA_OK;
}

// `launches` of the materialised-mode kernel queued back to back between one event pair (the stream held on a host
// function while they are enqueued), average execution window per launch.  mode: bit 0 = LDS-staged row-major stores,
// bit 1 = non-temporal stores.  r_dev / J_dev NULL: the library's own arrays.
extern "C" int ea_batch_bench_rows(ea_batch *b, const double *q, const double *t, int corrected, int layout, int mode, void *r_dev,
                                   void *J_dev, int64_t capacity_rows, int warmup, int launches, double *ms_per_launch) {
  if (!ms_per_launch || launches < 1 || warmup < 0) return fail(EA_ERR_INVALID_ARG, "bad argument");
  int rc = rows_prepare(b, q, t, layout, &r_dev, &J_dev, capacity_rows);
  if (rc != EA_OK) return rc;
  HIPCHK(hipMemsetAsync(b->d_rows_invalid, 0, sizeof(unsigned int), b->stream));
  EventPair evp;
  HIPCHK(hipEventCreate(&evp.e0));
  HIPCHK(hipEventCreate(&evp.e1));
  const int staged = mode & 1, nt = (mode >> 1) & 1;
  for (int i = 0; i < warmup; ++i) if ((rc = rows_launch(b, corrected, layout, staged, nt, r_dev, J_dev)) != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(hipLaunchHostFunc(b->stream, [](void *) { std::this_thread::sleep_for(std::chrono::milliseconds(3)); }, nullptr));
  HIPCHK(hipEventRecord(evp.e0, b->stream));
  for (int i = 0; i < launches; ++i) if ((rc = rows_launch(b, corrected, layout, staged, nt, r_dev, J_dev)) != EA_OK) return rc;
  HIPCHK(hipEventRecord(evp.e1, b->stream));
  HIPCHK(hipEventSynchronize(evp.e1));
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, evp.e0, evp.e1));
  *ms_per_launch = (double)ms / launches;
  return EA_OK;
}

extern "C" int ea_batch_set_tuning(ea_batch *b, const char *key, int value) {
  if (!b || !key) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  const std::string k(key);
  if (k == "lds_bytes") b->t_lds_bytes = value;
  else if (k == "points_per_thread") b->t_ppt = value;
  else if (k == "use_lds") b->t_use_lds = value;
  else if (k == "xcd_remap") b->t_xcd = value;
  else if (k == "threads") b->t_nt = value;
  else if (k == "buffer_loads") b->t_buf = value;
  else if (k == "wide_accumulate") b->t_wide = value;
  else if (k == "dt_f32") b->t_img32 = value;
  else if (k == "test_stall_ms") { b->t_test_stall_ms = value; return EA_OK; }
  else if (k == "test_fail_build") { b->t_test_fail_build = value; return EA_OK; }
  else if (k == "solve_streams") { b->t_streams = value; return EA_OK; }
  else if (k == "rows_staged") { b->t_rows_staged = value; return EA_OK; }
  else if (k == "rows_nontemporal") { b->t_rows_nt = value; return EA_OK; }
  else if (k == "poll_results") { b->t_poll = value != 0; return EA_OK; }
  else if (k == "fused_iterations") b->t_fused = value;  // (batch_build reads it when it picks the launch shape: rebuild)
  else if (k == "zero_copy_poses") { b->t_zero_copy = value; return EA_OK; }
  else if (k == "poses_per_launch") { b->t_kp_G = value > 0 ? value : 0; b->kp_K = 0; return EA_OK; }  // (resident poses are dropped)
  else if (k == "poses_order") { b->t_kp_order = value < 0 ? -1 : (value ? 1 : 0); return EA_OK; }
  // (0: the per-wavefront butterfly; read when the pose path is shaped, so resident poses and the pose path's tables are dropped)
  else if (k == "poses_wave_exchange") { b->t_kp_xchg = value < 0 ? kPosesWaveExchangeDefault : value != 0; b->kp_K = 0; b->kp_G = 0; return EA_OK; }
  // (read when poses are set: resident poses are dropped)
  else if (k == "poses_lane_per_pose") { b->t_kp_lanes = value < 0 ? -1 : value; b->kp_K = 0; return EA_OK; }
  else if (k == "starts_events") { b->t_starts_events = value > 0 ? 1 : 0; return EA_OK; }
  else if (k == "cost_form") { b->t_cost_form = value ? 1 : 0; return EA_OK; }  // 0: cost-only calls run the full evaluation (A/B)
  else return fail(EA_ERR_INVALID_ARG, "unknown tuning key: " + k);
  b->built = false;
  return EA_OK;
}

extern "C" int ea_batch_get_info(const ea_batch *b, const char *key, int64_t *value) {
  if (!b || !key || !value) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  const std::string k(key);
  if (k == "num_tiles") *value = b->ntiles;
  else if (k == "points_per_thread") *value = b->ppt;
  else if (k == "lds_bytes") *value = b->lds_bytes;
  else if (k == "xcd_remap") *value = b->xcd_remap;
  else if (k == "chunk") *value = b->chunk;
  else if (k == "threads") *value = b->nt;
  else if (k == "buffer_loads") *value = b->buffer_loads;
  else if (k == "wide_accumulate") *value = b->wide;
  else if (k == "dt_f32") *value = b->img32;
  else if (k == "num_points") { int64_t s = 0; for (auto *p : b->probs) s += p->n; *value = s; }
  else if (k == "num_rows") *value = b->total_rows;
  else if (k == "weighted") *value = b->weighted_terms;  // terms with per-point weights (any: the variant kernels run)
  else if (k == "poses_per_launch") *value = b->kp_G;  // G of the last ea_batch_set_poses (0: none resident)
  else if (k == "poses_points_per_thread") *value = b->kp_ppt;   // launch shape of the pose-batched evaluation
  else if (k == "poses_threads") *value = b->kp_nt;
  else if (k == "poses_tiles") *value = b->kp_ntiles;            // partial rows (= workgroups with work) per pose
  else if (k == "poses_wave_exchange") *value = b->last_kp_xchg;  // the last pose-batched launch: 1 = the wave-exchange reduction
  else if (k == "poses_lane_per_pose") *value = b->last_kp_lanes;  // the last pose-batched call: 1 = one pose per lane (ea_eval_poses_lanes_kernel)
  else if (k == "fused_iterations") *value = b->last_fused;      // the last solve ran one launch per LM iteration (ea_lm_iter_kernel)
  else if (k == "cost_form") *value = b->last_cost_form;         // the last cost-only call: 1 = ea_cost_poses_kernel, 0 = the full evaluation
  else if (k == "starts_form") *value = b->last_starts_form;     // the last ea_batch_solve_starts: 1 = lock-step, 0 = one batch solve per start
  else if (k == "starts_launches") *value = b->last_starts_launches;  // its evaluation launches (lock-step form)
  else if (k == "starts_iterations") *value = b->last_starts_iterations;  // iterations it enqueued (look-ahead included)
  else if (k == "starts_device_ns") *value = b->last_starts_device_ns;    // between the event pair of "starts_events" = 1
  else if (k == "frames_hysteresis_rounds") *value = b->frames_rounds;    // the last batched producer call's looks at the hysteresis flags, both sides (0: Laplacian)
  else if (k == "frames_without_edges") *value = b->frames_without_edges;  // current frames the last ea_batch_set_frames_ros call left alone (0: clean, Laplacian, Canny)
  else if (k == "frames_uploaded") *value = b->frames_uploaded;  // levels[0] of the last ea_batch_set_frames_ros_pyramid call: its host-to-device frame copies
  else return fail(EA_ERR_INVALID_ARG, "unknown info key: " + k);
  return EA_OK;
}

// ---- single-problem conveniences = batch of one ------------------------------------------------

static int self_batch(ea_problem *p, ea_batch **out) {
  if (!p) return fail(EA_ERR_INVALID_ARG, "NULL problem");
  if (!p->self) {
    ea_batch *b = nullptr;
    int rc = ea_batch_create(&b, &p, 1);
    if (rc != EA_OK) return rc;
    p->self = b;
  }
  *out = p->self;
  return EA_OK;
}

int ea::problem_self_batch(ea_problem *p, ea_batch **b) { return self_batch(p, b); }

int ea::problem_call_batch(ea_problem *p, ea_batch **b, bool build) {
  int rc = self_batch(p, b);
  if (rc == EA_OK && build) rc = batch_build(*b);  // (no DT image: EA_ERR_STATE, as ea_eval)
  if (rc != EA_OK) return rc;
  if (p->n == 0) return fail(EA_ERR_STATE, "no edge points (ea_problem_set_points)");
  return EA_OK;
}

extern "C" int ea_eval(ea_problem *p, const double q[4], const double t[3], double *cost, double JtJ[36],
                       double Jtr[6], int64_t *n_invalid) {
  ea_batch *b;
  int rc = self_batch(p, &b);
  if (rc != EA_OK) return rc;
  return ea_batch_eval(b, q, t, cost, JtJ, Jtr, n_invalid);
}

// materialised mode of one problem (its terms included, in term order): rows = ea_problem_num_rows(p)
extern "C" int ea_problem_num_rows(ea_problem *p, int64_t *rows) {
  if (!rows) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  ea_batch *b;
  int rc = self_batch(p, &b);
  if (rc != EA_OK) return rc;
  int64_t off[2];
  rc = ea_batch_row_offsets(b, off);
  if (rc == EA_OK) *rows = off[1];
  return rc;
}

extern "C" int ea_eval_rows(ea_problem *p, const double q[4], const double t[3], int corrected, int layout, void *r_host,
                            void *J_host, int64_t capacity_rows, int64_t *n_invalid) {
  ea_batch *b;
  int rc = self_batch(p, &b);
  if (rc != EA_OK) return rc;
  return ea_batch_eval_rows(b, q, t, corrected, layout, r_host, J_host, capacity_rows, n_invalid);
}

extern "C" int ea_eval_rows_device(ea_problem *p, const double q[4], const double t[3], int corrected, int layout, void *r_dev,
                                   void *J_dev, int64_t capacity_rows, int64_t *n_invalid) {
  ea_batch *b;
  int rc = self_batch(p, &b);
  if (rc != EA_OK) return rc;
  return ea_batch_eval_rows_device(b, q, t, corrected, layout, r_dev, J_dev, capacity_rows, n_invalid);
}

extern "C" int ea_cost(ea_problem *p, const double q[4], const double t[3], double *cost, int64_t *n_invalid) {
  return ea_eval(p, q, t, cost, nullptr, nullptr, n_invalid);
}

// ---- pose covariance (ceres::Covariance at one pose per problem; ea_cov.h) ----------------------------------------------
// One call = the evaluation ea_batch_eval runs (same descriptors, launch shape and fold, so the covariance inverts exactly
// the JtJ ea_eval returns at that pose) -> fold into the device result array -> ea_cov_kernel, one lane per problem: the
// 6x6 Jacobi decomposition, the rank rule, the (pseudo-)inverse and the ambient lift, written straight into pinned host
// memory; the kernel's last workgroup raises the completion flag the host polls (wait_results).  Three launches, one
// synchronisation.  The covariance is a few thousand flops per problem on one lane: a separate kernel behind the fold costs
// one launch gap (~1.5 us) and leaves the fold and the solve kernels exactly as they are.  Nothing of the pose-batched
// path (ea_batch_set_poses) is touched: resident poses survive.
// SIDE: the problems' NormalPriors (a table of `count`) enter the system first, at the pose of the evaluation -- as
// ceres::Covariance counts every residual block; apply_loss_function does not concern them.  The same table carries the
// constant tangent coordinates (PriorDesc::held): the covariance is that of the reduced system (ea_cov.h), priors first.
template <bool SIDE>
static __global__ __launch_bounds__(64) void ea_cov_kernel(const EvalOut *__restrict__ sums, const PoseState *__restrict__ poses,
                                                           CovOptions o, int count, ea_covariance *__restrict__ out,
                                                           unsigned int *__restrict__ counter, int *__restrict__ host_flag, int seq,
                                                           const PriorDesc *__restrict__ priors) {
  const int i = (int)(blockIdx.x * 64 + threadIdx.x);
  if constexpr (SIDE) {
    if (i < count) {
      double acc[kAccSlots], x[7];
      for (int k = 0; k < kAccSlots; ++k) acc[k] = sums[i].acc[k];
      for (int k = 0; k < 4; ++k) x[k] = poses[i].q[k];
      for (int k = 0; k < 3; ++k) x[4 + k] = poses[i].t[k];
      prior_add(priors[i], x, acc);
      cov_from_acc(acc, poses[i].q, 1, o, &out[i], priors[i].held);
    }
  } else {
    if (i < count) cov_from_acc(sums[i].acc, poses[i].q, 1, o, &out[i]);
  }
  __threadfence_system();  // (this wavefront's stores to host memory are visible before it counts itself in)
  if (threadIdx.x == 0) {
    const unsigned int prev = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
    if (prev == gridDim.x - 1) {
      __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      __threadfence_system();
      __hip_atomic_store(host_flag, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
}

extern "C" void ea_default_covariance_options(ea_covariance_options *o) {
  if (!o) return;
  o->algorithm = EA_COV_SPARSE_QR;
  o->min_reciprocal_condition_number = 1e-14;
  o->null_space_rank = 0;
  o->apply_loss_function = 1;
}

int ea::check_cov_options(const ea_covariance_options *o) {
  if (o->algorithm != EA_COV_SPARSE_QR && o->algorithm != EA_COV_DENSE_SVD) return fail(EA_ERR_INVALID_ARG, "unknown covariance algorithm");
  if (o->null_space_rank < -1 || o->null_space_rank > 6) return fail(EA_ERR_INVALID_ARG, "null_space_rank outside [-1, 6]");
  if (!(o->min_reciprocal_condition_number >= 0.0)) return fail(EA_ERR_INVALID_ARG, "min_reciprocal_condition_number must be >= 0");
  return EA_OK;
}

// no problem or batch exists without a device; this answers the "no device" question before a handle is dereferenced
int ea::require_device() {
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt <= 0)
    return fail(EA_ERR_NO_DEVICE, "no HIP device available (libea_hip has no CPU fallback)");
  return EA_OK;
}

int64_t ea::problem_points(const ea_problem *p) {
  int64_t n = p->n;
  for (const ea_problem *t : p->terms) n += t->n;
  return n;
}

static int batch_covariance(ea_batch *b, const double *q, const double *t, const ea_covariance_options *o, ea_covariance *out) {
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  const int count = (int)b->probs.size();
  if (!b->h_cov) {
    HIPCHK(cached_host_malloc(reinterpret_cast<void **>(&b->h_cov), (size_t)count * sizeof(ea_covariance), hipHostMallocMapped, b->device));
    HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->dv_cov), b->h_cov, 0));
  }
  // raw rows: the same descriptors with the loss forced to trivial and the weights dropped (the problems keep their loss, versions and resident poses)
  const ProblemDesc *probs = b->d_probs;
  if (!o->apply_loss_function) {
    const ProblemDesc *hd = reinterpret_cast<const ProblemDesc *>(b->h_desc);  // (batch_build's staging block)
    bool forced = false;
    for (int j = 0; j < b->nterms; ++j) forced = forced || hd[j].loss_kind != EA_LOSS_TRIVIAL || (hd[j].variant & 4);
    if (forced) {
      if (b->cdesc_cap < b->nterms) {
        HIPCHK(hipStreamSynchronize(b->stream));
        cached_free(b->d_cprobs); cached_host_free(b->h_cdesc);
        b->d_cprobs = nullptr; b->h_cdesc = nullptr; b->cdesc_cap = 0;
        HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_cprobs), (size_t)b->nterms * sizeof(ProblemDesc), b->device));
        HIPCHK(cached_host_malloc(reinterpret_cast<void **>(&b->h_cdesc), (size_t)b->nterms * sizeof(ProblemDesc), hipHostMallocDefault, b->device));
        b->cdesc_cap = b->nterms;
      }
      ProblemDesc *cd = reinterpret_cast<ProblemDesc *>(b->h_cdesc);
      // (the per-point weights are part of the loss -- ceres::ScaledLoss -- and go with it: bit 2 cleared, nothing loaded)
      for (int j = 0; j < b->nterms; ++j) { cd[j] = hd[j]; cd[j].loss_kind = EA_LOSS_TRIVIAL; cd[j].variant &= ~4; cd[j].w_off = 0; }
      // (the previous call out of this staging block is complete: every call returns on its results)
      HIPCHK(hipMemcpyAsync(b->d_cprobs, cd, (size_t)b->nterms * sizeof(ProblemDesc), hipMemcpyHostToDevice, b->stream));
      probs = b->d_cprobs;
    }
  }
  if ((rc = batch_upload_poses(b, q, t)) != EA_OK) return rc;
  HIPCHK(launch_eval_fused(eval_launch(b), probs, b->nterms, b->d_poses, b->d_partials, b->stream));
  HIPCHK(launch_reduce(b->d_groups, count, b->d_partials, b->d_out, b->stream));
  const CovOptions co = {o->algorithm, o->min_reciprocal_condition_number, o->null_space_rank};
  b->done_seq = b->done_seq == 0x7fffffff ? 1 : b->done_seq + 1;
  if (b->d_priors)
    hipLaunchKernelGGL(ea_cov_kernel<true>, dim3((count + 63) / 64), dim3(64), 0, b->stream, b->d_out, b->d_poses, co, count, b->dv_cov,
                       b->d_done_count, b->d_progress + 3 * (size_t)count, b->done_seq, b->d_priors);
  else
    hipLaunchKernelGGL(ea_cov_kernel<false>, dim3((count + 63) / 64), dim3(64), 0, b->stream, b->d_out, b->d_poses, co, count, b->dv_cov,
                       b->d_done_count, b->d_progress + 3 * (size_t)count, b->done_seq, nullptr);
  HIPCHK(hipGetLastError());
  if ((rc = wait_results(b)) != EA_OK) return rc;
  std::memcpy(out, b->h_cov, (size_t)count * sizeof(ea_covariance));
  for (int i = 0; i < count; ++i)
    if (problem_points(b->probs[(size_t)i]) == 0) {  // zero sums: "no points" rather than "rank deficient"
      out[i].ok = 0; out[i].why = 3; out[i].rank = 0;
    }
  return EA_OK;
}

extern "C" int ea_batch_covariance(ea_batch *b, const double *q, const double *t, const ea_covariance_options *o, ea_covariance *out) {
  if (!b || !q || !t || !o || !out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = check_cov_options(o);
  if (rc == EA_OK) rc = require_device();
  if (rc != EA_OK) return rc;
  return batch_covariance(b, q, t, o, out);
}

extern "C" int ea_problem_covariance(ea_problem *p, const double q[4], const double t[3], const ea_covariance_options *o,
                                     ea_covariance *out) {
  if (!p || !q || !t || !o || !out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = check_cov_options(o);
  if (rc == EA_OK) rc = require_device();
  if (rc != EA_OK) return rc;
  ea_batch *b;
  if ((rc = self_batch(p, &b)) != EA_OK) return rc;
  if ((rc = batch_build(b)) != EA_OK) return rc;  // (no DT image: EA_ERR_STATE, as ea_eval)
  if (problem_points(p) == 0) return fail(EA_ERR_STATE, "no edge points (ea_problem_set_points)");
  return batch_covariance(b, q, t, o, out);
}

// the reference's integer-pixel cost report (standalone_edge_align.cpp:2494-2567, :2704-2776)
extern "C" int ea_problem_pixel_cost(ea_problem *p, const double q[4], const double t[3], ea_pixel_cost *out) {
  if (!q || !t || !out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  ea_batch *b;
  int rc = self_batch(p, &b);
  if (rc != EA_OK) return rc;
  rc = batch_build(b);
  if (rc != EA_OK) return rc;
  std::memset(out, 0, sizeof(*out));
  out->max_cost = -1.0;
  if (p->n == 0) return EA_OK;
  rc = batch_upload_poses(b, q, t);
  if (rc != EA_OK) return rc;
  struct Partial { double sum, max, max_u, max_v; long long max_index, inside, outside, pad_; };
  const int nwg = (int)((p->n + kBlockThreads - 1) / kBlockThreads);
  DevBuf buf;
  HIPCHK(cached_malloc(&buf.p, (size_t)nwg * sizeof(Partial), p->device));
  HIPCHK(launch_pixel_cost(p->dtype, b->d_probs, 0, (int)p->n, b->d_poses, buf.p, b->stream));
  std::vector<Partial> parts((size_t)nwg);
  HIPCHK(hipMemcpyAsync(parts.data(), buf.p, (size_t)nwg * sizeof(Partial), hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  long long best = 0x7fffffffffffffffLL;
  for (const Partial &w : parts) {  // fixed order: workgroup 0, 1, ...
    out->total_cost += w.sum;
    out->count += w.inside;
    out->outside += w.outside;
    if (w.max > out->max_cost || (w.max == out->max_cost && w.max_index < best)) {
      out->max_cost = w.max; out->max_pixel[0] = w.max_u; out->max_pixel[1] = w.max_v; best = w.max_index;
    }
  }
  out->mean_cost = out->count > 0 ? out->total_cost / (double)out->count : 0.0;
  return EA_OK;
}

void ea::scatter_to_callers_order(const std::vector<int32_t> &order, size_t elem_bytes, const void *tmp, void *out) {
  const unsigned char *src = static_cast<const unsigned char *>(tmp);
  unsigned char *dst = static_cast<unsigned char *>(out);
  for (size_t i = 0; i < order.size(); ++i) std::memcpy(dst + (size_t)order[i] * elem_bytes, src + i * elem_bytes, elem_bytes);
}

extern "C" int ea_eval_points(ea_problem *p, const double q[4], const double t[3], double *r, double *J, int corrected) {
  if (!q || !t) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  ea_batch *b;
  int rc = self_batch(p, &b);
  if (rc != EA_OK) return rc;
  rc = batch_build(b);
  if (rc != EA_OK) return rc;
  if (p->n == 0) return EA_OK;
  rc = batch_upload_poses(b, q, t);
  if (rc != EA_OK) return rc;
  DevBuf buf_r, buf_J;
  if (r) HIPCHK(cached_malloc(&buf_r.p, p->n * sizeof(double), p->device));
  if (J) HIPCHK(cached_malloc(&buf_J.p, p->n * 6 * sizeof(double), p->device));
  double *d_r = buf_r.as<double>(), *d_J = buf_J.as<double>();
  hipError_t e = launch_eval_points(p->dtype, b->d_probs, 0, (int)p->n, b->d_poses, d_r, d_J, corrected, b->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  std::vector<double> tmp(p->order.empty() ? 0 : (size_t)p->n * 6);  // (tile order: by way of tmp)
  const struct { double *out; const double *dev; size_t elem; } rows[2] = {{r, d_r, sizeof(double)}, {J, d_J, 6 * sizeof(double)}};
  for (const auto &w : rows) {
    if (e != hipSuccess || !w.out) continue;
    e = hipMemcpy(tmp.empty() ? w.out : tmp.data(), w.dev, (size_t)p->n * w.elem, hipMemcpyDeviceToHost);
    if (e == hipSuccess && !tmp.empty()) scatter_to_callers_order(p->order, w.elem, tmp.data(), w.out);
  }
  if (e != hipSuccess) return fail(EA_ERR_HIP, hipGetErrorString(e));
  return EA_OK;
}

extern "C" int ea_solve(ea_problem *p, const ea_options *opt, double q[4], double t[3], ea_summary *summary) {
  ea_batch *b;
  int rc = self_batch(p, &b);
  if (rc != EA_OK) return rc;
  return ea_batch_solve(b, opt, q, t, summary);
}

// ---- K trust-region runs per problem, in lock-step on the device (ea_starts_map.h) --------------------------------------
//
// K independent solves of every problem of the batch from K starting poses.  An iteration is one (evaluate, step) launch pair
// per piece of at most G positions of the live list: ea_eval_starts_kernel evaluates the starts still running, as
// ea_batch_eval_poses would evaluate their poses, ea_lm_step_starts_kernel folds each start's rows and runs its state machine;
// the iteration's last step launch compacts the list and posts {iterations complete, n_live} to ONE pinned word.  The host
// keeps `ahead` iterations queued, sizes every grid from the last n_live it has seen (never smaller than the device's: a
// position past the end returns at once) and polls that word alone.  No result depends on K, the other starts, G or the
// moment another start ended: a start's rows are written and folded by its own workgroups in a fixed order.
namespace {
struct StartsLayout { size_t qt, states, live0, alive, nlive, counter, up_bytes, live1, poses, cold, bytes; };
StartsLayout starts_layout(size_t N, size_t K) {
  auto al = [](size_t v) { return (v + 15) & ~(size_t)15; };
  StartsLayout L;
  size_t o = 0;
  L.qt = o; o = al(o + N * 7 * sizeof(double));
  L.states = o; o = al(o + N * sizeof(LMState));
  L.live0 = o; o = al(o + K * sizeof(int));
  L.alive = o; o = al(o + K * sizeof(int));
  L.nlive = o; L.counter = o + 2 * sizeof(int); o += 16;
  L.up_bytes = o;
  L.live1 = o; o = al(o + K * sizeof(int));
  L.poses = o; o = al(o + N * sizeof(PoseState));
  L.cold = o; o = al(o + N * sizeof(LMCold));
  L.bytes = o;
  return L;
}
constexpr size_t kStartsWordBytes = 64;
}  // namespace

static int starts_reserve(ea_batch *b, int N, int K, bool traces) {
  if (N <= b->ms_cap_slots && K <= b->ms_cap_K && (!traces || b->ms_has_traces)) return EA_OK;
  HIPCHK(hipStreamSynchronize(b->stream));  // (launches still reading the old arrays)
  const int cap_n = std::max(N, b->ms_cap_slots), cap_k = std::max(K, b->ms_cap_K);
  const bool tr = traces || b->ms_has_traces;
  starts_free(b);
  const StartsLayout L = starts_layout((size_t)cap_n, (size_t)cap_k);
  HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_ms), L.bytes, b->device));
  HIPCHK(cached_host_malloc(reinterpret_cast<void **>(&b->h_ms_up), L.up_bytes, hipHostMallocDefault, b->device));
  const size_t dl = kStartsWordBytes + (size_t)cap_n * (sizeof(LMState) + (tr ? sizeof(LMTrace) : 0));
  HIPCHK(cached_host_malloc(reinterpret_cast<void **>(&b->h_ms_dl), dl, hipHostMallocMapped, b->device));
  HIPCHK(hipHostGetDevicePointer(reinterpret_cast<void **>(&b->dv_ms_dl), b->h_ms_dl, 0));
  std::memset(b->h_ms_dl, 0, kStartsWordBytes);  // (tag 0 is never posted)
  if (tr) HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_ms_traces), (size_t)cap_n * sizeof(LMTrace), b->device));
  b->ms_cap_slots = cap_n; b->ms_cap_K = cap_k; b->ms_has_traces = tr;
  return EA_OK;
}

// best[i]: the start with the smallest final cost among those that did not fail (ties: the lowest), -1 if none
static void starts_pick_best(int K, int count, const std::vector<int> &termination, const std::vector<double> &cost, int *best) {
  for (int i = 0; i < count; ++i) {
    int arg = -1;
    for (int k = 0; k < K; ++k) {
      const size_t s = (size_t)k * count + i;
      if (termination[s] == EA_FAILURE || !(cost[s] == cost[s])) continue;
      if (arg < 0 || cost[s] < cost[(size_t)arg * count + i]) arg = k;
    }
    best[i] = arg;
  }
}

// the batches the lock-step form does not cover: one batch solve per start
static int starts_fallback(ea_batch *b, int K, const ea_options *opt, double *q, double *t, ea_summary *summaries, int *best) {
  const int count = (int)b->probs.size();
  std::vector<ea_summary> own;
  if (!summaries && best) own.resize((size_t)count);
  std::vector<int> termination((size_t)K * count, EA_FAILURE);
  std::vector<double> cost((size_t)K * count, 0.0);
  for (int k = 0; k < K; ++k) {
    ea_summary *sm = summaries ? summaries + (size_t)k * count : (best ? own.data() : nullptr);
    const int rc = batch_solve(b, opt, q + (size_t)k * count * 4, t + (size_t)k * count * 3, sm, false);
    if (rc != EA_OK) return rc;
    if (sm)
      for (int i = 0; i < count; ++i) { termination[(size_t)k * count + i] = sm[i].termination; cost[(size_t)k * count + i] = sm[i].final_cost; }
  }
  if (best) starts_pick_best(K, count, termination, cost, best);
  return EA_OK;
}

extern "C" int ea_batch_solve_starts(ea_batch *b, int K, const ea_options *opt_in, double *q, double *t, ea_summary *summaries,
                                     int *best) {
  if (!b || !q || !t) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (K < 1 || K > kMaxStartSlots) return fail(EA_ERR_INVALID_ARG, "K out of range: 1 <= K, K x problems <= 16384");
  int rc = require_device();
  if (rc != EA_OK) return rc;
  const int count = (int)b->probs.size();
  if ((int64_t)K * count > kMaxStartSlots) return fail(EA_ERR_INVALID_ARG, "too many starts: K x problems <= 16384");
  const auto t0 = std::chrono::steady_clock::now();
  ea_options o;
  if (int vrc = resolve_options(opt_in, &o)) return vrc;
  const LMOptions lo = lm_options(o);
  if ((rc = batch_build(b)) != EA_OK) return rc;
  const int kept_G = b->kp_K > 0 ? b->kp_G : 0;  // (resident poses keep the launch size they were set with)
  if (b->kp_G == 0) kposes_shape(b);              // (once per build of the batch)
  b->last_starts_launches = 0;
  // (the step kernel folds in the order of a 256-lane workgroup: a pose shape tuned to 1024 threads takes the fall-back too)
  if (!kposes_flat(b) || b->kp_nt != 256) {
    b->last_starts_form = 0;
    return starts_fallback(b, K, opt_in, q, t, summaries, best);
  }
  b->last_starts_form = 1;
  const int N = K * count, G = kposes_group(b, K), rows = b->kp_ntiles;
  rc = kposes_tables(b, G);
  if (kept_G > 0) b->kp_G = kept_G;
  if (rc != EA_OK) return rc;
  const bool traces = summaries != nullptr || o.minimizer_progress_to_stdout;
  if ((rc = starts_reserve(b, N, K, traces)) != EA_OK) return rc;
  const StartsLayout L = starts_layout((size_t)N, (size_t)K);
  // (the previous call's upload out of the staging block was consumed before its first kernel ran, and that call did not
  // return before its kernels had posted)
  double *h_qt = reinterpret_cast<double *>(b->h_ms_up + L.qt);
  LMState *h_st = reinterpret_cast<LMState *>(b->h_ms_up + L.states);
  int *h_live = reinterpret_cast<int *>(b->h_ms_up + L.live0), *h_alive = reinterpret_cast<int *>(b->h_ms_up + L.alive);
  int *h_tail = reinterpret_cast<int *>(b->h_ms_up + L.nlive);
  for (int s = 0; s < N; ++s) {
    const ea_problem *p = b->probs[(size_t)(s % count)];
    lm_init(&h_st[s], &lo, q + 4 * (size_t)s, t + 3 * (size_t)s, p->rot_transposed, p->held);
    for (int k = 0; k < 7; ++k) h_qt[7 * (size_t)s + k] = h_st[s].x[k];
  }
  for (int k = 0; k < K; ++k) { h_live[k] = k; h_alive[k] = count; }
  h_tail[0] = K; h_tail[1] = 0; h_tail[2] = 0; h_tail[3] = 0;
  b->ms_tag = (b->ms_tag + 1) & 0x1ffffu;
  if (b->ms_tag == 0) b->ms_tag = 1;
  const unsigned tag = b->ms_tag;
  if (b->t_test_stall_ms > 0)  // (tests: a device that shows no progress must trip the deadline)
    HIPCHK(hipLaunchHostFunc(b->stream, [](void *ms) { std::this_thread::sleep_for(std::chrono::milliseconds((intptr_t)ms)); },
                             (void *)(intptr_t)b->t_test_stall_ms));
  HIPCHK(hipMemcpyAsync(b->d_ms, b->h_ms_up, L.up_bytes, hipMemcpyHostToDevice, b->stream));
  PoseState *d_poses = reinterpret_cast<PoseState *>(b->d_ms + L.poses);
  HIPCHK(launch_make_poses(reinterpret_cast<const double *>(b->d_ms + L.qt), N, count, b->d_probs, b->d_groups, d_poses, b->stream));
  int *d_live[2] = {reinterpret_cast<int *>(b->d_ms + L.live0), reinterpret_cast<int *>(b->d_ms + L.live1)};
  int *d_nlive = reinterpret_cast<int *>(b->d_ms + L.nlive);
  LMState *hd_states = reinterpret_cast<LMState *>(b->h_ms_dl + kStartsWordBytes);
  LMTrace *hd_traces = reinterpret_cast<LMTrace *>(b->h_ms_dl + kStartsWordBytes + (size_t)b->ms_cap_slots * sizeof(LMState));
  StartsStep a;
  a.groups = b->d_kgroups; a.side = b->d_groups; a.rows = b->d_krows;
  a.poses = d_poses; a.states = reinterpret_cast<LMState *>(b->d_ms + L.states); a.cold = reinterpret_cast<LMCold *>(b->d_ms + L.cold);
  a.traces = traces ? b->d_ms_traces : nullptr;
  a.host_states = reinterpret_cast<LMState *>(b->dv_ms_dl + kStartsWordBytes);
  a.host_traces = traces ? reinterpret_cast<LMTrace *>(b->dv_ms_dl + kStartsWordBytes + (size_t)b->ms_cap_slots * sizeof(LMState)) : nullptr;
  a.alive = reinterpret_cast<int *>(b->d_ms + L.alive);
  a.counter = reinterpret_cast<unsigned int *>(b->d_ms + L.counter);
  a.host_word = reinterpret_cast<unsigned long long *>(b->dv_ms_dl);
  a.count = count; a.rows_per_pose = rows; a.tag = tag;
  const EvalLaunch shape = eval_launch(b, /*kposes=*/true);
  PosesLaunch pl;
  pl.rows = rows; pl.order = std::max(0, b->t_kp_order); pl.single = b->nterms == 1; pl.exchange = b->kp_xchg;
  b->last_kp_xchg = rows > 0 ? b->kp_xchg : 0;
  // iteration j over n (possibly stale) live positions: reads list j & 1, its last step launch writes list (j + 1) & 1
  auto enqueue_iteration = [&](int j, int n) -> int {
    const int per = starts_piece(n, G), in = j & 1;
    a.live_in = d_live[in]; a.n_in = d_nlive + in; a.live_out = d_live[in ^ 1]; a.n_out = d_nlive + (in ^ 1);
    a.iteration = (unsigned)j + 1u;
    for (int off = 0; off < n; off += per) {
      pl.g = std::min(per, n - off);
      HIPCHK(launch_eval_starts(shape, pl, b->d_kprobs, d_poses, b->d_krows, a.live_in, a.n_in, off, b->stream));
      a.off = off; a.last = off + pl.g >= n;
      HIPCHK(launch_lm_step_starts(pl.g, a, lo, b->any_side, b->stream));
      ++b->last_starts_launches;
    }
    return EA_OK;
  };
  const int ahead = o.iterations_per_sync > 0 ? o.iterations_per_sync : 2, budget = o.max_num_iterations + 2;
  EventPair evp;  // ("starts_events": the device's own view of the queued launches, first to last)
  if (b->t_starts_events) {
    HIPCHK(hipEventCreate(&evp.e0));
    HIPCHK(hipEventCreate(&evp.e1));
    HIPCHK(hipEventRecord(evp.e0, b->stream));
  }
  const uint64_t *word = reinterpret_cast<const uint64_t *>(b->h_ms_dl);
  int enq = 0, seen = 0, n_host = K;
  unsigned spins = 0;
  bool fetch = false;
  SpinWait wait(resolve_timeout_ms(o));
  for (;;) {
    int it = 0, nl = K;
    if (!starts_word_read(__atomic_load_n(word, __ATOMIC_ACQUIRE), tag, &it, &nl)) { it = 0; nl = K; }
    if (it != seen) { seen = it; n_host = nl; wait.progress(); }
    if (it > 0 && nl == 0) break;  // every start has ended and delivered
    if (enq < budget && enq - it < ahead) {
      if ((rc = enqueue_iteration(enq, n_host)) != EA_OK) return rc;
      ++enq;
      wait.progress();
    } else if (enq >= budget && it >= enq) {
      fetch = true;  // cut short by the launch budget: some start is still running
      break;
    } else if (wait.poll()) {
      b->needs_drain = true;
      char msg[160];
      std::snprintf(msg, sizeof msg, "solve deadline: no progress on the device for %.0f ms (ea_options.solve_timeout_ms)", wait.timeout_ms());
      return fail(EA_ERR_HIP, msg);
    } else if ((++spins & 0x3fff) == 0) {  // nothing to enqueue and no progress for a while: is the stream still healthy?
      const hipError_t qe = hipStreamQuery(b->stream);
      if (qe != hipSuccess && qe != hipErrorNotReady) { b->needs_drain = true; return fail(EA_ERR_HIP, hipGetErrorString(qe)); }
    }
  }
  b->last_starts_iterations = enq;
  if (b->t_starts_events) {  // (waits for the launches queued ahead as well: they are part of what the call put on the device)
    HIPCHK(hipEventRecord(evp.e1, b->stream));
    HIPCHK(hipEventSynchronize(evp.e1));
    float ems = 0.f;
    HIPCHK(hipEventElapsedTime(&ems, evp.e0, evp.e1));
    b->last_starts_device_ns = (int64_t)((double)ems * 1e6);
  }
  if (fetch) {  // the classic way: states (and trace rows) of every slot from the device, behind a synchronisation
    HIPCHK(hipMemcpyAsync(hd_states, a.states, (size_t)N * sizeof(LMState), hipMemcpyDeviceToHost, b->stream));
    if (traces) HIPCHK(hipMemcpyAsync(hd_traces, b->d_ms_traces, (size_t)N * sizeof(LMTrace), hipMemcpyDeviceToHost, b->stream));
    HIPCHK(hipStreamSynchronize(b->stream));
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  std::vector<int> termination((size_t)N);
  std::vector<double> cost((size_t)N);
  for (int s = 0; s < N; ++s) {
    const LMState &st = hd_states[s];
    for (int k = 0; k < 4; ++k) q[4 * (size_t)s + k] = st.x[k];
    for (int k = 0; k < 3; ++k) t[3 * (size_t)s + k] = st.x[4 + k];
    termination[(size_t)s] = st.termination; cost[(size_t)s] = st.cost;
    if (summaries) fill_summary(st, hd_traces[s], b->probs[(size_t)(s % count)]->n, ms, &summaries[s]);
    if (o.minimizer_progress_to_stdout) {
      const LMTrace &tr = hd_traces[s];
      std::printf("start %d problem %d\niter      cost      cost_change  |gradient|   |step|    tr_ratio  tr_radius\n", s / count, s % count);
      const int ni = st.why == EA_WHY_INITIAL_EVAL_FAILED ? 0 : std::min(st.iteration + 1, (int)kTrace);
      for (int i = 0; i < ni; ++i)
        std::printf("%4d  %.6e  % .2e    %.2e   %.2e  % .2e  %.2e\n", i, tr.it_cost[i], tr.it_cost_change[i], tr.it_gradient_max_norm[i],
                    tr.it_step_norm[i], tr.it_relative_decrease[i], tr.it_radius[i]);
    }
  }
  if (best) starts_pick_best(K, count, termination, cost, best);
  return EA_OK;
}

extern "C" int ea_solve_starts(ea_problem *p, int K, const ea_options *opt, double *q, double *t, ea_summary *summaries, int *best) {
  if (!p || !q || !t) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (K < 1 || K > kMaxStartSlots) return fail(EA_ERR_INVALID_ARG, "K out of range: 1 <= K <= 16384");
  int rc = require_device();
  if (rc != EA_OK) return rc;
  ea_batch *b;
  if ((rc = self_batch(p, &b)) != EA_OK) return rc;
  return ea_batch_solve_starts(b, K, opt, q, t, summaries, best);
}

// ---- ranked search in front of the multi-start solve -----------------------------------------------------------------------
// K candidate poses per problem cost one cost-only evaluation each (ea_batch_cost_resident_poses); the host ranks them out of
// pinned memory (ea_search_rank.h: eligible = finite cost and no failed functor, by ascending cost, ties to the lower index;
// the ineligible behind them by index) and the M best per problem go into ea_batch_solve_starts.  The K candidates stay the
// batch's resident poses.
extern "C" int ea_batch_search_starts(ea_batch *b, int K, const double *q, const double *t, int M, const ea_options *opt,
                                      double *q_out, double *t_out, int *picked, ea_summary *summaries, int *best) {
  if (!b || !q || !t || !q_out || !t_out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (K < 1 || K > (1 << 20)) return fail(EA_ERR_INVALID_ARG, "K out of range");
  // (first for one problem, which needs nothing of the handle; then for the batch's own count)
  if (!search_rank_args_ok(K, M, 1)) return fail(EA_ERR_INVALID_ARG, "M out of range: 1 <= M <= K, M x problems <= 16384");
  const int count = (int)b->probs.size();
  if (!search_rank_args_ok(K, M, count)) return fail(EA_ERR_INVALID_ARG, "M out of range: 1 <= M <= K, M x problems <= 16384");
  int rc = ea_batch_cost_poses(b, K, q, t, nullptr, nullptr);
  if (rc != EA_OK) return rc;
  const size_t n = (size_t)K * count;
  std::vector<double> cost(n);
  std::vector<int64_t> bad(n);
  unpack_eval_out(b->h_kout, (int)n, cost.data(), nullptr, nullptr, bad.data());  // (priors are in: kposes_unpack)
  std::vector<int> own;
  if (!picked) { own.resize((size_t)M * count); picked = own.data(); }
  search_rank(K, M, count, cost.data(), bad.data(), picked);
  for (size_t s = 0; s < (size_t)M * count; ++s) {
    const size_t from = (size_t)picked[s] * count + s % count;
    for (int k = 0; k < 4; ++k) q_out[4 * s + k] = q[4 * from + k];
    for (int k = 0; k < 3; ++k) t_out[3 * s + k] = t[3 * from + k];
  }
  return ea_batch_solve_starts(b, M, opt, q_out, t_out, summaries, best);
}

extern "C" int ea_search_starts(ea_problem *p, int K, const double *q, const double *t, int M, const ea_options *opt,
                                double *q_out, double *t_out, int *picked, ea_summary *summaries, int *best) {
  if (!p || !q || !t || !q_out || !t_out) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (K < 1 || K > (1 << 20)) return fail(EA_ERR_INVALID_ARG, "K out of range");
  if (!search_rank_args_ok(K, M, 1)) return fail(EA_ERR_INVALID_ARG, "M out of range: 1 <= M <= K, M x problems <= 16384");
  int rc = require_device();
  if (rc != EA_OK) return rc;
  ea_batch *b;
  if ((rc = self_batch(p, &b)) != EA_OK) return rc;
  return ea_batch_search_starts(b, K, q, t, M, opt, q_out, t_out, picked, summaries, best);
}

// ---- one problem sharded by points over several processes / GPUs ----------------------------------
// Every rank holds a shard of the edge points and the whole DT image.  Per trust-region iteration: the local fused
// evaluation (device) -> the 32 accumulator slots -> `allreduce` (in-place sum over ranks: RCCL through
// torch.distributed in edge_alignment_amd/dist.py) -> the same state machine on every rank.  The step is a
// deterministic function of the reduced sums, so the ranks stay in lockstep without a broadcast.  The state machine
// runs on the host here (ea_lm.h, the code the device kernels run): the collective returns its result to the host
// anyway.  A rank with an empty shard takes part with zero sums.
extern "C" int ea_solve_sharded(ea_problem *p, const ea_options *opt_in, ea_allreduce_fn allreduce, void *user, double q[4],
                                double t[3], ea_summary *summary) {
  if (!p || !allreduce || !q || !t) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  const auto t0 = std::chrono::steady_clock::now();
  ea_options o;
  if (int vrc = resolve_options(opt_in, &o)) return vrc;
  ea_batch *b = nullptr;
  int rc = self_batch(p, &b);
  if (rc != EA_OK) return rc;
  rc = batch_build(b);
  if (rc != EA_OK) return rc;
  const LMOptions lo = lm_options(o);
  LMState st;
  LMCold cold;
  std::memset(&cold, 0, sizeof(cold));
  std::vector<LMTrace> trv(1);
  LMTrace &tr = trv[0];
  std::memset(&tr, 0, sizeof(tr));
  lm_init(&st, &lo, q, t, p->rot_transposed, p->held);
  int guard = o.max_num_iterations + 4;
  while (st.running && guard-- > 0) {
    const double *pose = st.num_evals == 0 ? st.x : st.cand;
    double acc[kAccSlots];
    if (p->n > 0 || !p->terms.empty()) {
      rc = batch_upload_poses(b, pose, pose + 4);
      if (rc != EA_OK) return rc;
      rc = batch_launch_eval(b);
      if (rc != EA_OK) return rc;
      HIPCHK(launch_reduce(b->d_groups, 1, b->d_partials, b->dv_out, b->stream));  // (straight into pinned host memory)
      HIPCHK(hipStreamSynchronize(b->stream));
      std::memcpy(acc, b->h_out[0].acc, sizeof(acc));
    } else {
      std::memset(acc, 0, sizeof(acc));
    }
    if (allreduce(acc, kAccSlots, user) != 0) return fail(EA_ERR_STATE, "the all-reduce callback reported a failure");
    // the prior once, on the reduced sums (every rank holds the same prior and adds the same bits); constant coordinates:
    // lm_feed masks the system it is given, so the mask too is applied to the all-reduced sums
    if (b->any_side) prior_add(b->h_priors[0], pose, acc);
    lm_feed(&st, &cold, &tr, &lo, acc);
  }
  if (st.running) return fail(EA_ERR_STATE, "sharded solve did not terminate");
  for (int k = 0; k < 4; ++k) q[k] = st.x[k];
  for (int k = 0; k < 3; ++k) t[k] = st.x[4 + k];
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  int64_t npts = p->n;
  for (ea_problem *tm : p->terms) npts += tm->n;
  if (summary) fill_summary(st, tr, npts, ms, summary);
  return EA_OK;
}

// The point-sharded solve with the exchange kept on the stream: evaluation -> fold into the
// caller's device buffer -> the caller's collective, enqueued on the batch's stream -> the device step kernel reading
// that buffer as "one partial row".  The state machine is the device one of ea_solve; the host only enqueues rounds of
// iterations and looks at the pinned progress word between rounds.  Every rank sees the same sums, hence the same
// state after every iteration, hence stops after the same round: the collectives match up without any extra
// communication.
extern "C" int ea_solve_sharded_device(ea_problem *p, const ea_options *opt_in, ea_device_allreduce_fn allreduce, void *user,
                                       double *device_sums, double q[4], double t[3], ea_summary *summary) {
  if (!p || !allreduce || !device_sums || !q || !t) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  if (reinterpret_cast<uintptr_t>(device_sums) % 16 != 0) return fail(EA_ERR_INVALID_ARG, "device_sums must be 16-byte aligned");
  const auto t0 = std::chrono::steady_clock::now();
  ea_options o;
  if (int vrc = resolve_options(opt_in, &o)) return vrc;
  ea_batch *b = nullptr;
  int rc = self_batch(p, &b);
  if (rc != EA_OK) return rc;
  const LMOptions lo = lm_options(o);
  SolveRun r;
  r.b = b;
  rc = solve_start(r, o, lo, q, t);  // builds the batch, uploads pose + state, arms the progress words
  if (rc != EA_OK) return rc;
  if (!b->d_one_row) {
    const GroupDesc one = {0, 1, 0, 1};
    HIPCHK(hipMalloc(&b->d_one_row, sizeof(GroupDesc) + sizeof(PriorDesc)));  // (+ the prior table of one problem behind it)
    HIPCHK(hipMemcpy(b->d_one_row, &one, sizeof(one), hipMemcpyHostToDevice));
  }
  if (b->any_side)  // the step kernel adds the prior once, to the reduced sums: it reads it behind its one-row group table
    HIPCHK(hipMemcpyAsync(b->d_one_row + 1, b->d_priors, sizeof(PriorDesc), hipMemcpyDeviceToDevice, b->stream));
  auto enqueue_iteration = [&]() -> int {
    int rc2 = batch_launch_eval(b);  // (an empty shard launches nothing; its fold below yields zeros)
    if (rc2 != EA_OK) return rc2;
    HIPCHK(launch_reduce(b->d_groups, 1, b->d_partials, reinterpret_cast<EvalOut *>(device_sums), b->stream));
    if (allreduce(device_sums, kAccSlots, (void *)b->stream, user) != 0) {
      b->needs_drain = true;
      return fail(EA_ERR_STATE, "the all-reduce callback reported a failure");
    }
    HIPCHK(launch_lm_step(b->d_one_row, 1, device_sums, lm_launch(b, lo, GroupDesc{0, 1, 0, 1}, /*post_done=*/1), b->stream));
    return EA_OK;
  };
  bool finished;
  if ((rc = solve_lookahead(r, o, enqueue_iteration, &finished)) != EA_OK) return rc;
  // the iterations queued past the end find the solve finished and return at once, their collectives still run (on every
  // rank alike); the caller's buffer must outlive them
  HIPCHK(hipStreamSynchronize(b->stream));
  return solve_finish(&r, 1, o, t0, q, t, summary);
}

// The point-sharded solve in the one-launch-per-iteration form (ea_solve_sharded_comm).  Between evaluation and step sits the
// exchange; with ea_lm_iter_kernel every workgroup folds the rows itself, so what is exchanged is the ROWS: launch j
// evaluates this rank's shard into its rows, ONE in-place all-reduce sums every rank's rows (a few tens of KB instead of 256
// bytes -- the same latency-bound collective), launch j + 1 folds the summed rows, steps and evaluates.  Per iteration: one
// kernel launch + one collective, where the (evaluate, fold, all-reduce, step) form has three launches + one collective.
// Every rank folds the same bits in the same order, so the replicated state machines stay in lockstep as before.
// Ranks may hold different numbers of rows (shards differ by a point): `agree` takes {this rank cannot, its row count} to the
// maximum over the ranks; every rank folds the widest count, its own rows beyond its shard kept at zero.
// *used = 0: some rank's shard does not qualify (see solve_start: another kernel family, or no point at all) -- every rank
// alike, after `agree` and before any exchange, with q, t and the summary untouched; the caller falls back to
// ea_solve_sharded_device.
extern "C" int ea_internal_solve_sharded_rows(ea_problem *p, const ea_options *opt_in, ea_device_allreduce_fn allreduce,
                                              int (*agree)(int vals[2], void *user), void *user, double q[4], double t[3],
                                              ea_summary *summary, int *used) {
  if (!p || !allreduce || !agree || !q || !t || !used) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  *used = 0;
  const auto t0 = std::chrono::steady_clock::now();
  ea_options o;
  if (int vrc = resolve_options(opt_in, &o)) return vrc;
  ea_batch *b = nullptr;
  int rc = self_batch(p, &b);
  if (rc != EA_OK) return rc;
  const LMOptions lo = lm_options(o);
  SolveRun r;
  r.b = b;
  rc = solve_start(r, o, lo, q, t);  // builds the batch, uploads pose + state, arms the progress words, decides r.fused
  if (rc != EA_OK) return rc;
  int vals[2] = {r.fused ? 0 : 1, b->ntiles};
  if (agree(vals, user) != 0) return fail(EA_ERR_STATE, "the ranks could not agree on the shape of the sharded solve");
  if (vals[0] != 0) { HIPCHK(hipStreamSynchronize(b->stream)); return EA_OK; }  // (*used = 0)
  const int max_rows = vals[1];
  if (max_rows > b->tiles_cap || max_rows > b->tiles_cap_alt) {
    HIPCHK(hipStreamSynchronize(b->stream));
    cached_free(b->d_partials); cached_free(b->d_partials_alt);
    b->d_partials = b->d_partials_alt = nullptr;
    b->tiles_cap = b->tiles_cap_alt = 0;
    const int cap = max_rows + 16;
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_partials), (size_t)cap * kAccSlots * sizeof(double), b->device));
    b->tiles_cap = cap;
    HIPCHK(cached_malloc(reinterpret_cast<void **>(&b->d_partials_alt), (size_t)cap * kAccSlots * sizeof(double), b->device));
    b->tiles_cap_alt = cap;
  }
  if (max_rows > b->ntiles)
    for (double *rows : {b->d_partials, b->d_partials_alt})
      HIPCHK(hipMemsetAsync(rows + (size_t)b->ntiles * kAccSlots, 0, (size_t)(max_rows - b->ntiles) * kAccSlots * sizeof(double), b->stream));
  const GroupDesc fold_range = {0, max_rows, 0, 1};
  auto exchange = [&](double *buf) -> int {
    if (allreduce(buf, max_rows * kAccSlots, (void *)b->stream, user) != 0) {
      b->needs_drain = true;
      return fail(EA_ERR_STATE, "the all-reduce callback reported a failure");
    }
    return EA_OK;
  };
  rc = batch_launch_eval(b);  // launch 0: the evaluation at the start pose
  if (rc != EA_OK) return rc;
  if ((rc = exchange(b->d_partials)) != EA_OK) return rc;
  // (solve_lookahead: every rank enqueues the same number of launches and collectives)
  auto enqueue_iteration = [&]() -> int {
    double *evaluated = nullptr;
    int rc2 = solve_launch_iter(r, lo, 1, fold_range, /*post_done=*/1, &evaluated);
    if (rc2 != EA_OK) return rc2;
    return exchange(evaluated);
  };
  bool finished;
  if ((rc = solve_lookahead(r, o, enqueue_iteration, &finished)) != EA_OK) return rc;
  // A finished solve has delivered its result into pinned host memory in front of the flag seen above: return on it.  The
  // launches and collectives queued past the end (every rank alike) drain behind our back -- they touch only buffers the
  // library owns, and whatever uses this stream or the communicator next is ordered behind them (ea_comm_destroy waits for
  // the stream of its last solve).  Only a solve cut short by the launch budget has to wait and fetch.
  if (!finished) HIPCHK(hipStreamSynchronize(b->stream));
  if ((rc = solve_finish(&r, 1, o, t0, q, t, summary)) != EA_OK) return rc;
  *used = 1;
  return EA_OK;
}

// Coarse-to-fine driver (BASELINE config C3; the reference has no pyramid -- SURVEY 8f row 4): levels[0] is the finest
// level; the solve starts on levels[nlevels-1] and carries the pose down level by level.  Every level is a complete
// problem (its own points, DT image and intrinsics scaled by the caller).  A level that fails (termination FAILURE)
// stops the descent and its status is returned through the summaries; q, t hold the last pose reached.
extern "C" int ea_solve_pyramid(ea_problem *const *levels, int nlevels, const ea_options *opt, double q[4], double t[3],
                                ea_summary *summaries) {
  if (!levels || nlevels < 1 || !q || !t) return fail(EA_ERR_INVALID_ARG, "bad argument");
  for (int l = 0; l < nlevels; ++l)
    if (!levels[l]) return fail(EA_ERR_INVALID_ARG, "NULL level");
  for (int l = nlevels - 1; l >= 0; --l) {
    ea_summary local;
    ea_summary *s = summaries ? &summaries[l] : &local;
    const int rc = ea_solve(levels[l], opt, q, t, s);
    if (rc != EA_OK) return rc;
    if (s->termination == EA_FAILURE) {
      for (int k = l - 1; k >= 0 && summaries; --k) std::memset(&summaries[k], 0, sizeof(ea_summary));
      break;
    }
  }
  return EA_OK;
}

// ea_solve_pyramid for every problem of a batch: levels[l] holds the level-l counterparts of the same `count` problems, in the
// same order; one ea_batch_solve per level, the coarsest first, carries all poses down.  A problem whose level ends in FAILURE
// stops there: its pose stays what that level returned and its finer summaries are zero, while its neighbours go on.  Every
// level is solved as the whole batch -- a stopped problem rides along from the pose it holds and what comes back for it is
// thrown away (its finer counterparts see an auto-scaled loss re-estimated, nothing else) -- so every other problem is solved
// by the launches, and to the bits, of a loop of ea_batch_solve over the levels.  summaries: nlevels x count, level-major.
extern "C" int ea_batch_solve_pyramid(ea_batch *const *levels, int nlevels, const ea_options *opt, double *q, double *t,
                                      ea_summary *summaries) {
  if (!levels || nlevels < 1 || !q || !t) return fail(EA_ERR_INVALID_ARG, "bad argument");
  for (int l = 0; l < nlevels; ++l) {
    if (!levels[l]) return fail(EA_ERR_INVALID_ARG, "NULL level");
    if (levels[l]->probs.size() != levels[0]->probs.size()) return fail(EA_ERR_INVALID_ARG, "the levels' batches differ in count");
  }
  const size_t n = levels[0]->probs.size();
  std::vector<unsigned char> stopped(n, 0);
  std::vector<ea_summary> local(summaries ? 0 : n);
  std::vector<double> held_q(4 * n), held_t(3 * n);
  size_t running = n;
  for (int l = nlevels - 1; l >= 0; --l) {
    ea_summary *s = summaries ? summaries + (size_t)l * n : local.data();
    if (running == 0) {
      if (summaries) std::memset(s, 0, n * sizeof(ea_summary));
      continue;
    }
    std::memcpy(held_q.data(), q, 4 * n * sizeof(double));
    std::memcpy(held_t.data(), t, 3 * n * sizeof(double));
    const int rc = ea_batch_solve(levels[l], opt, q, t, s);
    if (rc != EA_OK) return rc;
    for (size_t i = 0; i < n; ++i) {
      if (stopped[i]) {
        std::memcpy(q + 4 * i, &held_q[4 * i], 4 * sizeof(double));
        std::memcpy(t + 3 * i, &held_t[3 * i], 3 * sizeof(double));
        std::memset(&s[i], 0, sizeof(ea_summary));
      } else if (s[i].termination == EA_FAILURE) {
        stopped[i] = 1;
        --running;
      }
    }
  }
  return EA_OK;
}

// ---- self-test of the wavefront reduction primitives (DPP row_mirror / row_half_mirror with bank
// masks, v_permlane16/32_swap, quad_perm): in = 32 slots x 64 lanes (fp32); out32/out64 = the 32 wave
// totals from the fp32 and fp64 reductions; stages (nullable) = 16+8+4+2 rows of 64 lanes.
extern "C" int ea_selftest_wave_reduce(int device, const float *in, double *out32, double *out64, float *stages) {
  if (!in || !out32 || !out64) return fail(EA_ERR_INVALID_ARG, "NULL argument");
  int rc = check_device(device);
  if (rc != EA_OK) return rc;
  HIPCHK(hipSetDevice(device));
  DevBuf b_in, b_st, b_o;
  HIPCHK(hipMalloc(&b_in.p, 32 * 64 * sizeof(float)));
  HIPCHK(hipMalloc(&b_st.p, 30 * 64 * sizeof(float)));
  HIPCHK(hipMalloc(&b_o.p, 64 * sizeof(double)));
  float *d_in = b_in.as<float>(), *d_st = b_st.as<float>();
  double *d_o = b_o.as<double>();
  HIPCHK(hipMemcpy(d_in, in, 32 * 64 * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemset(d_o, 0, 64 * sizeof(double)));
  hipError_t e = launch_selftest_reduce(d_in, d_st, d_st + 16 * 64, d_st + 24 * 64, d_st + 28 * 64, d_o, d_o + 32, nullptr);
  if (e == hipSuccess) e = hipDeviceSynchronize();
  if (e == hipSuccess) e = hipMemcpy(out32, d_o, 32 * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess) e = hipMemcpy(out64, d_o + 32, 32 * sizeof(double), hipMemcpyDeviceToHost);
  if (e == hipSuccess && stages) e = hipMemcpy(stages, d_st, 30 * 64 * sizeof(float), hipMemcpyDeviceToHost);
  if (e != hipSuccess) return fail(EA_ERR_HIP, hipGetErrorString(e));
  return EA_OK;
}

#ifdef EA_STAMPS
static unsigned long long *g_lm_stamps_dev = nullptr;
// diagnostic library only: stamps of the LM step kernel of problem 0 for the next solve(s); 64 x 8 words
extern "C" int ea_debug_lm_stamps_begin(void) {
  if (!g_lm_stamps_dev) HIPCHK(hipMalloc(&g_lm_stamps_dev, 128 * 8 * sizeof(unsigned long long)));
  HIPCHK(hipMemset(g_lm_stamps_dev, 0, 128 * 8 * sizeof(unsigned long long)));
  HIPCHK(set_lm_stamp_buffer(g_lm_stamps_dev));
  return EA_OK;
}
extern "C" int ea_debug_lm_stamps_end(unsigned long long *out) {
  HIPCHK(hipDeviceSynchronize());
  HIPCHK(set_lm_stamp_buffer(nullptr));
  HIPCHK(hipMemcpy(out, g_lm_stamps_dev, 128 * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  return EA_OK;
}
// diagnostic library only: run one fused evaluation and return the s_memtime stamps (8 per workgroup)
extern "C" int ea_debug_eval_stamps(ea_batch *b, const double *q, const double *t, unsigned long long *stamps,
                                    int64_t capacity_wgs, int64_t *n_wgs, int gx_gy[2]) {
  int rc = batch_build(b);
  if (rc != EA_OK) return rc;
  rc = batch_upload_poses(b, q, t);
  if (rc != EA_OK) return rc;
  const int gx = b->xcd_remap ? ((b->max_chunks + 7) / 8) * 8 : b->max_chunks, gy = b->nterms;
  const int64_t wgs = (int64_t)gx * gy;
  if (wgs > capacity_wgs) return fail(EA_ERR_INVALID_ARG, "stamp buffer too small");
  unsigned long long *d = nullptr;
  HIPCHK(hipMalloc(&d, wgs * 8 * sizeof(unsigned long long)));
  HIPCHK(hipMemset(d, 0, wgs * 8 * sizeof(unsigned long long)));
  for (int i = 0; i < 3; ++i) { rc = batch_launch_eval(b); if (rc != EA_OK) return rc; }
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(set_stamp_buffer(d));
  rc = batch_launch_eval(b);
  if (rc != EA_OK) return rc;
  HIPCHK(hipStreamSynchronize(b->stream));
  HIPCHK(set_stamp_buffer(nullptr));
  HIPCHK(hipMemcpy(stamps, d, wgs * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
  (void)hipFree(d);
  *n_wgs = wgs; gx_gy[0] = gx; gx_gy[1] = gy;
  return EA_OK;
}
#endif
