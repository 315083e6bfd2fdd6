// ea_frame_ws.h — where every buffer of the frame producers (ea_frames.hip) lies in a problem's workspace, as one pure
// function of the frame's extent that the host tests without a device (tests/frame_ws_host_shim.cpp).  Every producer and
// the tracker's ref_points_begin name the regions they use; nobody carves the workspace by position, so a buffer added here
// moves nothing a later call looks for, and ensure_ws takes the size to allocate from the same function.
//
// Regions of an H x W frame (np = H * W), each starting 256-byte aligned, laid out one behind the other without sharing:
//
//   region   bytes                  written / read by (ea_launch.h)
//   bgr      3 np                   the uploaded colour frame; launch_edge_strength, launch_canny, launch_resize_half_bgr8 (its target)
//   depth    4 np                   the depth frame, uint16 (2 np used) or float: launch_edge_count_scan, launch_edge_scatter[_ros]
//   keep     np                     the caller's mask: launch_gate_by_mask, launch_canny (keep)
//   gray     np                     launch_edge_strength, launch_canny
//   lap      np                     launch_edge_strength -> launch_threshold_median, launch_edge_count_scan, launch_edge_scatter
//   mask     np                     launch_threshold_median -> launch_chamfer
//   mag      4 np                   launch_canny (ints)
//   dir, label, edges, inv   np     launch_canny; edges -> launch_edge_count_scan / _scatter[_ros], inv -> launch_chamfer
//   changed  16 ints                launch_canny: one change flag per launch of a hysteresis batch (8 used);
//                                   launch_canny_frames: two such halves per frame, used by the looks in turn
//   counts   (nblocks + 1) ints     launch_edge_count_scan / launch_edge_scatter[_ros]: per-block counts, nblocks =
//                                   ceil(np / 1024), and the total behind them
//   G, dist  4 np                   launch_chamfer (ints; dist doubles as the float32 distance of the exact transform)
//   scan     4 ceil(H / 32) W ints  launch_chamfer: segment ends and carries of the column pass
//   plain    4 np                   launch_dt_store: the unpadded float image of the debug entry points
//   minmax   2 words                launch_chamfer -> launch_dt_store
//
// The total: 31 np bytes of per-pixel regions; scan = 16 ceil(H / 32) W <= np / 2 + 16 W; counts = 4 (nblocks + 1) <=
// np / 256 + 8; changed and minmax 72; and less than 256 bytes of rounding per region, 18 regions.  So
//   frame_ws(H, W).total <= frame_ws_bound(H, W) = 32 np + 16 W + 19 * 256,
// about 31.5 bytes per pixel (9.2 MiB for 640 x 480); for the largest frame any producer accepts (np <= 2^30) that is below
// 2^36, far inside size_t.
//
// The batched producers (ea_batch_set_frames) use the same layout N times over: frame i of a call lives at i * total bytes
// from frame 0 in a block the batch owns (total is a multiple of 256, so every region keeps its alignment), and a kernel
// reaches its frame's region as `frame 0's pointer + blockIdx.z * total`.  At most 65535 frames of at most 2^30 pixels: below
// 2^52 bytes.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ea {

template <typename U> struct WsRegion {
  size_t off = 0, bytes = 0;
  template <typename V = U> V *at(unsigned char *base) const { return reinterpret_cast<V *>(base + off); }
};

struct FrameWs {
  WsRegion<uint8_t> bgr, depth, keep, gray, lap, mask;
  WsRegion<int> mag;
  WsRegion<uint8_t> dir, label, edges, inv;
  WsRegion<int> changed, counts, G, dist, scan;
  WsRegion<float> plain;
  WsRegion<unsigned int> minmax;
  size_t total = 0;
};

// blocks of launch_edge_count_scan; the total lands in counts[frame_ws_blocks(H, W)]
inline int frame_ws_blocks(int H, int W) { return (int)(((size_t)H * W + 1023) / 1024); }

inline FrameWs frame_ws(int H, int W) {
  const size_t np = (size_t)H * W;
  FrameWs w;
  size_t off = 0;
  auto put = [&off](auto &r, size_t bytes) {
    r.off = off;
    r.bytes = bytes;
    off = (off + bytes + 255) & ~(size_t)255;
  };
  put(w.bgr, 3 * np);
  put(w.depth, 4 * np);
  put(w.keep, np);
  put(w.gray, np);
  put(w.lap, np);
  put(w.mask, np);
  put(w.mag, 4 * np);
  put(w.dir, np);
  put(w.label, np);
  put(w.edges, np);
  put(w.inv, np);
  put(w.changed, 16 * sizeof(int));
  put(w.counts, ((size_t)frame_ws_blocks(H, W) + 1) * sizeof(int));
  put(w.G, 4 * np);
  put(w.dist, 4 * np);
  put(w.scan, 4 * (size_t)((H + 31) / 32) * W * sizeof(int));
  put(w.plain, 4 * np);
  put(w.minmax, 2 * sizeof(unsigned int));
  w.total = off;
  return w;
}

inline size_t frame_ws_bound(int H, int W) { return 32 * (size_t)H * W + 16 * (size_t)W + 19 * 256; }

// The halving stage of ea_batch_set_frames_ros: where the full-resolution frames of one frame pair lie on their way to the
// working resolution (full >> halvings), `halvings` times the 2 x 2 mean.  The stage FOLLOWS the frame's workspace in the
// frame's block -- every offset is from the start of frame_ws(full_H >> halvings, full_W >> halvings), none below its
// total -- so one stride, frame_stage(...).total, takes a kernel from frame z's workspace and stage to frame z + 1's.
// Like frame_ws it is a pure function, swept on the host by tests/frame_stage_host_shim.cpp.
// With npf = full_H * full_W pixels per full-size frame:
//
//   region         bytes         holds
//   bgr_full       3 npf         the uploaded full-size colour frame   (host frames only: a device frame is read in place
//   depth_full     4 npf         the uploaded full-size float depth     by the first halving step)
//   bgr_a, depth_a 3, 4 npf/4    what halving step 0, 2, 4, ... writes when it is not the last  (halvings >= 2)
//   bgr_b, depth_b 3, 4 npf/16   what halving step 1, 3, 5, ... writes when it is not the last  (halvings >= 3)
//
// The last step writes the frame's `bgr` / `depth` regions of the workspace, and a step reads what the step before wrote,
// so step k (extent full >> k -> full >> (k + 1), at most npf / 4^(k + 1) pixels out) fits the partner of its parity.  The
// two sides of a pair use the stage one after the other (the current side has no depth).  halvings == 0: no stage, total
// = the workspace's.  Per full-size pixel that is 7 bytes for host frames, 7/4 with two halvings and 7/16 more with three:
//   frame_stage(...).total <= frame_stage_bound(...) = frame_ws_bound(working extent) + (7 + 7/4 + 7/16) npf + 6 * 256,
// 9.19 bytes per full-size pixel at most (2.19 for device frames) on top of the workspace's 31.5 per working pixel: for
// 640 x 480 frames halved once, 2.3 + 2.1 MiB per frame from host memory.  npf <= 2^30: below 2^34.
struct FrameStage {
  WsRegion<uint8_t> bgr_full;
  WsRegion<float> depth_full;
  WsRegion<uint8_t> bgr_a;
  WsRegion<float> depth_a;
  WsRegion<uint8_t> bgr_b;
  WsRegion<float> depth_b;
  size_t ws_total = 0;  // frame_ws(working extent).total: where the stage begins
  size_t total = 0;     // workspace and stage: the stride from one frame's block to the next
};

inline FrameStage frame_stage(int full_H, int full_W, int halvings, bool host_frames) {
  const size_t npf = (size_t)full_H * full_W;
  FrameStage st;
  st.ws_total = frame_ws(full_H >> halvings, full_W >> halvings).total;
  size_t off = st.ws_total;
  auto put = [&off](auto &r, size_t bytes) {
    r.off = off;
    r.bytes = bytes;
    off = (off + bytes + 255) & ~(size_t)255;
  };
  if (halvings > 0 && host_frames) {
    put(st.bgr_full, 3 * npf);
    put(st.depth_full, 4 * npf);
  }
  if (halvings > 1) {
    put(st.bgr_a, 3 * (npf / 4));
    put(st.depth_a, 4 * (npf / 4));
  }
  if (halvings > 2) {
    put(st.bgr_b, 3 * (npf / 16));
    put(st.depth_b, 4 * (npf / 16));
  }
  st.total = off;
  return st;
}

inline size_t frame_stage_bound(int full_H, int full_W, int halvings) {
  const size_t npf = (size_t)full_H * full_W;
  return frame_ws_bound(full_H >> halvings, full_W >> halvings) + 7 * npf + 7 * (npf / 4) + 7 * (npf / 16) + 6 * 256;
}

// The frame's block of ea_batch_set_frames_ros_pyramid: the workspaces of `levels` pyramid levels of one frame pair, level l
// at the working extent full >> (halvings + l), one behind the other -- level l's regions are frame_ws of its extent shifted
// by level_off[l] -- and behind them the stage, region for region frame_stage's of (full extent, halvings):
//
//   bgr_full, depth_full    the uploaded full-size frames (host frames, halvings >= 1; with halvings == 0 level 0's own
//                           `bgr` / `depth` hold the full-size frame, uploaded as it is)
//   bgr_a, depth_a          (halvings >= 2) the frame after 3 halvings, when that is no kept level (halvings > 3)
//   bgr_b, depth_b          (halvings >= 3) the frame after 6 halvings, when that is no kept level (halvings > 6)
//
// The halving chain (ea_launch.h: launch_halving_chain_*) writes every kept level straight into that level's `bgr` /
// `depth`; it takes kChainSteps = 3 steps per launch, counted from the full-size frame, so a chain of more steps continues
// from what step 3 and step 6 left in HBM: a kept level, or a / b, which are larger than that needs (npf / 64 and npf / 4096
// pixels) because the stage keeps frame_stage's sizes -- levels == 1 IS frame_stage(full, halvings, host_frames), number
// for number, and a caller who moves from one level to several finds the stage where it was.
// One stride, total, takes a kernel from frame z to frame z + 1 on every level and in the stage.
//   frame_pyramid(...).total <= frame_pyramid_bound(...) = sum over l of frame_ws_bound(level l's extent)
//                                                          + (7 + 7/4 + 7/16) npf + 6 * 256;
// the levels' bounds sum to less than 4/3 of level 0's plus 16 W + 19 * 256 per level.  halvings + levels - 1 <= 8.
constexpr int kPyramidMaxLevels = 9;
struct FramePyramid {
  int levels = 0;
  size_t level_off[kPyramidMaxLevels] = {};
  FrameWs ws[kPyramidMaxLevels];  // level l's layout; its regions lie at level_off[l] + their offset
  WsRegion<uint8_t> bgr_full;
  WsRegion<float> depth_full;
  WsRegion<uint8_t> bgr_a;
  WsRegion<float> depth_a;
  WsRegion<uint8_t> bgr_b;
  WsRegion<float> depth_b;
  size_t ws_total = 0;  // all levels' workspaces: where the stage begins
  size_t total = 0;     // the stride from one frame's block to the next
};

inline FramePyramid frame_pyramid(int full_H, int full_W, int halvings, int levels, bool host_frames) {
  const size_t npf = (size_t)full_H * full_W;
  FramePyramid py;
  py.levels = levels;
  size_t off = 0;
  for (int l = 0; l < levels && l < kPyramidMaxLevels; ++l) {
    py.level_off[l] = off;
    py.ws[l] = frame_ws(full_H >> (halvings + l), full_W >> (halvings + l));
    off += py.ws[l].total;  // (a multiple of 256)
  }
  py.ws_total = off;
  auto put = [&off](auto &r, size_t bytes) {
    r.off = off;
    r.bytes = bytes;
    off = (off + bytes + 255) & ~(size_t)255;
  };
  if (halvings > 0 && host_frames) {
    put(py.bgr_full, 3 * npf);
    put(py.depth_full, 4 * npf);
  }
  if (halvings > 1) {
    put(py.bgr_a, 3 * (npf / 4));
    put(py.depth_a, 4 * (npf / 4));
  }
  if (halvings > 2) {
    put(py.bgr_b, 3 * (npf / 16));
    put(py.depth_b, 4 * (npf / 16));
  }
  py.total = off;
  return py;
}

inline size_t frame_pyramid_bound(int full_H, int full_W, int halvings, int levels) {
  const size_t npf = (size_t)full_H * full_W;
  size_t b = 7 * npf + 7 * (npf / 4) + 7 * (npf / 16) + 6 * 256;
  for (int l = 0; l < levels; ++l) b += frame_ws_bound(full_H >> (halvings + l), full_W >> (halvings + l));
  return b;
}

}  // namespace ea
