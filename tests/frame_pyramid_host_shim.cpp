// The frame block of ea_batch_set_frames_ros_pyramid (edge_alignment_amd/csrc/ea_frame_ws.h: frame_pyramid) swept on the
// host: a stand-alone program (built by tests/test_frame_pyramid_host.py with -fsanitize=address,undefined) that lays the
// block out over full extents, halvings and level counts, for host and for device frames, and checks that no two regions
// overlap -- every region of every level's workspace and every region of the stage --, that each starts 256-aligned, that
// level l's layout is frame_ws of its extent shifted by level_off[l], that the total stays within the stated bound, and that
// levels = 1 is frame_stage number for number.  It then WALKS the halving chain as the producer does -- three steps per
// launch counted from the full-size frame, a kept level written to its workspace's bgr / depth, the output of step 3 and 6
// staged in a / b when it is no kept level -- checking that every launch finds a source and that every destination is large
// enough for its extent.  What each region must hold is restated from the chain's needs.  Exit status 0 and "ok <cases>".
#include <cstdio>
#include <cstring>
#include <vector>

#include "ea_frame_ws.h"

using namespace ea;
typedef unsigned __int128 u128;

struct Region { const char *name; int level; size_t off, bytes; };

static int fail(const char *what, const Region &r, int H, int W, int halvings, int levels, int host) {
  std::printf("FAILED: %s (region %s of level %d, full %d x %d, halvings %d, levels %d, %s frames)\n", what, r.name, r.level, H, W,
              halvings, levels, host ? "host" : "device");
  return 1;
}

template <typename U>
static void add(std::vector<Region> &v, const char *name, int level, size_t shift, const WsRegion<U> &r) {
  v.push_back({name, level, shift + r.off, r.bytes});
}

static bool same_region(const WsRegion<uint8_t> &a, const WsRegion<uint8_t> &b) { return a.off == b.off && a.bytes == b.bytes; }
static bool same_region(const WsRegion<float> &a, const WsRegion<float> &b) { return a.off == b.off && a.bytes == b.bytes; }

static int check(int H, int W, int halvings, int levels, bool host) {
  const FramePyramid py = frame_pyramid(H, W, halvings, levels, host);
  const Region whole = {"total", -1, 0, py.total};
  const u128 npf = (u128)H * (u128)W;
  std::vector<Region> regions;
  size_t expect_off = 0;
  for (int l = 0; l < levels; ++l) {
    const FrameWs want = frame_ws(H >> (halvings + l), W >> (halvings + l));
    const FrameWs &ws = py.ws[l];
    static_assert(sizeof(FrameWs) == 18 * 2 * sizeof(size_t) + sizeof(size_t), "a region of FrameWs is missing from the table below");
    if (std::memcmp(&ws, &want, sizeof(FrameWs)) != 0) return fail("a level's layout is not frame_ws of its extent", whole, H, W, halvings, levels, host);
    if (py.level_off[l] != expect_off) return fail("the levels do not lie one behind the other", whole, H, W, halvings, levels, host);
    expect_off += want.total;
    const size_t s = py.level_off[l];
    add(regions, "bgr", l, s, ws.bgr); add(regions, "depth", l, s, ws.depth); add(regions, "keep", l, s, ws.keep);
    add(regions, "gray", l, s, ws.gray); add(regions, "lap", l, s, ws.lap); add(regions, "mask", l, s, ws.mask);
    add(regions, "mag", l, s, ws.mag); add(regions, "dir", l, s, ws.dir); add(regions, "label", l, s, ws.label);
    add(regions, "edges", l, s, ws.edges); add(regions, "inv", l, s, ws.inv); add(regions, "changed", l, s, ws.changed);
    add(regions, "counts", l, s, ws.counts); add(regions, "G", l, s, ws.G); add(regions, "dist", l, s, ws.dist);
    add(regions, "scan", l, s, ws.scan); add(regions, "plain", l, s, ws.plain); add(regions, "minmax", l, s, ws.minmax);
  }
  if (py.ws_total != expect_off) return fail("the stage does not begin where the last level ends", whole, H, W, halvings, levels, host);
  const size_t first_stage = regions.size();
  add(regions, "bgr_full", -1, 0, py.bgr_full); add(regions, "depth_full", -1, 0, py.depth_full);
  add(regions, "bgr_a", -1, 0, py.bgr_a); add(regions, "depth_a", -1, 0, py.depth_a);
  add(regions, "bgr_b", -1, 0, py.bgr_b); add(regions, "depth_b", -1, 0, py.depth_b);
  if (py.total % 256 != 0 || py.total < py.ws_total) return fail("the stride is not a multiple of 256 behind the levels", whole, H, W, halvings, levels, host);
  u128 used = 0;
  std::vector<const Region *> sorted;
  for (size_t i = 0; i < regions.size(); ++i) {
    const Region &r = regions[i];
    if (r.bytes == 0) continue;
    used += r.bytes;
    if (r.off % 256 != 0) return fail("a region does not start 256-aligned", r, H, W, halvings, levels, host);
    if ((u128)r.off + (u128)r.bytes > (u128)py.total) return fail("a region ends behind the total", r, H, W, halvings, levels, host);
    if (i >= first_stage && r.off < py.ws_total) return fail("a stage region lies among the levels", r, H, W, halvings, levels, host);
    sorted.push_back(&r);
  }
  // (the regions were appended in layout order: pairwise disjoint == each ends before the next begins)
  for (size_t i = 1; i < sorted.size(); ++i)
    if ((u128)sorted[i - 1]->off + (u128)sorted[i - 1]->bytes > (u128)sorted[i]->off)
      return fail("two regions overlap", *sorted[i], H, W, halvings, levels, host);
  if (used > (u128)py.total) return fail("the regions do not fit the total (size_t overflow?)", whole, H, W, halvings, levels, host);
  // the bound the header states
  u128 bound = 7 * npf + 7 * (npf / 4) + 7 * (npf / 16) + 6 * 256;
  for (int l = 0; l < levels; ++l)
    bound += 32 * (npf >> (2 * (halvings + l))) + 16 * (u128)(W >> (halvings + l)) + 19 * 256;
  if ((u128)frame_pyramid_bound(H, W, halvings, levels) != bound) return fail("frame_pyramid_bound overflows", whole, H, W, halvings, levels, host);
  if ((u128)py.total > bound) return fail("the total exceeds the bound stated in the header", whole, H, W, halvings, levels, host);
  if (!host && (py.bgr_full.bytes || py.depth_full.bytes)) return fail("full-size regions for device frames", whole, H, W, halvings, levels, host);
  if (levels == 1) {
    const FrameStage st = frame_stage(H, W, halvings, host);
    if (st.total != py.total || st.ws_total != py.ws_total || !same_region(st.bgr_full, py.bgr_full) ||
        !same_region(st.depth_full, py.depth_full) || !same_region(st.bgr_a, py.bgr_a) || !same_region(st.depth_a, py.depth_a) ||
        !same_region(st.bgr_b, py.bgr_b) || !same_region(st.depth_b, py.depth_b))
      return fail("levels = 1 is not frame_stage", whole, H, W, halvings, levels, host);
  }
  // the walk of the chain: launches of up to three steps from the full-size frame; the source of the first is the upload
  // (host frames: bgr_full / depth_full, or level 0's bgr / depth without halvings) or the caller's frame in place
  const int T = halvings + levels - 1;
  u128 h = (u128)H, w = (u128)W;
  bool have_src = true;  // (device frames are read in place; host frames are checked below)
  if (host && T > 0) {
    const u128 bsrc = halvings > 0 ? py.bgr_full.bytes : py.ws[0].bgr.bytes, dsrc = halvings > 0 ? py.depth_full.bytes : py.ws[0].depth.bytes;
    if (bsrc < 3 * npf || dsrc < 4 * npf) return fail("the full-size frame has no room", whole, H, W, halvings, levels, host);
  }
  for (int k = 1; k <= T; ++k) {
    if ((h & 1) || (w & 1)) return fail("an odd extent reaches a halving step", whole, H, W, halvings, levels, host);
    h /= 2; w /= 2;
    const bool kept = k >= halvings, launch_end = k % 3 == 0 || k == T;
    if ((k - 1) % 3 == 0 && !have_src) return fail("a launch has no source in memory", whole, H, W, halvings, levels, host);
    if (kept) {
      const FrameWs &ws = py.ws[k - halvings];
      if ((u128)ws.bgr.bytes < 3 * h * w || (u128)ws.depth.bytes < 4 * h * w) return fail("a kept level has no room", whole, H, W, halvings, levels, host);
      have_src = true;
    } else if (launch_end) {
      const u128 b = k == 3 ? py.bgr_a.bytes : py.bgr_b.bytes, d = k == 3 ? py.depth_a.bytes : py.depth_b.bytes;
      if (k != 3 && k != 6) return fail("a staged step other than 3 and 6", whole, H, W, halvings, levels, host);
      if (b < 3 * h * w || d < 4 * h * w) return fail("a staged level has no room", whole, H, W, halvings, levels, host);
      have_src = true;
    } else {
      have_src = false;  // passed through in LDS
    }
  }
  if (py.total <= ((size_t)64 << 20)) {
    std::vector<unsigned char> buf(py.total);
    for (const Region &r : regions)
      if (r.bytes) { buf[r.off] = 1; buf[r.off + r.bytes - 1] = 1; }
  }
  return 0;
}

int main() {
  // {full H, full W}: the GPU tests' extents, the node's frame, a camera's 1280 x 960, small and large frames; with every
  // (halvings, levels) of halvings + levels - 1 <= 8 the extent is divisible for
  const int extents[][2] = {{74, 140}, {296, 560}, {272, 1040}, {24, 48}, {480, 640}, {960, 1280}, {768, 768}, {1024, 4096}, {32768, 32512}, {256, 32768}};
  long long n = 0;
  for (const auto &e : extents)
    for (int halvings = 0; halvings <= 8; ++halvings)
      for (int levels = 1; halvings + levels - 1 <= 8; ++levels) {
        const int T = halvings + levels - 1;
        if ((e[0] & ((1 << T) - 1)) || (e[1] & ((1 << T) - 1)) || (e[0] >> T) < 3 || (e[1] >> T) < 3) continue;
        for (int host = 0; host < 2; ++host) {
          if (check(e[0], e[1], halvings, levels, host != 0)) return 1;
          ++n;
        }
      }
  std::printf("ok %lld\n", n);
  return 0;
}
