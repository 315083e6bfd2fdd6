// The halving stage of ea_batch_set_frames_ros (edge_alignment_amd/csrc/ea_frame_ws.h: frame_stage) swept on the host: a
// stand-alone program (built by tests/test_frame_stage_host.py with -fsanitize=address,undefined) that lays the stage out
// for the extents the GPU tests use, the node's 640 x 480 with 0..3 halvings and the largest accepted frames, for host and
// for device frames, and then WALKS the halving steps as batch_stage_ros does -- full -> a -> b -> a ... -> the workspace --
// checking that every step's source and destination exist, are large enough for the step's extent, and differ.  What each
// region must hold is restated here from the steps' needs, not taken from the header's own sizes.  Exit status 0 and
// "ok <cases>" on success; the first violated property is printed and the status is 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ea_frame_ws.h"

using namespace ea;
typedef unsigned __int128 u128;

struct Region { const char *name; size_t off, bytes; };

static int fail(const char *what, const char *region, int H, int W, int halvings, int host) {
  std::printf("FAILED: %s (region %s, full %d x %d, halvings %d, %s frames)\n", what, region, H, W, halvings, host ? "host" : "device");
  return 1;
}

static int check(int H, int W, int halvings, bool host) {
  const FrameStage st = frame_stage(H, W, halvings, host);
  const FrameWs ws = frame_ws(H >> halvings, W >> halvings);
  const u128 npf = (u128)H * (u128)W;
  const Region regions[] = {
      {"bgr_full", st.bgr_full.off, st.bgr_full.bytes}, {"depth_full", st.depth_full.off, st.depth_full.bytes},
      {"bgr_a", st.bgr_a.off, st.bgr_a.bytes},          {"depth_a", st.depth_a.off, st.depth_a.bytes},
      {"bgr_b", st.bgr_b.off, st.bgr_b.bytes},          {"depth_b", st.depth_b.off, st.depth_b.bytes},
  };
  const int n = (int)(sizeof(regions) / sizeof(regions[0]));
  static_assert(sizeof(FrameStage) == (sizeof(regions) / sizeof(regions[0])) * 2 * sizeof(size_t) + 2 * sizeof(size_t),
                "a region of FrameStage is missing from this table");
  if (st.ws_total != ws.total) return fail("the stage does not begin where the workspace ends", "ws_total", H, W, halvings, host);
  if (st.total % 256 != 0 || st.total < ws.total) return fail("the stride is not a multiple of 256 behind the workspace", "total", H, W, halvings, host);
  u128 used = 0;
  for (int i = 0; i < n; ++i) {
    const Region &r = regions[i];
    if (r.bytes == 0) continue;  // (a region this case does not have)
    used += r.bytes;
    if (r.off % 256 != 0) return fail("a region does not start 256-aligned", r.name, H, W, halvings, host);
    if ((u128)r.off < (u128)ws.total) return fail("a region overlaps the frame's workspace", r.name, H, W, halvings, host);
    if ((u128)r.off + (u128)r.bytes > (u128)st.total) return fail("a region ends behind the total", r.name, H, W, halvings, host);
    for (int k = 0; k < i; ++k) {
      const Region &o = regions[k];
      if (o.bytes && (u128)r.off < (u128)o.off + (u128)o.bytes && (u128)o.off < (u128)r.off + (u128)r.bytes)
        return fail("two regions overlap", r.name, H, W, halvings, host);
    }
  }
  // the bound the header states: the workspace's, 7 + 7/4 + 7/16 bytes per full-size pixel, 6 regions' rounding
  const u128 bound = (32 * (npf >> (2 * halvings)) + 16 * (u128)(W >> halvings) + 19 * 256) + 7 * npf + 7 * (npf / 4) + 7 * (npf / 16) + 6 * 256;
  if ((u128)frame_stage_bound(H, W, halvings) != bound) return fail("frame_stage_bound overflows", "total", H, W, halvings, host);
  if ((u128)st.total > bound) return fail("the total exceeds the bound stated in the header", "total", H, W, halvings, host);
  if (used + (u128)ws.total > (u128)st.total) return fail("the regions do not fit the total (size_t overflow?)", "total", H, W, halvings, host);
  if (halvings == 0 && st.total != ws.total) return fail("a stage without halvings", "total", H, W, halvings, host);
  if (!host && (st.bgr_full.bytes || st.depth_full.bytes)) return fail("full-size regions for device frames", "bgr_full", H, W, halvings, host);
  // the walk of batch_stage_ros: step k reads what step k - 1 wrote (step 0: the full-size frame) and writes a (k even) or b
  // (k odd), the last step the workspace's bgr / depth
  u128 h = (u128)H, w = (u128)W;
  const Region *bsrc = host ? &regions[0] : nullptr, *dsrc = host ? &regions[1] : nullptr;  // (device frames: read in place)
  const Region ws_bgr = {"ws.bgr", ws.bgr.off, ws.bgr.bytes}, ws_depth = {"ws.depth", ws.depth.off, ws.depth.bytes};
  for (int k = 0; k < halvings; ++k) {
    if ((h & 1) || (w & 1)) return fail("an odd extent reaches a halving step", "walk", H, W, halvings, host);
    const bool last = k == halvings - 1;
    const Region *bdst = last ? &ws_bgr : (k & 1) ? &regions[4] : &regions[2];
    const Region *ddst = last ? &ws_depth : (k & 1) ? &regions[5] : &regions[3];
    if (bsrc && (u128)bsrc->bytes < 3 * h * w) return fail("a step's colour source is too small", bsrc->name, H, W, halvings, host);
    if (dsrc && (u128)dsrc->bytes < 4 * h * w) return fail("a step's depth source is too small", dsrc->name, H, W, halvings, host);
    h /= 2; w /= 2;
    if ((u128)bdst->bytes < 3 * h * w) return fail("a step's colour destination is too small", bdst->name, H, W, halvings, host);
    if ((u128)ddst->bytes < 4 * h * w) return fail("a step's depth destination is too small", ddst->name, H, W, halvings, host);
    if (bdst == bsrc || ddst == dsrc) return fail("a step writes what it reads", bdst->name, H, W, halvings, host);
    bsrc = bdst; dsrc = ddst;
  }
  if (h != (u128)(H >> halvings) || w != (u128)(W >> halvings)) return fail("the walk ends at another extent", "walk", H, W, halvings, host);
  // the regions are real: a buffer of `total` bytes takes a write to the first and last byte of each (small frames only)
  if (st.total <= ((size_t)64 << 20)) {
    std::vector<unsigned char> buf(st.total);
    for (int i = 0; i < n; ++i)
      if (regions[i].bytes) {
        buf[regions[i].off] = 1;
        buf[regions[i].off + regions[i].bytes - 1] = 1;
      }
    if (halvings > 1 && (unsigned char *)st.depth_a.at(buf.data()) != buf.data() + st.depth_a.off)
      return fail("at() is base + offset", "depth_a", H, W, halvings, host);
  }
  return 0;
}

int main() {
  // {full H, full W, halvings}: the GPU tests' extents, the node's frame with 0..3 halvings, 8 halvings, the largest frames
  const int cases[][3] = {{12, 12, 2},    {74, 140, 1},   {256, 1028, 2}, {480, 640, 0},    {480, 640, 1},     {480, 640, 2},
                          {480, 640, 3},  {3, 3, 0},      {6, 6, 1},      {768, 768, 8},    {1024, 4096, 5},   {32768, 32766, 1},
                          {32764, 32768, 2}, {24, 32768, 3}, {32768, 24, 3}, {32767, 32768, 0}};
  long long n = 0;
  for (const auto &c : cases)
    for (int host = 0; host < 2; ++host) {
      if (check(c[0], c[1], c[2], host != 0)) return 1;
      ++n;
    }
  std::printf("ok %lld\n", n);
  return 0;
}
