// The workspace layout of the frame producers (edge_alignment_amd/csrc/ea_frame_ws.h) swept on the host: a stand-alone
// program (built by tests/test_frame_ws_host.py with -fsanitize=address,undefined) that lays out the workspace for small, odd,
// strip-shaped and the largest accepted frames and checks what the producers and their kernels rely on.  What each region
// must hold is restated here from the launchers' needs, not taken from the header's own sizes.  Exit status 0 and
// "ok <shapes>" on success; the first violated property is printed and the status is 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ea_frame_ws.h"

using namespace ea;
typedef unsigned __int128 u128;

struct Region { const char *name; size_t off, bytes; u128 need; };

static int fail(const char *what, const char *region, int H, int W) {
  std::printf("FAILED: %s (region %s, H %d, W %d)\n", what, region, H, W);
  return 1;
}

static int check(int H, int W) {
  const FrameWs w = frame_ws(H, W);
  const u128 np = (u128)H * (u128)W, nblocks = (np + 1023) / 1024, segs = ((u128)H + 31) / 32;
  const Region regions[] = {
      {"bgr", w.bgr.off, w.bgr.bytes, 3 * np},
      {"depth", w.depth.off, w.depth.bytes, 4 * np},  // uint16 or float
      {"keep", w.keep.off, w.keep.bytes, np},
      {"gray", w.gray.off, w.gray.bytes, np},
      {"lap", w.lap.off, w.lap.bytes, np},
      {"mask", w.mask.off, w.mask.bytes, np},
      {"mag", w.mag.off, w.mag.bytes, 4 * np},
      {"dir", w.dir.off, w.dir.bytes, np},
      {"label", w.label.off, w.label.bytes, np},
      {"edges", w.edges.off, w.edges.bytes, np},
      {"inv", w.inv.off, w.inv.bytes, np},
      {"changed", w.changed.off, w.changed.bytes, 16 * 4},
      {"counts", w.counts.off, w.counts.bytes, (nblocks + 1) * 4},
      {"G", w.G.off, w.G.bytes, 4 * np},
      {"dist", w.dist.off, w.dist.bytes, 4 * np},
      {"scan", w.scan.off, w.scan.bytes, 4 * segs * (u128)W * 4},
      {"plain", w.plain.off, w.plain.bytes, 4 * np},
      {"minmax", w.minmax.off, w.minmax.bytes, 2 * 4},
  };
  const int n = (int)(sizeof(regions) / sizeof(regions[0]));
  static_assert(sizeof(FrameWs) == (sizeof(regions) / sizeof(regions[0])) * 2 * sizeof(size_t) + sizeof(size_t),
                "a region of FrameWs is missing from this table");
  // nothing overflows size_t: the same layout in 128-bit arithmetic gives the same offsets, and the total
  u128 wide = 0;
  for (int i = 0; i < n; ++i) {
    const Region &r = regions[i];
    if (r.off % 256 != 0) return fail("a region does not start 256-aligned", r.name, H, W);
    if ((u128)r.bytes < r.need) return fail("a region is smaller than its kernels need", r.name, H, W);
    if ((u128)r.off != wide) return fail("an offset differs from the 128-bit layout (size_t overflow?)", r.name, H, W);
    wide = ((wide + (u128)r.bytes + 255) / 256) * 256;
    if ((u128)r.off + (u128)r.bytes > (u128)w.total) return fail("a region ends behind the total", r.name, H, W);
    for (int j = 0; j < i; ++j) {
      const Region &o = regions[j];
      if ((u128)r.off < (u128)o.off + (u128)o.bytes && (u128)o.off < (u128)r.off + (u128)r.bytes)
        return fail("two regions overlap", r.name, H, W);
    }
  }
  if ((u128)w.total != wide) return fail("the total differs from the 128-bit layout (size_t overflow?)", "total", H, W);
  const u128 bound = 32 * np + 16 * (u128)W + 19 * 256;
  if ((u128)frame_ws_bound(H, W) != bound) return fail("frame_ws_bound overflows", "total", H, W);
  if ((u128)w.total > bound) return fail("the total exceeds the bound derived in the header", "total", H, W);
  if ((u128)frame_ws_blocks(H, W) != nblocks) return fail("frame_ws_blocks", "counts", H, W);
  // the regions are real: a buffer of `total` bytes takes a write to the first and last byte of each (small frames only)
  if (w.total <= ((size_t)64 << 20)) {
    std::vector<unsigned char> buf(w.total);
    for (int i = 0; i < n; ++i) {
      buf[regions[i].off] = 1;
      buf[regions[i].off + regions[i].bytes - 1] = 1;
    }
    if (w.bgr.at(buf.data()) != buf.data() || (unsigned char *)w.minmax.at(buf.data()) != buf.data() + w.minmax.off ||
        (unsigned char *)w.depth.at<float>(buf.data()) != buf.data() + w.depth.off)
      return fail("at() is base + offset", "minmax", H, W);
  }
  return 0;
}

int main() {
  const int sweep[] = {3, 4, 31, 32, 33, 63, 64, 65, 255, 256, 257};
  const int more[][2] = {{480, 640}, {1536, 2048}, {3, 16384}, {32768, 3}, {32767, 32768}};
  long long shapes = 0;
  for (int H : sweep)
    for (int W : sweep) {
      if (check(H, W)) return 1;
      ++shapes;
    }
  for (const auto &hw : more) {
    if (check(hw[0], hw[1])) return 1;
    ++shapes;
  }
  std::printf("ok %lld\n", shapes);
  return 0;
}
