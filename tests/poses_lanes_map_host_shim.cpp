// The work-list mapping of ea_eval_poses_lanes_kernel (edge_alignment_amd/csrc/ea_poses_map.h: one pose per lane, a work item
// is (row of a pose, group of 64 consecutive poses)) swept on the host: a stand-alone program (built by
// tests/test_poses_lanes_map_host.py with -fsanitize=address,undefined) that walks every workgroup of a launch in dispatch
// order and checks what the kernel and its launcher rely on.  Exit status 0 and "ok <cases>" on success; the first violated
// property is printed and the status is 1.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ea_poses_map.h"

using namespace ea;

static int fail(const char *what, int rows, int g, int riders, int order, long long at) {
  std::printf("FAILED: %s (rows %d, g %d, riders %d, order %d, at %lld)\n", what, rows, g, riders, order, at);
  return 1;
}

// one launch: terms of `chunks[j]` chunks each (rows = their sum), g poses, `riders` riders, `count` problems
static int check(const std::vector<int> &chunks, int g, int riders, int order, bool xcd) {
  const int nterms = (int)chunks.size(), count = nterms;
  int rows = 0;
  std::vector<PosesRow> table;
  std::vector<int> row0(nterms + 1, 0);
  for (int j = 0; j < nterms; ++j) {
    for (int c = 0; c < chunks[j]; ++c) table.push_back(PosesRow{j, rows, count, 0});
    rows += chunks[j];
    row0[j + 1] = rows;
  }
  if (rows == 0) return 0;  // (the host enqueues the fold alone)
  const bool single = nterms == 1;
  const int shape = poses_shape(xcd, order, single, riders);
  const int groups = poses_lanes_groups(g);
  if (groups != (g + 63) / 64) return fail("groups = ceil(g / 64)", rows, g, riders, order, groups);
  const unsigned grid = poses_lanes_grid(rows, g, riders);
  const long long T = (long long)rows * groups, per = (T + 7) / 8;
  if (grid != (unsigned)poses_shape_slots(shape) + 8u * (unsigned)per) return fail("grid = rider slots + 8 ceil(T / 8)", rows, g, riders, order, grid);
  std::vector<int> seen_rider(riders, 0), per_xcd(8, 0);
  std::vector<int> seen((size_t)rows * g, 0);  // indexed by the partial row pose * rows + row
  long long empty = 0, items = 0;
  bool eval_started = false;
  int prev_row = -1;
  for (unsigned L = 0; L < grid; ++L) {
    const PosesLanesWork w = poses_lanes_work(L, shape, rows, g, riders);
    if (w.kind == 0) { ++empty; continue; }
    if (w.kind == 1) {
      if (eval_started) return fail("a rider behind an evaluation item in dispatch order", rows, g, riders, order, L);
      if (w.rider < 0 || w.rider >= riders) return fail("rider out of range", rows, g, riders, order, L);
      ++seen_rider[w.rider];
      continue;
    }
    eval_started = true;
    ++items;
    if (w.row < 0 || w.row >= rows) return fail("row out of range", rows, g, riders, order, L);
    if (w.pose0 < 0 || w.pose0 >= g || w.pose0 % kPosesLanes != 0) return fail("first pose of a group", rows, g, riders, order, L);
    const int want = g - w.pose0 < kPosesLanes ? g - w.pose0 : kPosesLanes;
    if (w.live != want || w.live < 1) return fail("live lanes", rows, g, riders, order, L);
    const PosesLanesChunk c = poses_lanes_chunk(w.row, shape, single ? nullptr : table.data());
    if (c.term < 0 || c.term >= nterms) return fail("term out of range", rows, g, riders, order, L);
    if (c.chunk < 0 || c.chunk >= chunks[c.term] || row0[c.term] + c.chunk != w.row) return fail("chunk outside its term", rows, g, riders, order, L);
    if (c.count != count) return fail("problem count", rows, g, riders, order, L);
    for (int l = 0; l < w.live; ++l) ++seen[(size_t)(w.pose0 + l) * rows + w.row];
    if (xcd) {
      ++per_xcd[L & 7];
      // order 0: the items of one XCD residue class walk contiguous rows (its points and image rows stay in one L2)
      if (!order && (L & 7) == 0) {
        if (w.row < prev_row) return fail("an XCD's rows run backwards", rows, g, riders, order, L);
        prev_row = w.row;
      }
    }
  }
  for (int r = 0; r < riders; ++r) if (seen_rider[r] != 1) return fail("every rider exactly once", rows, g, riders, order, r);
  for (size_t t = 0; t < seen.size(); ++t) if (seen[t] != 1) return fail("every (row, pose) exactly once", rows, g, riders, order, (long long)t);
  if (items != T) return fail("rows x groups items", rows, g, riders, order, items);
  for (int x = 0; x < 8; ++x)
    if (per_xcd[x] > per) return fail("an XCD residue class holds more than ceil(T / 8) items", rows, g, riders, order, x);
  const long long unused_slots = poses_shape_slots(shape) - riders;
  if (empty - unused_slots > 7 || empty - unused_slots < 0) return fail("more than 7 empty evaluation workgroups", rows, g, riders, order, empty);
  return 0;
}

int main() {
  const int rows_sweep[] = {1, 2, 7, 8, 9, 13, 98}, g_sweep[] = {1, 7, 63, 64, 65, 128, 130, 1024}, rider_sweep[] = {0, 1, 7, 8, 9};
  long long cases = 0;
  for (int order = 0; order < 2; ++order)
    for (int xcd = 0; xcd < 2; ++xcd)
      for (int g : g_sweep)
        for (int riders : rider_sweep)
          for (int rows : rows_sweep) {
            // the same rows as one term, and cut raggedly into 2-4 terms (one of them without a chunk)
            std::vector<std::vector<int>> cuts = {{rows}, {rows / 3, rows - rows / 3}, {rows - rows / 2, 0, rows / 2},
                                                  {rows / 4, 0, rows - rows / 4 - rows / 5, rows / 5}};
            for (const auto &chunks : cuts) {
              if (check(chunks, g, riders, order, xcd != 0)) return 1;
              ++cases;
            }
          }
  // launch sizes: G = the bound rounded down to whole groups (left alone below one group); K poses in launches of G, the
  // last takes the remainder -- every launch but the last a multiple of 64 when the bound allows one group
  for (int bound : {1, 7, 63, 64, 65, 100, 127, 128, 1337, 2000, 5000}) {
    const int G = poses_lanes_group_size(bound);
    if (G < 1 || G > bound || (bound >= 64 && G % 64 != 0) || (bound >= 64 && bound - G >= 64) || (bound < 64 && G != bound)) {
      std::printf("FAILED: G %d under bound %d\n", G, bound);
      return 1;
    }
    for (int K = 1; K <= 2100; ++K) {
      const int per = poses_lanes_launch_size(K, G);
      long long covered = 0;
      int launches = 0;
      for (int start = 0; start < K; start += per, ++launches) {
        const int g = K - start < per ? K - start : per;
        if (g < 1 || g > G) { std::printf("FAILED: launch of %d under G %d (K %d)\n", g, G, K); return 1; }
        if (bound >= 64 && start + g < K && g % 64 != 0) { std::printf("FAILED: launch of %d in front of the last (K %d, G %d)\n", g, K, G); return 1; }
        covered += g;
      }
      if (covered != K || launches != (K + G - 1) / G) { std::printf("FAILED: split of K %d under G %d\n", K, G); return 1; }
    }
  }
  std::printf("ok %lld\n", cases);
  return 0;
}
