// The work-list mapping of ea_eval_poses_kernel (edge_alignment_amd/csrc/ea_poses_map.h) swept on the host: a stand-alone
// program (built by tests/test_poses_map_host.py with -fsanitize=address,undefined) that walks every workgroup of a launch in
// dispatch order and checks what the kernel and its launcher rely on.  Exit status 0 and "ok <cases>" on success; the first
// violated property is printed and the status is 1.
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
  if (rows == 0) return 0;  // (the launcher refuses a launch without rows: the host enqueues the fold alone)
  const bool single = nterms == 1;
  const int shape = poses_shape(xcd, order, single, riders);
  const unsigned grid = poses_grid(rows, g, riders);
  const long long T = (long long)rows * g, per = (T + 7) / 8;
  if (poses_shape_slots(shape) % 8 != 0 || poses_shape_slots(shape) < riders || poses_shape_slots(shape) >= riders + 8)
    return fail("rider slots are the rider count rounded up to 8", rows, g, riders, order, poses_shape_slots(shape));
  std::vector<int> seen_rider(riders, 0), per_xcd(8, 0);
  std::vector<int> seen((size_t)T, 0);      // indexed by the partial row pose * rows + row
  std::vector<int> seen_chunk((size_t)T, 0);  // indexed by (pose, term, chunk) through the term's first row
  long long empty = 0, evals = 0;
  bool eval_started = false;
  for (unsigned L = 0; L < grid; ++L) {
    const PosesWork w = poses_work(L, shape, rows, g, riders);
    if (w.kind == 0) { ++empty; continue; }
    if (w.kind == 1) {
      if (eval_started) return fail("a rider behind an evaluation item in dispatch order", rows, g, riders, order, L);
      if (w.rider < 0 || w.rider >= riders) return fail("rider out of range", rows, g, riders, order, L);
      ++seen_rider[w.rider];
      int pose, problem;
      poses_rider(w.rider, count, &pose, &problem);
      if (problem < 0 || problem >= count || pose * count + problem != w.rider) return fail("rider -> (pose, problem)", rows, g, riders, order, L);
      continue;
    }
    eval_started = true;
    ++evals;
    if (w.pose < 0 || w.pose >= g || w.row < 0 || w.row >= rows) return fail("item out of range", rows, g, riders, order, L);
    const PosesChunk c = poses_chunk(w, shape, rows, single ? nullptr : table.data());
    if (c.term < 0 || c.term >= nterms) return fail("term out of range", rows, g, riders, order, L);
    if (c.chunk < 0 || c.chunk >= chunks[c.term]) return fail("chunk outside its term", rows, g, riders, order, L);
    if (c.out_row != w.pose * rows + w.row || c.out_row != w.pose * rows + row0[c.term] + c.chunk)
      return fail("partial row is pose * rows + row", rows, g, riders, order, L);
    if (c.slot != w.pose * count + c.term) return fail("pose slot is pose * count + group", rows, g, riders, order, L);
    ++seen[(size_t)c.out_row];
    ++seen_chunk[(size_t)w.pose * rows + row0[c.term] + c.chunk];
    if (xcd) ++per_xcd[L & 7];
  }
  for (int r = 0; r < riders; ++r) if (seen_rider[r] != 1) return fail("every rider exactly once", rows, g, riders, order, r);
  for (long long t = 0; t < T; ++t)
    if (seen[(size_t)t] != 1 || seen_chunk[(size_t)t] != 1) return fail("every (pose, term, chunk) exactly once", rows, g, riders, order, t);
  if (evals != T) return fail("T evaluation items", rows, g, riders, order, evals);
  for (int x = 0; x < 8; ++x)
    if (per_xcd[x] > per) return fail("an XCD residue class holds more than ceil(T / 8) items", rows, g, riders, order, x);
  // workgroups without work: the unused rider slots (< 8) apart, at most 7
  const long long unused_slots = poses_shape_slots(shape) - riders;
  if (empty - unused_slots > 7 || empty - unused_slots < 0) return fail("more than 7 empty evaluation workgroups", rows, g, riders, order, empty);
  return 0;
}

int main() {
  const int rows_sweep[] = {1, 2, 7, 8, 9, 13, 98, 977}, g_sweep[] = {1, 2, 3, 8, 11, 335}, rider_sweep[] = {0, 1, 7, 8, 9};
  long long cases = 0;
  for (int order = 0; order < 2; ++order)
    for (int xcd = 0; xcd < 2; ++xcd)
      for (int g : g_sweep)
        for (int riders : rider_sweep) {
          for (int rows : rows_sweep) {
            // the same rows as one term, and cut raggedly into 2-4 terms (one of them without a chunk)
            std::vector<std::vector<int>> cuts = {{rows}, {rows / 3, rows - rows / 3}, {rows - rows / 2, 0, rows / 2},
                                                  {rows / 4, 0, rows - rows / 4 - rows / 5, rows / 5}};
            for (const auto &chunks : cuts) {
              if (check(chunks, g, riders, order, xcd != 0)) return 1;
              ++cases;
            }
          }
        }
  // the even split of K poses over launches of at most G
  for (int K = 1; K <= 2100; ++K)
    for (int G : {1, 2, 3, 7, 333, 335, 2000, 5000}) {
      const int per = poses_launch_size(K, G), n = (K + per - 1) / per;
      if (per < 1 || per > G || per > K || n > poses_launches(K, G) || (long long)(n - 1) * per >= K) {
        std::printf("FAILED: split of K %d under G %d: %d launches of %d\n", K, G, n, per);
        return 1;
      }
      if (n > 1 && K - (n - 1) * per < per - n) {  // the remainder is short of a full launch by less than the launch count
        std::printf("FAILED: uneven split of K %d under G %d: last launch %d of %d\n", K, G, K - (n - 1) * per, per);
        return 1;
      }
    }
  std::printf("ok %lld\n", cases);
  return 0;
}
