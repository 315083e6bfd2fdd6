// The live-list mapping of a multi-start solve (edge_alignment_amd/csrc/ea_starts_map.h) swept on the host: for a live list
// of `live` starts out of K, walked in pieces sized from a STALE (too large) length as the host does, every (position < live,
// row) must be evaluated exactly once at its own start's pose slot into the partial row its step workgroup folds, every
// (position < live, problem) stepped exactly once, nothing taken at or beyond `live`; the compaction of the list (256 lanes,
// a round per 256 positions) must keep the survivors in order; the posted word must round-trip under its tag only.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ea_starts_map.h"

using namespace ea;

static long long checks = 0;
#define REQUIRE(c)                                                                   \
  do {                                                                               \
    ++checks;                                                                        \
    if (!(c)) { std::printf("FAILED %s line %d\n", #c, __LINE__); std::exit(1); }    \
  } while (0)

// the row table of `count` one-term problems with ragged chunk counts that add up to `rows` (fewer rows than problems: the
// first problems have no points)
static std::vector<PosesRow> row_table(int rows, int count) {
  std::vector<int> n((size_t)count, rows / count);
  n[(size_t)count - 1] = rows - (rows / count) * (count - 1);
  if (count > 1 && rows / count > 1) { ++n[0]; --n[1]; }
  std::vector<PosesRow> tab((size_t)rows);
  int r = 0;
  for (int j = 0; j < count; ++j) {
    for (int k = 0; k < n[(size_t)j]; ++k) tab[(size_t)(r + k)] = PosesRow{j, r, count, 0};
    r += n[(size_t)j];
  }
  return tab;
}

static void sweep(int rows, int count, int K, int live, int stale, int G, int order) {
  // the live list: `live` ascending starts out of K (every other one first, then the tail)
  std::vector<int> list;
  for (int k = 0; k < K && (int)list.size() < live; k += 2) list.push_back(k);
  for (int k = 1; k < K && (int)list.size() < live; k += 2) list.push_back(k);
  REQUIRE((int)list.size() == live);
  list.resize((size_t)K, -1);  // (what lies behind n_live is never a start)
  const std::vector<PosesRow> tab = row_table(rows, count);
  const bool single = count == 1;
  std::vector<int> evaluated((size_t)K * rows, 0), stepped((size_t)K * count, 0);
  const int per = starts_piece(stale, G);
  REQUIRE(starts_pairs(stale, G) == (stale + per - 1) / per && per <= G);
  for (int off = 0; off < stale; off += per) {
    const int g = per < stale - off ? per : stale - off;
    const int shape = poses_shape(true, order, single, 0);
    std::vector<int> row_of((size_t)g * rows, -1);  // partial row -> start that wrote it
    for (unsigned L = 0; L < poses_grid(rows, g, 0); ++L) {
      const PosesWork w = poses_work(L, shape, rows, g, 0);
      if (w.kind != 2) { REQUIRE(w.kind == 0); continue; }
      REQUIRE(w.pose < g && w.row < rows);
      if (!starts_position_live(off, w.pose, live)) { REQUIRE(off + w.pose >= live); continue; }
      REQUIRE(off + w.pose < K);
      const int start = list[(size_t)(off + w.pose)];
      REQUIRE(start >= 0);
      const PosesChunk c = starts_chunk(w, start, shape, rows, tab.data());
      REQUIRE(c.term == tab[(size_t)w.row].term && c.chunk == w.row - tab[(size_t)w.row].row0);
      REQUIRE(c.slot == start * count + c.term && c.out_row == w.pose * rows + w.row);
      REQUIRE(row_of[(size_t)c.out_row] == -1);
      row_of[(size_t)c.out_row] = start;
      ++evaluated[(size_t)start * rows + w.row];
    }
    for (unsigned blk = 0; blk < starts_step_grid(g, count); ++blk) {
      int pose, problem;
      starts_step_item(blk, count, &pose, &problem);
      REQUIRE(pose < g && problem < count);
      if (!starts_position_live(off, pose, live)) continue;
      const int start = list[(size_t)(off + pose)];
      ++stepped[(size_t)start * count + problem];
      // the rows this workgroup folds are those its own start's evaluation wrote
      for (int r = 0; r < rows; ++r)
        if (tab[(size_t)r].term == problem) REQUIRE(row_of[(size_t)(pose * rows + r)] == start);
    }
  }
  std::vector<char> is_live((size_t)K, 0);
  for (int i = 0; i < live; ++i) is_live[(size_t)list[(size_t)i]] = 1;
  for (int k = 0; k < K; ++k) {
    for (int r = 0; r < rows; ++r) REQUIRE(evaluated[(size_t)k * rows + r] == (is_live[(size_t)k] ? 1 : 0));
    for (int i = 0; i < count; ++i) REQUIRE(stepped[(size_t)k * count + i] == (is_live[(size_t)k] ? 1 : 0));
  }
}

// the compaction as the step kernel's last workgroup runs it: 256 lanes, a round per 256 positions
static void compaction(int n, unsigned seed) {
  std::vector<int> in((size_t)n), keep((size_t)n), want;
  for (int i = 0; i < n; ++i) {
    in[(size_t)i] = 3 * i + 1;
    seed = seed * 1664525u + 1013904223u;
    keep[(size_t)i] = (int)((seed >> 16) % 3 != 0);
    if (keep[(size_t)i]) want.push_back(in[(size_t)i]);
  }
  std::vector<int> out((size_t)n + 1, -1);
  int kept = 0;
  for (int first = 0; first < n; first += 256) {
    uint64_t masks[4] = {0, 0, 0, 0};
    for (int tid = 0; tid < 256; ++tid)
      if (first + tid < n && keep[(size_t)(first + tid)]) masks[tid >> 6] |= (uint64_t)1 << (tid & 63);
    for (int tid = 0; tid < 256; ++tid)
      if (first + tid < n && keep[(size_t)(first + tid)]) {
        const int slot = starts_compact_slot(masks, tid >> 6, tid & 63, kept);
        REQUIRE(slot >= 0 && slot < n && out[(size_t)slot] == -1);
        out[(size_t)slot] = in[(size_t)(first + tid)];
      }
    kept += starts_compact_kept(masks);
  }
  REQUIRE(kept == (int)want.size());
  for (int i = 0; i < kept; ++i) REQUIRE(out[(size_t)i] == want[(size_t)i]);
  REQUIRE(out[(size_t)kept] == -1);
}

int main() {
  long long cases = 0;
  const int rows_list[] = {1, 7, 98}, count_list[] = {1, 3}, live_list[] = {0, 1, 8, 9};
  for (int rows : rows_list)
    for (int count : count_list) {
      for (int live : live_list)
        for (int K : {9, 12})
          for (int stale : {live, live + 1, K})
            for (int G : {1, 3, 4, 16})
              for (int order = 0; order < 2; ++order) {
                if (stale < 1 || stale > K || stale < live) continue;
                sweep(rows, count, K, live, stale, G, order);
                ++cases;
              }
    }
  for (int n : {0, 1, 63, 64, 65, 255, 256, 257, 1000, 16384})
    for (unsigned seed = 1; seed <= 3; ++seed) { compaction(n, seed); ++cases; }
  // the posted word: fields round-trip at their extremes, another call's tag is not taken for this one's
  for (unsigned tag : {1u, 2u, 0x1ffffu})
    for (unsigned it : {1u, 52u, 0x7fffffffu, 0xffffffffu})
      for (int nl : {0, 1, 9, kMaxStartSlots}) {
        int i2 = -1, n2 = -1;
        const uint64_t w = starts_word(tag, it, nl);
        REQUIRE(starts_word_read(w, tag, &i2, &n2) && (unsigned)i2 == it && n2 == nl);
        REQUIRE(!starts_word_read(w, tag == 1u ? 2u : tag - 1u, &i2, &n2));
        REQUIRE(!starts_word_read(0, tag, &i2, &n2));
        ++cases;
      }
  std::printf("ok %lld cases %lld checks\n", cases, checks);
  return 0;
}
