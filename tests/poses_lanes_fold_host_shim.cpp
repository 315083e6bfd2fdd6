// The fold inside the launches of ea_eval_poses_lanes_kernel (edge_alignment_amd/csrc/ea_poses_map.h, "the rows of the lanes
// path") swept on the host: a stand-alone program (built by tests/test_poses_lanes_fold_host.py with
// -fsanitize=address,undefined) that plays every launch of a call the way the kernel does -- every item stores its row and
// takes its level-1 ticket, every completed run stores its partial and takes its level-2 ticket -- into arrays of exactly the
// sizes the host allocates.  Exit status 0 and "ok <cases>" on success; the first violated property is printed, status 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "ea_poses_map.h"

using namespace ea;

static int fail(const char *what, int rows, int K, int G, int order, long long at) {
  std::printf("FAILED: %s (rows %d, K %d, G %d, order %d, at %lld)\n", what, rows, K, G, order, at);
  return 1;
}

// one call: problems of nrows[i] rows each, K poses in launches of G (the last takes the remainder)
static int check(const std::vector<int> &nrows, int K, int G, int order, bool xcd) {
  const int count = (int)nrows.size();
  int rows = 0;
  std::vector<PosesRow> table;
  std::vector<int> row0(count + 1, 0);
  for (int i = 0; i < count; ++i) {
    for (int c = 0; c < nrows[i]; ++c) table.push_back(PosesRow{i, rows, count, 0});
    rows += nrows[i];
    row0[i + 1] = rows;
  }
  if (rows == 0) return 0;  // (the host enqueues no lanes launch for a batch without a point)
  const bool single = count == 1;
  const int shape = poses_shape(xcd, order, single, 0);
  // what the host allocates: rows, partials and counters for a launch of G poses, flags for the call of K
  const int groups_cap = poses_lanes_groups(G), slots = poses_lanes_run_slots(rows, count);
  std::vector<char> row_words((size_t)groups_cap * rows * kPosesLanesBlock, 0);
  std::vector<char> part_words((size_t)groups_cap * slots * kPosesLanesBlock, 0);
  std::vector<int> flags((size_t)poses_lanes_call_groups(K, G) * count, 0);
  int group0 = 0;
  for (int start = 0; start < K; start += poses_lanes_launch_size(K, G)) {
    const int g = std::min(poses_lanes_launch_size(K, G), K - start), groups = poses_lanes_groups(g);
    if (groups > groups_cap) return fail("a launch has more groups than the arrays hold", rows, K, G, order, groups);
    const size_t ncounters = poses_lanes_counters(groups, rows, count);
    if (ncounters % 4 != 0 || ncounters > poses_lanes_counters(groups_cap, rows, count)) return fail("counter block size", rows, K, G, order, (long long)ncounters);
    std::vector<unsigned> counters(ncounters, 0);  // (zeroed ahead of the launch)
    std::fill(row_words.begin(), row_words.end(), 0);
    std::fill(part_words.begin(), part_words.end(), 0);
    std::vector<int> slot_owner((size_t)groups * slots, -1);  // (problem, run) that uses a run slot
    const unsigned grid = poses_lanes_grid(rows, g, 0);
    long long items = 0;
    for (unsigned L = 0; L < grid; ++L) {
      const PosesLanesWork w = poses_lanes_work(L, shape, rows, g, 0);
      if (w.kind == 0) continue;
      if (w.kind != 2) return fail("a launch without riders has a rider", rows, K, G, order, L);
      ++items;
      const PosesLanesChunk pc = poses_lanes_chunk(w.row, shape, table.data());
      const int group = w.pose0 / kPosesLanes, problem = pc.term, n = nrows[problem], r0 = w.row - pc.chunk;
      if (r0 != row0[problem] || pc.chunk < 0 || pc.chunk >= n) return fail("item -> (problem, chunk)", rows, K, G, order, L);
      // the row
      const size_t ro = poses_lanes_row_off(group, w.row, rows);
      if (ro + kPosesLanesBlock > row_words.size()) return fail("row outside the row array", rows, K, G, order, L);
      if (row_words[ro]++) return fail("a row stored twice", rows, K, G, order, L);
      // its run: every row in exactly one run, runs of kPosesRun except the last
      const int run = poses_lanes_run(pc.chunk), nruns = poses_lanes_runs(n), in_run = poses_lanes_run_rows(n, run);
      if (run < 0 || run >= nruns) return fail("run of a row out of range", rows, K, G, order, L);
      if (in_run != (run + 1 < nruns ? kPosesRun : n - (nruns - 1) * kPosesRun) || in_run < 1 || in_run > kPosesRun)
        return fail("runs have kPosesRun rows except the last", rows, K, G, order, L);
      if (pc.chunk < run * kPosesRun || pc.chunk >= run * kPosesRun + in_run) return fail("a row outside its run", rows, K, G, order, L);
      // level-1 ticket
      const int slot = poses_lanes_run_slot(r0, problem, run);
      if (slot < 0 || slot >= slots) return fail("run slot out of range", rows, K, G, order, L);
      int &owner = slot_owner[(size_t)group * slots + slot];
      if (owner >= 0 && owner != problem * 65536 + run) return fail("two runs share a run slot", rows, K, G, order, L);
      owner = problem * 65536 + run;
      const size_t c1 = poses_lanes_counter1(group, slot, rows, count);
      if (c1 >= (size_t)groups * slots || c1 >= ncounters) return fail("level-1 counter outside its block", rows, K, G, order, L);
      if (++counters[c1] > (unsigned)in_run) return fail("more level-1 arrivals than the target", rows, K, G, order, L);
      if (counters[c1] != (unsigned)in_run) continue;
      // the run's last arrival: reads the run's rows, writes the partial, takes the level-2 ticket
      for (int c = run * kPosesRun; c < run * kPosesRun + in_run; ++c)
        if (!row_words[poses_lanes_row_off(group, r0 + c, rows)]) return fail("a run summed before all its rows arrived", rows, K, G, order, L);
      if (poses_lanes_row_off(group, r0 + run * kPosesRun, rows) + (size_t)in_run * kPosesLanesBlock > row_words.size())
        return fail("a run read past the row array", rows, K, G, order, L);
      const size_t po = poses_lanes_partial_off(group, slot, rows, count);
      if (po + kPosesLanesBlock > part_words.size()) return fail("partial outside the partial array", rows, K, G, order, L);
      if (part_words[po]++) return fail("a partial stored twice", rows, K, G, order, L);
      const size_t c2 = poses_lanes_counter2(groups, group, problem, rows, count);
      if (c2 < (size_t)groups * slots || c2 >= (size_t)groups * (slots + count) || c2 >= ncounters) return fail("level-2 counter outside its block", rows, K, G, order, L);
      if (++counters[c2] > (unsigned)nruns) return fail("more level-2 arrivals than the target", rows, K, G, order, L);
      if (counters[c2] != (unsigned)nruns) continue;
      // the problem's last arrival: the partials lie one behind the other from run 0 on, then the flag
      for (int r = 0; r < nruns; ++r) {
        const size_t pr = poses_lanes_partial_off(group, poses_lanes_run_slot(r0, problem, 0), rows, count) + (size_t)r * kPosesLanesBlock;
        if (pr != poses_lanes_partial_off(group, poses_lanes_run_slot(r0, problem, r), rows, count)) return fail("run partials are not consecutive", rows, K, G, order, L);
        if (pr + kPosesLanesBlock > part_words.size() || !part_words[pr]) return fail("a partial read before it was stored", rows, K, G, order, L);
      }
      const size_t f = poses_lanes_flag(group0 + group, problem, count);
      if (f >= flags.size()) return fail("flag outside the flag array", rows, K, G, order, L);
      if (flags[f]++) return fail("a flag raised twice", rows, K, G, order, L);
    }
    if (items != (long long)rows * groups) return fail("items of a launch", rows, K, G, order, items);
    // ticket targets equal the counts that arrived
    for (int group = 0; group < groups; ++group)
      for (int i = 0; i < count; ++i) {
        if (counters[poses_lanes_counter2(groups, group, i, rows, count)] != (unsigned)poses_lanes_runs(nrows[i]))
          return fail("level-2 arrivals differ from the target", rows, K, G, order, group);
        for (int r = 0; r < poses_lanes_runs(nrows[i]); ++r)
          if (counters[poses_lanes_counter1(group, poses_lanes_run_slot(row0[i], i, r), rows, count)] != (unsigned)poses_lanes_run_rows(nrows[i], r))
            return fail("level-1 arrivals differ from the target", rows, K, G, order, group);
      }
    group0 += groups;
  }
  if (group0 != poses_lanes_call_groups(K, G)) return fail("groups of the call", rows, K, G, order, group0);
  // flags: one per (group of the call, problem with rows), none for a problem without
  for (int cg = 0; cg < group0; ++cg)
    for (int i = 0; i < count; ++i)
      if (flags[poses_lanes_flag(cg, i, count)] != (nrows[i] > 0 ? 1 : 0)) return fail("one flag per (group, problem)", rows, K, G, order, cg);
  return 0;
}

int main() {
  std::vector<int> firsts;
  for (int n = 1; n <= 40; ++n) firsts.push_back(n);
  firsts.push_back(98);
  const int Ks[] = {1, 63, 64, 65, 130, 2000};
  long long cases = 0;
  for (int n : firsts)
    for (int nprob = 1; nprob <= 4; ++nprob) {
      // ragged company: a short problem, one without a point, one across a run boundary
      const int others[3] = {1, 0, kPosesRun + 1 + n % 3};
      std::vector<int> nrows(1, n);
      for (int i = 1; i < nprob; ++i) nrows.push_back(others[i - 1]);
      if (nprob == 3) std::swap(nrows[0], nrows[2]);  // (the swept problem not always first: its row0 is not 0)
      for (int K : Ks)
        for (int G : {K, 64, 7}) {
          if (G > K || (K == 2000 && G == 7)) continue;
          for (int order = 0; order < 2; ++order) {
            if (check(nrows, K, poses_lanes_group_size(G) < K ? poses_lanes_group_size(G) : K, order, true)) return 1;
            ++cases;
          }
        }
    }
  // without the XCD deal
  if (check({98}, 2000, 2000, 1, false) || check({17, 0, 33}, 130, 64, 0, false)) return 1;
  cases += 2;
  std::printf("ok %lld\n", cases);
  return 0;
}
