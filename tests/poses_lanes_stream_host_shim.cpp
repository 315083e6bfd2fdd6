// The coordinate stream of a wavefront of ea_eval_poses_lanes_kernel (edge_alignment_amd/csrc/ea_lanes_stream.h) played on
// the host: a stand-alone program (built by tests/test_poses_lanes_stream_host.py with -fsanitize=address,undefined) that
// walks a sub-run of every length 1 .. 130 the way lanes_run does -- the prologue loads pair 0, iteration k loads pair k + 1
// into the registers iteration k + 1 reads and consumes what the slot in front of it loaded -- out of arrays of exactly n_sub
// doubles, so that a load outside the sub-run is a sanitizer report as well as a failed check.
// Exit status 0 and "ok <sub-runs>" on success; the first violated property is printed, status 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "ea_lanes_stream.h"

using namespace ea;

static int fail(const char *what, int n_sub, int k) {
  std::printf("FAILED: %s (n_sub %d, slot %d)\n", what, n_sub, k);
  return 1;
}

// what the kernel does with a slot: one 16-byte load of two adjacent points, or two 8-byte loads
static int load(const std::vector<double> &p, const LanesStreamLoad &ld, int n_sub, int k, double (&reg)[2]) {
  if (ld.i0 < 0 || ld.i0 >= n_sub || ld.i1 < 0 || ld.i1 >= n_sub) return fail("a loaded index outside [0, n_sub)", n_sub, k);
  if (ld.wide) {
    if (ld.i1 != ld.i0 + 1) return fail("a 16-byte load of points that are not adjacent", n_sub, k);
    std::memcpy(reg, p.data() + ld.i0, 2 * sizeof(double));
  } else {
    reg[0] = p[ld.i0];
    reg[1] = p[ld.i1];
  }
  return 0;
}

static int check(int n_sub) {
  std::vector<double> p(n_sub);  // (exactly the sub-run: the sanitizer sees a read at or beyond n_sub)
  for (int i = 0; i < n_sub; ++i) p[i] = 1000.0 + i;
  const int last = n_sub - 1, iters = lanes_stream_iters(n_sub);
  if (iters != (n_sub + 1) / 2) return fail("iterations", n_sub, iters);
  std::vector<int> taken(n_sub, 0);
  double reg[2];
  if (load(p, lanes_stream_load(-1, n_sub), n_sub, -1, reg)) return 1;
  int next = 0;  // the next point to be consumed
  for (int k = 0; k < iters; ++k) {
    // the pair this iteration consumes: (i, min(i + 1, last)), out of the registers the slot in front of it loaded
    const int i = 2 * k, j = i + 1 < last ? i + 1 : last;
    const LanesStreamLoad pr = lanes_stream_pair(k, n_sub);
    if (pr.i0 != i || pr.i1 != j) return fail("an iteration consumes (i, min(i + 1, last))", n_sub, k);
    if (reg[0] != 1000.0 + i || reg[1] != 1000.0 + j) return fail("the registers hold another pair than the iteration consumes", n_sub, k);
    if (i != next) return fail("points are consumed in order", n_sub, k);
    ++taken[i];
    ++next;
    if (j != i) { ++taken[j]; ++next; }  // (an odd sub-run's last point comes twice and counts once: the copy is not summed)
    // the registers are free once both points are projected: the next pair lands in them
    if (load(p, lanes_stream_load(k, n_sub), n_sub, k, reg)) return 1;
  }
  if (next != n_sub) return fail("every point is consumed", n_sub, next);
  for (int i = 0; i < n_sub; ++i)
    if (taken[i] != 1) return fail("a point consumed more or less than once", n_sub, i);
  return 0;
}

int main() {
  int cases = 0;
  for (int n_sub = 1; n_sub <= 130; ++n_sub) {
    if (check(n_sub)) return 1;
    ++cases;
  }
  std::printf("ok %d\n", cases);
  return 0;
}
