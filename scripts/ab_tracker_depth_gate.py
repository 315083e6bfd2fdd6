"""What the depth gate inside the multi-stream tracker costs per push (ea_tracker_batch_set_depth_gate): same process, same box,
32 streams, fp64, frames in ea_host_alloc memory (capi.pinned_array), stream i seeing bundled frame (i + k) % 5 at push k.
Three cases:

  canny    flavour 1 at 640 x 480, uint16 depth (the gate reads it at s = 0).
  ros_l1   flavour 2 with halvings = 1 from 1280 x 960 frames (the bundled frames enlarged by pixel repetition, depth = uint16 /
           5000 as float32), one level: the gate reads the full-size depth at s = 1.
  ros_l3   the same frames, three pyramid levels (640 x 480, 320 x 240, 160 x 120): s = 1, 2, 3.

Four legs per case, each a tracker of its own:

  never    the gate is never set: the push of the parent commit.
  count    set_depth_gate(apply = 0): counts only.
  apply    set_depth_gate(apply = 1): the gated weights replace every stream's weights before each solve, so every stream
           runs the weighted kernels.
  dw       no gate, but depth weighting on in every stream (z_ref 1, power 1): the weighted kernels without the gate -- what
           of `apply`'s cost is the kernel family and not the gate.

Every timed push ends synchronised (a push returns with its poses), so a time is a host clock around the push.  A run is 2
warm-up pushes (the first aligns nothing) and 20 timed ones on a fresh tracker; a run's figure is the MEDIAN push.  The legs
run interleaved, never count apply dw, three times over; the table gives every run and the median of a leg's three runs.

usage: python scripts/ab_tracker_depth_gate.py                      > profiles/tracker_depth_gate_ab.txt
       python scripts/ab_tracker_depth_gate.py never                the `never` leg alone (it needs nothing of the gate: run
                                                                    from the tree of another build for its figure)
       python scripts/ab_tracker_depth_gate.py trace CASE LEG PUSHES   PUSHES pushes of one leg and nothing else that launches
                                                                    a kernel, to be run under rocprofv3 --kernel-trace
                                                                    --hip-trace --stats: two runs with different PUSHES give
                                                                    the launches and waits per push as a difference"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402  (first: one HIP runtime in the process)

if torch.cuda.is_available():
    torch.cuda.init()
from edge_alignment_amd import capi, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (525.0, 525.0, 319.5, 239.5)
N, WARM, PUSHES, ROUNDS = 32, 2, 20, 3
CASES = {"canny": (1, 0, 1), "ros_l1": (2, 1, 1), "ros_l3": (2, 1, 3)}   # flavour, halvings, levels
LEGS = ("never", "count", "apply", "dw")
STAT_KEYS = ("n", "n_behind", "n_outside", "n_unknown", "n_consistent", "n_occluded", "n_free")


def pinned(a):
    out = capi.pinned_array(a.shape, a.dtype)
    out[:] = a
    return out


def load(case):
    """the five bundled frames as the case takes them, page-locked -> [(bgr, depth)]"""
    frames = synth.load_bundled_frames(os.path.join(ROOT, "tests", "golden", "rgbd"))
    out = []
    for k in range(1, 6):
        bgr, dep = frames[k]
        if CASES[case][0] == 2:
            bgr = np.repeat(np.repeat(bgr, 2, axis=0), 2, axis=1)
            dep = np.repeat(np.repeat(dep.astype(np.float32) / np.float32(5000.0), 2, axis=0), 2, axis=1)
        out.append((pinned(np.ascontiguousarray(bgr)), pinned(np.ascontiguousarray(dep))))
    return out


def pick(frames, k):
    return [frames[(i + k) % 5][0] for i in range(N)], [frames[(i + k) % 5][1] for i in range(N)]


def make(case, leg):
    flavour, halvings, levels = CASES[case]
    if levels == 1:
        cams = [K] * N
    else:
        cams = [[tuple(v / (1 << l) for v in K)] * N for l in range(levels)]
    tb = capi.TrackerBatch(cams, dtype=capi.EA_F64, flavour=flavour, halvings=halvings, levels=levels)
    for l in range(levels):
        for i in range(N):
            P = tb.level_problem(l, i)
            P.set_loss(capi.LOSS_CAUCHY, 1.0)
            if leg == "dw":
                P.set_depth_weighting(1.0, 1)
    if leg in ("count", "apply"):
        tb.set_depth_gate(apply=int(leg == "apply"))
    return tb


def run(case, leg, frames, pushes=PUSHES):
    tb = make(case, leg)
    levels = CASES[case][2]
    times = []
    for k in range(WARM + pushes):
        bgr, depth = pick(frames, k)
        s = time.perf_counter()
        q, t, _, _ = tb.push_frames(bgr, depth)
        if k >= WARM:
            times.append((time.perf_counter() - s) * 1e3)
    info = {key: tb.info(key) for key in ("aligned",)}
    if leg in ("count", "apply"):
        info["gated"] = tb.info("gated")
        total = {key: 0 for key in STAT_KEYS}
        for l in range(levels):
            for i in range(N):
                st = tb.last_depth_gate(i, level=l)
                for key in STAT_KEYS:
                    total[key] += st[key]
        info["last_push_counts"] = total
    tb.close()
    return float(np.median(times)), min(times), max(times), (q, t), info


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        case, leg, pushes = sys.argv[2], sys.argv[3], int(sys.argv[4])
        tb = make(case, leg)
        frames = load(case)
        for k in range(pushes):
            tb.push_frames(*pick(frames, k))
        print("trace: %d pushes of %d streams, case %s, leg %s" % (pushes, N, case, leg))
        tb.close()
        return 0
    legs = ("never",) if len(sys.argv) > 1 and sys.argv[1] == "never" else LEGS
    for case in CASES:
        frames = load(case)
        runs = {leg: [] for leg in legs}
        for _ in range(ROUNDS):
            for leg in legs:
                runs[leg].append(run(case, leg, frames))
        H, W = frames[0][1].shape
        print("case %s: %d streams of %d x %d frames, fp64, %d timed pushes per run after %d warm-up pushes, %d interleaved runs per leg"
              % (case, N, W, H, PUSHES, WARM, ROUNDS))
        med = {}
        for leg in legs:
            med[leg] = float(np.median([r[0] for r in runs[leg]]))
            for r, (m, lo, hi, _, info) in enumerate(runs[leg]):
                print("  %-5s run %d: median push %8.3f ms   (%8.3f .. %8.3f)   %s" % (leg, r + 1, m, lo, hi, info if r == 0 else ""))
            print("  %-5s median of %d runs: %8.3f ms per push, %7.4f ms per stream" % (leg, ROUNDS, med[leg], med[leg] / N))
        if len(legs) > 1:
            # (apply = 0 must not move a pose; the repeats of a leg agree exactly)
            for a, b in zip(runs["never"][0][3], runs["count"][0][3]):
                assert np.array_equal(a, b), case
            print("  count - never %+.3f ms, apply - never %+.3f ms, dw - never %+.3f ms (the weighted kernels alone), apply - dw %+.3f ms"
                  % (med["count"] - med["never"], med["apply"] - med["never"], med["dw"] - med["never"], med["apply"] - med["dw"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
