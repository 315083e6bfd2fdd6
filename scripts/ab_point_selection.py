"""What thinning the points of a batch costs on the device (ea_batch_select_points) against the caller's loop it replaces: same
process, same box, 32 problems x 50 000 weighted points on a 640 x 480 grid, fp64.  The points are random pixels of the grid
back-projected at random depths (several per pixel and per cell), the weights random.

Two legs, each starting from the same freshly loaded problems (the reload is not timed):

  loop     the BASELINE: per problem get_points / get_weights, the numpy restatement of the rule (tests/point_select_ref.py),
           set_points / set_weights -- what a caller has to do without the call, host round trip and re-upload included.
  device   ONE ea_batch_select_points over the batch.

Two parameter sets: `stride30` (the reference's `i += 30`) and `cells` (cell_px 8, EA_CELL_NEAREST, target 2000: one point per
cell, then the reference's iterStep rule).  Both legs must leave the same point and weight bits in every problem: checked on
every run.  A run is one call (or one loop over the batch) between host clocks -- both return synchronised; the legs run
interleaved, ROUNDS times over, and the table gives every run and each leg's median.

usage: python scripts/ab_point_selection.py                       > profiles/point_selection_ab.txt
       python scripts/ab_point_selection.py trace LEG SET REPS    REPS repetitions of one leg (reloads included) and nothing
                                                                  else, to be run under rocprofv3 --kernel-trace --hip-trace
                                                                  --stats: two runs with different REPS give the launches
                                                                  and waits per call as a difference
       python scripts/ab_point_selection.py counts DIR_A REPS_A DIR_B REPS_B
                                                                  that difference, from the two runs' stats files"""
import csv
import glob
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K = (525.0, 525.0, 319.5, 239.5)
H, W = 480, 640
N, POINTS, ROUNDS = 32, 50000, 7
SETS = {"stride30": dict(stride=30), "cells": dict(cell_px=8, cell_rule=1, target=2000)}


def make_inputs():
    rng = np.random.default_rng(5)
    out = []
    for _ in range(N):
        u = rng.integers(0, W, POINTS).astype(np.float64)
        v = rng.integers(0, H, POINTS).astype(np.float64)
        z = rng.uniform(0.5, 6.0, POINTS)
        xyz = np.stack([(u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z], axis=1)
        out.append((xyz, rng.uniform(0.0, 1.0, POINTS)))
    return out


def reload(problems, inputs):
    for P, (xyz, w) in zip(problems, inputs):
        P.set_points(xyz)
        P.set_weights(w)


def leg_device(B, problems, prm):
    return B.select_points(height=H, width=W, **prm)


def leg_loop(B, problems, prm):
    import point_select_ref as ps
    stats = []
    for P in problems:
        xyz, w = P.get_points(), P.get_weights()
        kept, st = ps.select(xyz, K, H, W, **prm)
        P.set_points(xyz[kept])
        P.set_weights(w[kept])
        stats.append(st)
    return stats


LEGS = {"loop": leg_loop, "device": leg_device}


def state(problems):
    return [(P.get_points().view(np.uint64).copy(), P.get_weights().view(np.uint64).copy()) for P in problems]


def counts(dir_a, reps_a, dir_b, reps_b):
    def read(d, pattern):
        rows = {}
        for path in glob.glob(os.path.join(d, "**", pattern), recursive=True):
            with open(path) as f:
                for row in csv.DictReader(f):
                    rows[row["Name"]] = rows.get(row["Name"], 0) + int(row["Calls"])
        return rows
    per = float(reps_b - reps_a)
    for title, pattern in (("kernels", "*kernel_stats.csv"), ("HIP calls", "*hip_api_stats.csv")):
        a, b = read(dir_a, pattern), read(dir_b, pattern)
        print("  %s per repetition (reload included), from %d and %d repetitions:" % (title, reps_a, reps_b))
        total = 0.0
        for name in sorted(set(a) | set(b)):
            d = (b.get(name, 0) - a.get(name, 0)) / per
            if d != 0:
                print("    %-72s %8.2f" % (name[:72], d))
                total += d
        print("    %-72s %8.2f" % ("(all)", total))
    return 0


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "counts":
        return counts(sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    import torch  # (first: one HIP runtime in the process)
    if torch.cuda.is_available():
        torch.cuda.init()
    from edge_alignment_amd import capi
    inputs = make_inputs()
    problems = [capi.Problem(*K, dtype=capi.EA_F64) for _ in range(N)]
    B = capi.Batch(problems)
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        leg, name, reps = sys.argv[2], sys.argv[3], int(sys.argv[4])
        for _ in range(reps):
            reload(problems, inputs)
            LEGS[leg](B, problems, SETS[name])
        print("trace: %d repetitions of leg %s, set %s" % (reps, leg, name))
        return 0
    print("%d problems x %d weighted points on a %d x %d grid, fp64; %d interleaved runs per leg; ms per batch, host clock"
          % (N, POINTS, W, H, ROUNDS))
    for name, prm in SETS.items():
        times = {leg: [] for leg in LEGS}
        want = None
        for _ in range(ROUNDS + 1):                            # (the first round warms allocations up and is not reported)
            for leg, fn in LEGS.items():
                reload(problems, inputs)
                s = time.perf_counter()
                stats = fn(B, problems, prm)
                times[leg].append((time.perf_counter() - s) * 1e3)
                got = (stats, state(problems))
                if want is None:
                    want = got
                assert got[0] == want[0], (name, leg)
                for (ax, aw), (bx, bw) in zip(got[1], want[1]):
                    assert np.array_equal(ax, bx) and np.array_equal(aw, bw), (name, leg)
        print("set %s %s: %d -> %d points in problem 0 (stride_used %d); both legs leave the same point and weight bits"
              % (name, prm, want[0][0]["n_before"], want[0][0]["n_after"], want[0][0]["stride_used"]))
        med = {}
        for leg in LEGS:
            t = times[leg][1:]
            med[leg] = float(np.median(t))
            print("  %-6s %s   median %9.3f ms" % (leg, " ".join("%9.3f" % x for x in t), med[leg]))
        print("  device / loop = %.4f" % (med["device"] / med["loop"]))
    B.close()
    for P in problems:
        P.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
