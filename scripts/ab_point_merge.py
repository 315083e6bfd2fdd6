"""What moving and joining point sets costs on the device (ea_batch_transform_points, ea_batch_merge_points) against the
caller's loop they replace, and what carrying points across a keyframe replacement costs the multi-stream tracker per push:
same process, same box, fp64.

Part 1, the calls: 32 problems x 50 000 weighted points on a 640 x 480 grid.  The points are random pixels of the grid
back-projected at random depths, the weights random, the DT image random; the motion is a small rigid one.  Legs, each starting
from the same freshly loaded problems (the reload is not timed):

  loop     the BASELINE: per problem get_points / get_weights read-backs, the numpy restatement of the rule
           (tests/point_merge_ref.py), set_points / set_weights -- what a caller has to do without the call.
  device   ONE ea_batch_transform_points, or ONE ea_batch_merge_points, over the batch.

Sets: `transform`; `copy` (merge, every filter off: a_X2 = T * a_X into problems that hold 50 000 points already) and `carry`
(merge with require_pixel, margin 2, max_dt 1, cell_px 4 nearest, weight_scale 0.5).  Both legs must leave the same point and
weight bits in every problem: checked on every run.  The legs run interleaved, ROUNDS times over; the table gives every run and
each leg's median.

Part 2, the tracker: Canny 640 x 480, 32 streams in keyframe mode, frames in page-locked memory, stream i seeing bundled frame
(i + k) % 5 at push k.  Legs, each a tracker of its own:

  off        the carry is never set: the push of the parent commit (keyframe rule: every rule off, max_frames = 0).
  on_kept    the carry is set, no stream ever replaces its keyframe (the same rule).
  on_taking  the carry is set and every stream replaces its keyframe in every push (max_frames = 1).
  taking     no carry, max_frames = 1: what of on_taking is the replacement itself.

A run is 2 warm-up pushes and 20 timed ones on a fresh tracker; a run's figure is the MEDIAN push.  The legs run interleaved,
three times over.

usage: python scripts/ab_point_merge.py                         > profiles/point_merge_ab.txt
       python scripts/ab_point_merge.py off                     the `off` leg of part 2 alone (it needs nothing of this
                                                                feature: run from the tree of another build for its figure)
       python scripts/ab_point_merge.py trace LEG SET REPS      REPS repetitions of one leg of part 1 (reloads included) and
                                                                nothing else, to be run under rocprofv3 --kernel-trace
                                                                --hip-trace --stats
       python scripts/ab_point_merge.py trace_push LEG PUSHES   PUSHES pushes of one leg of part 2, likewise
       python scripts/ab_point_merge.py counts DIR_A REPS_A DIR_B REPS_B
                                                                the per-repetition difference of two traced runs"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, ".")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

K = (525.0, 525.0, 319.5, 239.5)
H, W = 480, 640
N, POINTS, ROUNDS = 32, 50000, 7
MOTION = np.eye(4)
MOTION[:3, :3] = [[1.0, -0.004, 0.006], [0.004, 1.0, -0.005], [-0.006, 0.005, 1.0]]
MOTION[:3, 3] = (0.02, -0.01, 0.03)
SETS = {"transform": None, "copy": dict(), "carry": dict(require_pixel=1, margin=2, max_dt=1.0, cell_px=4, cell_rule=1, weight_scale=0.5)}
WARM, PUSHES, TRACKER_ROUNDS = 2, 20, 3
TRACKER_LEGS = {"off": (False, 0), "on_kept": (True, 0), "on_taking": (True, 1), "taking": (False, 1)}
CARRY = dict(require_pixel=1, margin=2, cell_px=4, cell_rule=1, weight_scale=0.5)


def make_inputs():
    rng = np.random.default_rng(5)
    out = []
    for _ in range(2 * N):
        u = rng.integers(0, W, POINTS).astype(np.float64)
        v = rng.integers(0, H, POINTS).astype(np.float64)
        z = rng.uniform(0.5, 6.0, POINTS)
        xyz = np.stack([(u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z], axis=1)
        out.append((xyz, rng.uniform(0.0, 1.0, POINTS)))
    dt = rng.integers(0, 4 * 64, (H, W)).astype(np.float64) / 64.0
    return out[:N], out[N:], dt


def reload(problems, inputs):
    for P, (xyz, w) in zip(problems, inputs):
        P.set_points(xyz)
        P.set_weights(w)


def leg_device(B, dst, src, prm, dt):
    if prm is None:
        B.transform_points(np.stack([MOTION] * N))
        return None
    return B.merge_points(src, [MOTION] * N, **prm)


def leg_loop(B, dst, src, prm, dt):
    import point_merge_ref as pm
    stats = []
    for P, S in zip(dst, src):
        xyz, w = P.get_points(), P.get_weights()
        if prm is None:
            P.set_points(pm.transform(xyz, MOTION))
            P.set_weights(w)
            continue
        pts, ww, st, _ = pm.merge(xyz, w, S.get_points(), S.get_weights(), MOTION, K, dt, **prm)
        P.set_points(pts)
        P.set_weights(ww)
        stats.append(st)
    return stats or None


LEGS = {"loop": leg_loop, "device": leg_device}


def state(problems):
    return [(P.get_points().view(np.uint64).copy(), P.get_weights().view(np.uint64).copy()) for P in problems]


def counts(dir_a, reps_a, dir_b, reps_b):
    import csv
    import glob

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
        print("  %s per repetition, from %d and %d repetitions:" % (title, reps_a, reps_b))
        total = 0.0
        for name in sorted(set(a) | set(b)):
            d = (b.get(name, 0) - a.get(name, 0)) / per
            if d != 0:
                print("    %-72s %8.2f" % (name[:72], d))
                total += d
        print("    %-72s %8.2f" % ("(all)", total))
    return 0


# ---- part 2: the tracker ----------------------------------------------------------------------------------------------------------

def tracker_frames(capi, synth):
    frames = synth.load_bundled_frames(os.path.join(ROOT, "tests", "golden", "rgbd"))
    out = []
    for k in range(1, 6):
        pair = []
        for a in frames[k]:
            p = capi.pinned_array(a.shape, a.dtype)
            p[:] = a
            pair.append(p)
        out.append(tuple(pair))
    return out


def pick(frames, k):
    return [frames[(i + k) % 5][0] for i in range(N)], [frames[(i + k) % 5][1] for i in range(N)]


def make_tracker(capi, leg):
    carry, max_frames = TRACKER_LEGS[leg]
    tb = capi.TrackerBatch([K] * N, dtype=capi.EA_F64, flavour=1)
    for i in range(N):
        tb.problem(i).set_loss(capi.LOSS_CAUCHY, 1.0)
    tb.set_keyframes(min_visible_fraction=0.0, min_inlier_fraction=0.0, max_mean_flow=0.0, max_frames=max_frames)
    if carry:
        tb.set_point_carry(**CARRY)
    return tb


def run_tracker(capi, leg, frames, pushes=PUSHES):
    tb = make_tracker(capi, leg)
    times = []
    for k in range(WARM + pushes):
        bgr, depth = pick(frames, k)
        s = time.perf_counter()
        q, t, _, _ = tb.push_frames(bgr, depth)
        if k >= WARM:
            times.append((time.perf_counter() - s) * 1e3)
    info = {key: tb.info(key) for key in ("aligned", "keyframes_taken")}
    if TRACKER_LEGS[leg][0]:
        info["carried"] = tb.info("carried")
        info["points_carried"] = sum(st["carried"] for st in tb.last_point_carry())
    info["points"] = sum(tb.problem(i).num_points for i in range(N))
    tb.close()
    return float(np.median(times)), min(times), max(times), (q, t), info


def tracker_table(capi, synth, legs):
    frames = tracker_frames(capi, synth)
    runs = {leg: [] for leg in legs}
    for _ in range(TRACKER_ROUNDS):
        for leg in legs:
            runs[leg].append(run_tracker(capi, leg, frames))
    print("tracker: %d streams of %d x %d Canny frames in keyframe mode, fp64, %d timed pushes per run after %d warm-up pushes, "
          "%d interleaved runs per leg" % (N, W, H, PUSHES, WARM, TRACKER_ROUNDS))
    med = {}
    for leg in legs:
        med[leg] = float(np.median([r[0] for r in runs[leg]]))
        for r, (m, lo, hi, _, info) in enumerate(runs[leg]):
            print("  %-9s run %d: median push %8.3f ms   (%8.3f .. %8.3f)   %s" % (leg, r + 1, m, lo, hi, info if r == 0 else ""))
        print("  %-9s median of %d runs: %8.3f ms per push; the runs spread by %.3f ms"
              % (leg, TRACKER_ROUNDS, med[leg], max(r[0] for r in runs[leg]) - min(r[0] for r in runs[leg])))
    if len(legs) > 1:
        for a, b in zip(runs["off"][0][3], runs["on_kept"][0][3]):     # a carry that never runs moves no pose
            assert np.array_equal(a, b)
        print("  on_kept - off %+.3f ms, on_taking - taking %+.3f ms (the carry itself), taking - off %+.3f ms (the replacement)"
              % (med["on_kept"] - med["off"], med["on_taking"] - med["taking"], med["taking"] - med["off"]))


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "counts":
        return counts(sys.argv[2], int(sys.argv[3]), sys.argv[4], int(sys.argv[5]))
    import torch  # (first: one HIP runtime in the process)
    if torch.cuda.is_available():
        torch.cuda.init()
    from edge_alignment_amd import capi, synth
    if len(sys.argv) > 1 and sys.argv[1] == "off":
        tracker_table(capi, synth, ("off",))
        return 0
    if len(sys.argv) > 1 and sys.argv[1] == "trace_push":
        leg, pushes = sys.argv[2], int(sys.argv[3])
        tb, frames = make_tracker(capi, leg), tracker_frames(capi, synth)
        for k in range(pushes):
            tb.push_frames(*pick(frames, k))
        print("trace_push: %d pushes of %d streams, leg %s" % (pushes, N, leg))
        tb.close()
        return 0
    dst_in, src_in, dt = make_inputs()
    dst = [capi.Problem(*K, dtype=capi.EA_F64) for _ in range(N)]
    src = [capi.Problem(*K, dtype=capi.EA_F64) for _ in range(N)]
    for P in dst + src:
        P.set_point_order(0)
    for P in dst:
        P.set_dt_grid(np.ascontiguousarray(dt.T))
    reload(src, src_in)
    B = capi.Batch(dst)
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        leg, name, reps = sys.argv[2], sys.argv[3], int(sys.argv[4])
        for _ in range(reps):
            reload(dst, dst_in)
            LEGS[leg](B, dst, src, SETS[name], dt)
        print("trace: %d repetitions of leg %s, set %s" % (reps, leg, name))
        return 0
    print("%d problems x %d weighted points (and as many in every src) on a %d x %d grid, fp64; %d interleaved runs per leg; "
          "ms per batch, host clock" % (N, POINTS, W, H, ROUNDS))
    for name, prm in SETS.items():
        times = {leg: [] for leg in LEGS}
        want = None
        for _ in range(ROUNDS + 1):                            # (the first round warms allocations up and is not reported)
            for leg, fn in LEGS.items():
                reload(dst, dst_in)
                s = time.perf_counter()
                stats = fn(B, dst, src, prm, dt)
                times[leg].append((time.perf_counter() - s) * 1e3)
                got = (stats, state(dst))
                if want is None:
                    want = got
                assert got[0] == want[0], (name, leg)
                for (ax, aw), (bx, bw) in zip(got[1], want[1]):
                    assert np.array_equal(ax, bx) and np.array_equal(aw, bw), (name, leg)
        print("set %s %s: problem 0 %s; both legs leave the same point and weight bits"
              % (name, prm if prm is not None else "", want[0][0] if want[0] else "transformed in place"))
        med = {}
        for leg in LEGS:
            t = times[leg][1:]
            med[leg] = float(np.median(t))
            print("  %-6s %s   median %9.3f ms" % (leg, " ".join("%9.3f" % x for x in t), med[leg]))
        print("  device / loop = %.4f" % (med["device"] / med["loop"]))
    B.close()
    for P in dst + src:
        P.close()
    print()
    tracker_table(capi, synth, tuple(TRACKER_LEGS))
    return 0


if __name__ == "__main__":
    sys.exit(main())
