"""What a push of the multi-stream tracker costs in keyframe mode against frame to frame: same process, same box, 32 streams of
640 x 480 frames (the bundled grabs, page-locked), fp64, Canny flavour.  Three kinds of push:

  frame to frame    no keyframe mode: every push scatters every stream's reference (the behaviour before the mode existed)
  nothing replaced  keyframe mode with every rule off: after the first push no stream replaces -- no count fetch, no table
                    upload, no scatter, no depth-weight launch; one ea_batch_pose_stats (2 launches, 1 wait) per solved group
  all replaced      keyframe mode with max_frames = 1: every solved stream replaces -- the frame-to-frame reference stage plus
                    the statistics

on two sequences: `still` (stream i sees bundled frame i % 5 in every push: the solves start at their optimum in all three
kinds, so the difference is the reference stage and the statistics) and `cycling` (stream i sees frame (i + k) % 5 at push k:
a held keyframe is up to four frames away from the current one, so its solves run longer than frame-to-frame ones).

A run is 2 warm-up pushes (the first aligns nothing) and 12 timed ones on a fresh tracker; its figure is the MEDIAN push; every
kind runs twice, interleaved.  Every push ends synchronised, so a time is a host clock around the call.  The launch counts of
the reference stage are read off csrc/ea_frames.hip (tracker_batch_push), not measured.  Nothing is asserted but that the
repeats of a leg agree exactly and that the kinds replace what they say.

usage: python scripts/ab_tracker_keyframes.py > profiles/tracker_keyframes_ab.txt"""
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
N, WARM, TIMED = 32, 2, 12
OFF = dict(min_visible_fraction=0.0, min_inlier_fraction=0.0, inlier_residual=0.05, max_mean_flow=0.0, max_frames=0, margin=0)
KINDS = (("frame to frame", None), ("nothing replaced", OFF), ("all replaced", dict(OFF, max_frames=1)))
# reference stage of one push, from tracker_batch_push: (count + scan launch, count fetch, table upload, scatter launch,
# depth-weight launch [only with depth weighting: none here], statistics launches per solved group, statistics waits)
STAGE = {"frame to frame": (1, 1, 1, 1, 0, 0, 0), "nothing replaced": (1, 0, 0, 0, 0, 2, 1), "all replaced": (1, 1, 1, 1, 0, 2, 1)}


def pinned(a):
    out = capi.pinned_array(a.shape, a.dtype)
    out[:] = a
    return out


def run(frames, params, cycling):
    tb = capi.TrackerBatch([K] * N, dtype=capi.EA_F64, flavour=1, loss=(capi.LOSS_CAUCHY, 1.0))
    if params is not None:
        tb.set_keyframes(**params)
    times, poses, taken, iters = [], [], [], []
    for k in range(WARM + TIMED):
        pick = [(i + (k if cycling else 0)) % 5 for i in range(N)]
        bgr, depth = [frames[j][0] for j in pick], [frames[j][1] for j in pick]
        s = time.perf_counter()
        q, t, sums, aligned = tb.push_frames(bgr, depth)
        if k >= WARM:
            times.append((time.perf_counter() - s) * 1e3)
            iters.append(int(np.sum([x["num_iterations"] for x in sums if x is not None])))
        poses.append((q, t))
        taken.append(tb.info("keyframes_taken"))
    tb.close()
    return float(np.median(times)), min(times), max(times), poses, taken, float(np.mean(iters))


def main():
    raw = synth.load_bundled_frames(os.path.join(ROOT, "tests", "golden", "rgbd"))
    frames = [(pinned(raw[k][0]), pinned(raw[k][1])) for k in range(1, 6)]
    print("%d streams of 640 x 480 frames, fp64, Canny flavour, %d timed pushes per run after %d warm-up pushes" % (N, TIMED, WARM))
    print("reference stage per push (count+scan launch, count fetch, table upload, scatter launch, depth-weight launch,"
          " statistics launches per solved group, statistics waits):")
    for name, _ in KINDS:
        print("  %-17s %s" % (name, STAGE[name]))
    for cycling in (False, True):
        print("sequence: %s" % ("cycling" if cycling else "still"))
        runs = {name: [] for name, _ in KINDS}
        for _ in range(2):
            for name, params in KINDS:
                runs[name].append(run(frames, params, cycling))
        for name, params in KINDS:
            a, b = runs[name]
            for (qa, ta), (qb, tb_) in zip(a[3], b[3]):
                assert np.array_equal(qa, qb) and np.array_equal(ta, tb_), name
            want = [0] * (WARM + TIMED) if params is None else [N] + ([0] if params["max_frames"] == 0 else [N]) * (WARM + TIMED - 1)
            assert a[4] == want, (name, a[4])
            for r, (med, lo, hi, _, _, it) in enumerate(runs[name]):
                print("  %-17s run %d: median push %8.3f ms   (%8.3f .. %8.3f)   per stream %7.4f ms   solver iterations per push %6.1f"
                      % (name, r + 1, med, lo, hi, med / N, it))
        f2f = min(r[0] for r in runs["frame to frame"])
        for name in ("nothing replaced", "all replaced"):
            slow = max(r[0] for r in runs[name])
            print("  %s, slower run, against frame to frame, faster run: %.3f against %.3f ms (%+.3f ms, x %.3f)"
                  % (name, slow, f2f, slow - f2f, slow / f2f))
    return 0


if __name__ == "__main__":
    sys.exit(main())
