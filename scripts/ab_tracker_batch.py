"""What tracking 32 VGA streams costs per push, ea_tracker_batch_push_frames against the per-stream loops that existed before
it: same process, same box, fp64, frames in ea_host_alloc memory (capi.pinned_array), stream i seeing bundled frame
(i + k) % 5 at push k.  Two cases:

  canny   flavour 1 at 640 x 480.  Baseline: a loop of 32 capi.Tracker.push_frame (ea_tracker_push_frame).
  ros     flavour 2 with halvings = 1 from 1280 x 960 frames (the bundled frames enlarged by pixel repetition, depth = uint16 /
          5000 as float32), cameras of the 640 x 480 working extent.  Baseline: per problem set_now_frame_ros(halvings = 1),
          solve from the prior, set_ref_frame_ros(halvings = 1) -- the manual loop of tests/test_gpu_tracker_batch.py.

Every timed push ends synchronised (a push returns with its poses), so a time is a host clock around the push.  A run is 2
warm-up pushes (the first aligns nothing) and 20 timed ones on fresh trackers; a run's figure is the MEDIAN push.  Each case
runs loop, batch, loop, batch; the batched push passes when the slower of its two runs is below the faster of the loop's two:
no margin beyond the spread between the interleaved repeats.  The largest difference between the two legs' poses is reported.

usage: python scripts/ab_tracker_batch.py                       > profiles/tracker_batch_ab.txt
       python scripts/ab_tracker_batch.py trace canny|ros batch|loop   11 pushes (the first aligns nothing) of one leg and
                                              nothing else that launches a kernel, to be run under a kernel tracer"""
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
N, WARM, PUSHES = 32, 2, 20


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
        if case == "ros":
            bgr = np.repeat(np.repeat(bgr, 2, axis=0), 2, axis=1)
            dep = np.repeat(np.repeat(dep.astype(np.float32) / np.float32(5000.0), 2, axis=0), 2, axis=1)
        out.append((pinned(np.ascontiguousarray(bgr)), pinned(np.ascontiguousarray(dep))))
    return out


def pick(frames, k):
    return [frames[(i + k) % 5][0] for i in range(N)], [frames[(i + k) % 5][1] for i in range(N)]


class BatchLeg:
    def __init__(self, case):
        self.tb = capi.TrackerBatch([K] * N, dtype=capi.EA_F64, flavour=1 if case == "canny" else 2, halvings=int(case == "ros"),
                                    loss=(capi.LOSS_CAUCHY, 1.0))

    def push(self, bgr, depth):
        q, t, _, _ = self.tb.push_frames(bgr, depth)
        return q, t

    def close(self):
        self.tb.close()


class CannyLoop:
    def __init__(self, case):
        self.tr = [capi.Tracker(*K, dtype=capi.EA_F64, flavour=1, loss=(capi.LOSS_CAUCHY, 1.0)) for _ in range(N)]

    def push(self, bgr, depth):
        out = [T.push_frame(b, d) for T, b, d in zip(self.tr, bgr, depth)]
        return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])

    def close(self):
        for T in self.tr:
            T.close()


class RosLoop:
    def __init__(self, case):
        self.p = [capi.Problem(*K, dtype=capi.EA_F64) for _ in range(N)]
        for P in self.p:
            P.set_loss(capi.LOSS_CAUCHY, 1.0)
        self.q, self.t, self.frames = np.tile([1.0, 0, 0, 0], (N, 1)), np.zeros((N, 3)), 0

    def push(self, bgr, depth):
        for i, P in enumerate(self.p):
            P.set_now_frame_ros(bgr[i], halvings=1)
            if self.frames > 0 and P.num_points > 0:
                q, t, s = P.solve(self.q[i], self.t[i])
                if s["termination"] != capi.FAILURE:
                    self.q[i], self.t[i] = q, t
            P.set_ref_frame_ros(bgr[i], depth[i], halvings=1)
        self.frames += 1
        return self.q.copy(), self.t.copy()

    def close(self):
        for P in self.p:
            P.close()


def run(leg_class, case, frames, pushes=PUSHES):
    leg = leg_class(case)
    times, poses = [], []
    for k in range(WARM + pushes):
        bgr, depth = pick(frames, k)
        s = time.perf_counter()
        q, t = leg.push(bgr, depth)
        if k >= WARM:
            times.append((time.perf_counter() - s) * 1e3)
        poses.append((q, t))
    info = {key: leg.tb.info(key) for key in ("aligned", "edge_passes", "hysteresis_rounds")} if leg_class is BatchLeg else {}
    leg.close()
    return float(np.median(times)), min(times), max(times), poses, info


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "trace":
        case, which = sys.argv[2], sys.argv[3]
        leg = (BatchLeg if which == "batch" else CannyLoop if case == "canny" else RosLoop)(case)
        frames = load(case)
        for k in range(11):
            leg.push(*pick(frames, k))
        print("trace: 11 pushes of %d streams, case %s, leg %s" % (N, case, which))
        leg.close()
        return
    ok = True
    for case in ("canny", "ros"):
        frames = load(case)
        loop_class = CannyLoop if case == "canny" else RosLoop
        runs = {"loop": [], "batch": []}
        for _ in range(2):
            runs["loop"].append(run(loop_class, case, frames))
            runs["batch"].append(run(BatchLeg, case, frames))
        # (32 VGA streams: the batch's launch heuristics take two points per lane where a lone problem takes one, so the legs
        # sum in different orders and agree to rounding, not to the bit; the repeats of a leg must agree exactly)
        dq = max(np.abs(ql - qb).max() for (ql, _), (qb, _) in zip(runs["loop"][0][3], runs["batch"][0][3]))
        dt = max(np.abs(tl - tb).max() for (_, tl), (_, tb) in zip(runs["loop"][0][3], runs["batch"][0][3]))
        for name in ("loop", "batch"):
            for (qa, ta), (qb, tb) in zip(runs[name][0][3], runs[name][1][3]):
                assert np.array_equal(qa, qb) and np.array_equal(ta, tb), (case, name)
        H, W = frames[0][1].shape
        print("case %s: %d streams of %d x %d frames, fp64, %d timed pushes per run after %d warm-up pushes; poses of the two legs differ by at most %.3g (q) and %.3g (t)"
              % (case, N, W, H, PUSHES, WARM, dq, dt))
        for name in ("loop", "batch"):
            for r, (med, lo, hi, _, info) in enumerate(runs[name]):
                print("  %-5s run %d: median push %8.3f ms   (%8.3f .. %8.3f)   per stream %7.4f ms   %s"
                      % (name, r + 1, med, lo, hi, med / N, info or ""))
        slow, fast = max(r[0] for r in runs["batch"]), min(r[0] for r in runs["loop"])
        wins = slow < fast
        ok = ok and wins
        print("  the batched push's slower run %s the loop's faster run: %.3f against %.3f ms, x %.2f"
              % ("is below" if wins else "IS NOT BELOW", slow, fast, fast / slow))
    print("PASS" if ok else "FAIL")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
