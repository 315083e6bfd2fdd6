"""What coarse-to-fine tracking of 32 streams costs and gives: same process, same box, fp64, 1280 x 960 frames (the bundled
frames enlarged by pixel repetition, depth = uint16 / 5000 as float32) in ea_host_alloc memory, halvings = 1, levels 1..3, the
camera of level l scaled by 2^-(1 + l); stream i sees bundled frame (i + k) % 5 at push k.  Three parts:

  (a) time per push   TrackerBatch(levels = L) against the per-stream loop of calls that existed before it: per problem and
      level set_now_frame_ros(halvings = 1 + l), ea_solve_pyramid over the levels from the prior, per level
      set_ref_frame_ros(halvings = 1 + l).  A run is 2 warm-up pushes (the first aligns nothing) and 12 timed ones on fresh
      trackers; a run's figure is the MEDIAN push; each L runs loop, batch, loop, batch.
  (b) frame side alone   set_frames_ros_pyramid(L levels) against Batch.set_frames_ros once per level (both sides, host
      frames), 2 warm-up calls and 12 timed ones, interleaved the same way; with the uploads and halving launches each issues
      (uploads: "frames_uploaded" / 3 N per single-level call; halving launches: counted from the code, per side one launch per
      kind and three steps for the chain, one per kind and step for the single-level call).
  (c) what the levels buy   the five bundled pairs at 640 x 480, halvings = 1, the current frame shifted right by 4, 8, 16 and
      32 px (edge columns repeated): final level-0 cost and translation from levels = 1 and from levels = 3, both started at
      identity (solve_pyramid_batch).

Every timed call ends synchronised, so a time is a host clock around the call.  Nothing here is asserted but that the
repeats of a leg agree exactly: the figures are the result.

usage: python scripts/ab_tracker_pyramid.py > profiles/tracker_pyramid_ab.txt"""
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
K = (525.0, 525.0, 319.5, 239.5)                 # at 640 x 480
N, WARM, TIMED, HALVINGS = 32, 2, 12, 1


def pinned(a):
    out = capi.pinned_array(a.shape, a.dtype)
    out[:] = a
    return out


def bundled():
    frames = synth.load_bundled_frames(os.path.join(ROOT, "tests", "golden", "rgbd"))
    return [(frames[k][0], frames[k][1].astype(np.float32) / np.float32(5000.0)) for k in range(1, 6)]


def enlarged(frames):
    """1280 x 960, page-locked"""
    return [(pinned(np.ascontiguousarray(np.repeat(np.repeat(b, 2, axis=0), 2, axis=1))),
             pinned(np.ascontiguousarray(np.repeat(np.repeat(d, 2, axis=0), 2, axis=1)))) for b, d in frames]


def cam(level, full_scale=1.0):
    """the camera of `level`: K belongs to 640 x 480, the frames are full_scale times that"""
    s = full_scale / (1 << (HALVINGS + level))
    return tuple(k * s for k in K)


def pick(frames, k):
    return [frames[(i + k) % 5][0] for i in range(N)], [frames[(i + k) % 5][1] for i in range(N)]


class BatchLeg:
    def __init__(self, levels):
        self.tb = capi.TrackerBatch([[cam(l, 2.0)] * N for l in range(levels)], dtype=capi.EA_F64, flavour=2, halvings=HALVINGS,
                                    levels=levels)
        for l in range(levels):
            for i in range(N):
                self.tb.level_problem(l, i).set_loss(capi.LOSS_CAUCHY, 1.0)

    def push(self, bgr, depth):
        q, t, _, _ = self.tb.push_frames(bgr, depth)
        return q, t

    def close(self):
        self.tb.close()


class LoopLeg:
    def __init__(self, levels):
        self.levels = levels
        self.p = [[capi.Problem(*cam(l, 2.0), dtype=capi.EA_F64) for l in range(levels)] for _ in range(N)]
        for Ps in self.p:
            for P in Ps:
                P.set_loss(capi.LOSS_CAUCHY, 1.0)
        self.q, self.t, self.frames = np.tile([1.0, 0, 0, 0], (N, 1)), np.zeros((N, 3)), 0

    def push(self, bgr, depth):
        for i, Ps in enumerate(self.p):
            for l, P in enumerate(Ps):
                P.set_now_frame_ros(bgr[i], halvings=HALVINGS + l)
            if self.frames > 0 and all(P.num_points > 0 for P in Ps):
                q, t, s = capi.solve_pyramid(Ps, self.q[i], self.t[i])
                if all(x["termination"] != capi.FAILURE for x in s):
                    self.q[i], self.t[i] = q, t
            for l, P in enumerate(Ps):
                P.set_ref_frame_ros(bgr[i], depth[i], halvings=HALVINGS + l)
        self.frames += 1
        return self.q.copy(), self.t.copy()

    def close(self):
        for Ps in self.p:
            for P in Ps:
                P.close()


def run_pushes(leg_class, levels, frames):
    leg = leg_class(levels)
    times, poses = [], []
    for k in range(WARM + TIMED):
        bgr, depth = pick(frames, k)
        s = time.perf_counter()
        q, t = leg.push(bgr, depth)
        if k >= WARM:
            times.append((time.perf_counter() - s) * 1e3)
        poses.append((q, t))
    info = {key: leg.tb.info(key) for key in ("aligned", "edge_passes", "levels")} if leg_class is BatchLeg else {}
    leg.close()
    return float(np.median(times)), min(times), max(times), poses, info


def part_a(frames):
    print("(a) time per push: %d streams of 1280 x 960 frames, halvings = %d, fp64, %d timed pushes per run after %d warm-up pushes"
          % (N, HALVINGS, TIMED, WARM))
    for levels in (1, 2, 3):
        runs = {"loop": [], "batch": []}
        for _ in range(2):
            runs["loop"].append(run_pushes(LoopLeg, levels, frames))
            runs["batch"].append(run_pushes(BatchLeg, levels, frames))
        for name in ("loop", "batch"):
            for (qa, ta), (qb, tb) in zip(runs[name][0][3], runs[name][1][3]):
                assert np.array_equal(qa, qb) and np.array_equal(ta, tb), (levels, name)
        dq = max(np.abs(ql - qb).max() for (ql, _), (qb, _) in zip(runs["loop"][0][3], runs["batch"][0][3]))
        dt = max(np.abs(tl - tb).max() for (_, tl), (_, tb) in zip(runs["loop"][0][3], runs["batch"][0][3]))
        print("  levels = %d; poses of the two legs differ by at most %.3g (q) and %.3g (t)" % (levels, dq, dt))
        for name in ("loop", "batch"):
            for r, (med, lo, hi, _, info) in enumerate(runs[name]):
                print("    %-5s run %d: median push %8.3f ms   (%8.3f .. %8.3f)   per stream %7.4f ms   %s"
                      % (name, r + 1, med, lo, hi, med / N, info or ""))
        slow, fast = max(r[0] for r in runs["batch"]), min(r[0] for r in runs["loop"])
        print("    the batched push's slower run against the loop's faster run: %.3f against %.3f ms, x %.2f" % (slow, fast, fast / slow))


def timed_calls(call):
    times = []
    for k in range(WARM + TIMED):
        s = time.perf_counter()
        call()
        if k >= WARM:
            times.append((time.perf_counter() - s) * 1e3)
    return float(np.median(times)), min(times), max(times)


def part_b(frames):
    print("(b) frame side alone: %d pairs of 1280 x 960 host frames, both sides, halvings = %d, fp64, %d timed calls per run after %d"
          % (N, HALVINGS, TIMED, WARM))
    ref, dep = pick(frames, 0)
    now, _ = pick(frames, 1)
    for levels in (1, 2, 3):
        probs = [[capi.Problem(*cam(l, 2.0), dtype=capi.EA_F64) for _ in range(N)] for l in range(levels)]
        batches = [capi.Batch(p) for p in probs]

        def per_level():
            for l, b in enumerate(batches):
                b.set_frames_ros(ref, dep, now, halvings=HALVINGS + l)

        def pyramid():
            capi.set_frames_ros_pyramid(batches, ref, dep, now, halvings=HALVINGS)

        runs = {"per level": [], "pyramid": []}
        for _ in range(2):
            runs["per level"].append(timed_calls(per_level))
            runs["pyramid"].append(timed_calls(pyramid))
        uploaded = batches[0].info("frames_uploaded")
        steps = HALVINGS + levels - 1
        launches = {"per level": 3 * sum(HALVINGS + l for l in range(levels)), "pyramid": 3 * ((steps + 2) // 3)}
        uploads = {"per level": 3 * N * levels, "pyramid": uploaded}
        print("  levels = %d" % levels)
        for name in ("per level", "pyramid"):
            for r, (med, lo, hi) in enumerate(runs[name]):
                print("    %-9s run %d: median call %8.3f ms   (%8.3f .. %8.3f)   frame uploads %4d   halving launches %2d"
                      % (name, r + 1, med, lo, hi, uploads[name], launches[name]))
        slow, fast = max(r[0] for r in runs["pyramid"]), min(r[0] for r in runs["per level"])
        print("    the pyramid call's slower run against the per-level calls' faster run: %.3f against %.3f ms, x %.2f"
              % (slow, fast, fast / slow))
        for b in batches:
            b.close()
        for p in probs:
            for P in p:
                P.close()


def shifted(img, s):
    out = np.empty_like(img)
    out[:, s:] = img[:, :img.shape[1] - s]
    out[:, :s] = img[:, :1]
    return out


def part_c(frames):
    pairs = ((0, 1), (1, 2), (2, 3), (3, 4), (4, 0))
    n = len(pairs)
    print("(c) final level-0 cost and translation after a shift of the current frame: the five bundled pairs at 640 x 480,"
          " halvings = %d, from identity" % HALVINGS)
    q0, t0 = np.tile([1.0, 0, 0, 0], (n, 1)), np.zeros((n, 3))
    for shift in (0, 4, 8, 16, 32):
        ref, dep = [frames[a][0] for a, _ in pairs], [frames[a][1] for a, _ in pairs]
        now = [shifted(frames[b][0], shift) if shift else frames[b][0] for _, b in pairs]
        rows = {}
        for levels in (1, 3):
            probs = [[capi.Problem(*cam(l), dtype=capi.EA_F64) for _ in range(n)] for l in range(levels)]
            for p in probs:
                for P in p:
                    P.set_loss(capi.LOSS_CAUCHY, 1.0)
            batches = [capi.Batch(p) for p in probs]
            capi.set_frames_ros_pyramid(batches, ref, dep, now, halvings=HALVINGS)
            q, t, sums = capi.solve_pyramid_batch(batches, q0, t0)
            rows[levels] = ([s["final_cost"] for s in sums[0]], [s["initial_cost"] for s in sums[0]], t,
                            [[s["num_iterations"] for s in lv] for lv in sums])
            for b in batches:
                b.close()
            for p in probs:
                for P in p:
                    P.close()
        print("  shift %2d px (%g px at level 0)" % (shift, shift / (1 << HALVINGS)))
        for i in range(n):
            c1, c3 = rows[1][0][i], rows[3][0][i]
            print("    pair %d: cost at identity %10.2f   levels = 1: final %10.2f  t = (%+.4f %+.4f %+.4f)  iterations %s"
                  "   levels = 3: final %10.2f  t = (%+.4f %+.4f %+.4f)  iterations (level 0, 1, 2) %s   cost ratio 3 / 1: %.3f"
                  % (i, rows[1][1][i], c1, *rows[1][2][i], rows[1][3][0][i], c3, *rows[3][2][i], [lv[i] for lv in rows[3][3]],
                     c3 / c1 if c1 else float("nan")))
        print("    median final level-0 cost: levels = 1 %10.2f   levels = 3 %10.2f"
              % (float(np.median(rows[1][0])), float(np.median(rows[3][0]))))


def main():
    small = bundled()
    big = enlarged(small)
    part_a(big)
    part_b(big)
    part_c(small)
    return 0


if __name__ == "__main__":
    sys.exit(main())
