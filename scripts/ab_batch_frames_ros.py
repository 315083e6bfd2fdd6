"""What producing the ROS frames of a C4 batch costs, per-problem producers against ea_batch_set_frames_ros: same process,
same box, 32 pairs from synth.config_c4_specs(32) (bundled frames, 640 x 480, depth = uint16 / 5000 as float32) in the node's
shape -- halvings = 1, producers at 320 x 240, intrinsics x 0.5 -- fp64.  Legs, each warmed up first:

  loop       Problem.set_ref_frame_ros + Problem.set_now_frame_ros (halvings = 1) for every problem, pageable numpy frames:
             the baseline
  host       Batch.set_frames_ros from the same frames in pinned host memory (capi.pinned_array)
  device     Batch.set_frames_ros from torch tensors on the GPU (frames read in place by the first halving step)

Every timed call ends synchronised (the producers return with their work done), so a time is a host clock around the call.
`repeats` repeats of 20 calls of every leg, the legs alternating call by call; a repeat's figure is its mean call, reported as
min .. max over the repeats in milliseconds (ranges, not means of repeats), and for each batched leg whether its slowest
repeat beats the loop's fastest.  The legs' results are compared bit for bit once, before the timing.

Launches and waits are counted from the code, not traced: per side the halving steps (2 for the reference side, 1 for the
current side, per halving), Sobel and NMS, 8 hysteresis launches per look at the flags, the finish, count and scan, then the
scatter (reference) or the two column passes, the exact row pass and the store (current).  Waits: one per look, the counts of
each side, the end (the per-problem reference call also waits for its points to land).  The looks of a batched call are
ea_batch_get_info("frames_hysteresis_rounds"); the loop is counted with one look per side and frame, its minimum.
usage: python scripts/ab_batch_frames_ros.py [repeats]          > profiles/batch_frames_ros_ab.txt
       python scripts/ab_batch_frames_ros.py trace [halvings]  ten host-entry calls and nothing else that launches a kernel,
                                                               to be run under a kernel / HIP API tracer: launches and waits
                                                               per call are the traced counts divided by ten"""
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
K_HALF = (0.5 * 525.0, 0.5 * 525.0, 0.5 * 319.5, 0.5 * 239.5)
N = 32
HALVINGS = 1
REPS = 20  # calls of every leg per repeat
TRACE = len(sys.argv) > 1 and sys.argv[1] == "trace"
repeats = 5 if TRACE or len(sys.argv) < 2 else int(sys.argv[1])
if TRACE and len(sys.argv) > 2:
    HALVINGS = int(sys.argv[2])
# launches of a side besides the hysteresis (no depth weighting here), and its waits besides the looks
SIDE_FIXED = {"ref": 2 * HALVINGS + 2 + 1 + 3, "now": HALVINGS + 2 + 1 + 2 + 4}


def rng_of(xs):
    return "%8.3f .. %8.3f" % (min(xs), max(xs))


def pinned(frames):
    out = capi.pinned_array((len(frames),) + frames[0].shape, frames[0].dtype)
    out[:] = np.stack(frames)
    return out


def main():
    frames = synth.load_bundled_frames(os.path.join(ROOT, "tests", "golden", "rgbd"))
    specs = synth.config_c4_specs(N)
    ref = [frames[s[0]][0] for s in specs]
    dep = [frames[s[0]][1].astype(np.float32) / np.float32(5000.0) for s in specs]
    now = [frames[s[1]][0] for s in specs]
    H, W = dep[0].shape

    def problems():
        return [capi.Problem(*K_HALF, dtype=capi.EA_F64) for _ in range(N)]

    if TRACE:
        if HALVINGS == 0:  # (frames of the working extent: the library's own reduction, before the traced calls)
            ref, now = [capi.resize_half(f) for f in ref], [capi.resize_half(f) for f in now]
            dep = [capi.resize_half(d, nan_to_zero=True) for d in dep]
        probs = problems()
        batch = capi.Batch(probs)
        pin = [pinned(ref), pinned(dep), pinned(now)]
        for _ in range(10):
            batch.set_frames_ros(*pin, halvings=HALVINGS)
        print("trace: 10 calls of Batch.set_frames_ros, %d pairs, halvings %d, looks per call %d"
              % (N, HALVINGS, batch.info("frames_hysteresis_rounds")))
        batch.close()
        for P in probs:
            P.close()
        return
    loop_p, host_p, dev_p = problems(), problems(), problems()
    host_b, dev_b = capi.Batch(host_p), capi.Batch(dev_p)
    pin = [pinned(ref), pinned(dep), pinned(now)]
    dev = [torch.from_numpy(np.stack(ref)).cuda(), torch.from_numpy(np.stack(dep)).cuda(), torch.from_numpy(np.stack(now)).cuda()]
    torch.cuda.synchronize()

    def loop():
        for P, r, d, c in zip(loop_p, ref, dep, now):
            P.set_ref_frame_ros(r, d, halvings=HALVINGS)
            P.set_now_frame_ros(c, halvings=HALVINGS)

    legs = [("loop", loop), ("host", lambda: host_b.set_frames_ros(*pin, halvings=HALVINGS)),
            ("device", lambda: dev_b.set_frames_ros(*dev, halvings=HALVINGS))]
    for _ in range(3):  # warm-up: code objects, workspaces, point and image allocations
        for _, fn in legs:
            fn()
    for name, probs in (("host", host_p), ("device", dev_p)):
        for P, R in zip(probs, loop_p):
            assert P.num_points == R.num_points and np.array_equal(P.get_points().view(np.int64), R.get_points().view(np.int64)), name
            assert np.array_equal(P.get_dt(), R.get_dt()), name
    looks = {"host": host_b.info("frames_hysteresis_rounds"), "device": dev_b.info("frames_hysteresis_rounds"), "loop": 2 * N}
    launches = {"loop": N * (SIDE_FIXED["ref"] + SIDE_FIXED["now"]) + 8 * looks["loop"]}
    waits = {"loop": looks["loop"] + 4 * N}  # per pair: the reference's count and points, the current frame's count and image
    for name in ("host", "device"):
        launches[name] = SIDE_FIXED["ref"] + SIDE_FIXED["now"] + 8 * looks[name]
        waits[name] = looks[name] + 3
    times = {name: [] for name, _ in legs}
    for _ in range(repeats):
        acc = {name: 0.0 for name, _ in legs}
        for _ in range(REPS):
            for name, fn in legs:
                s = time.perf_counter()
                fn()
                acc[name] += time.perf_counter() - s
        for name, _ in legs:
            times[name].append(acc[name] / REPS * 1e3)
    pts = [P.num_points for P in loop_p]
    print("%d ROS pairs of config_c4_specs, %d x %d halved %d time(s), fp64; %d .. %d points per problem; %d repeats of %d calls; "
          "results of every leg equal bits" % (N, W, H, HALVINGS, min(pts), max(pts), repeats, REPS))
    print("upload per pair: %.2f MB (two colour frames and one float depth frame at full size)" % ((2 * H * W * 3 + H * W * 4) / 1e6))
    for name, _ in legs:
        verdict = ""
        if name != "loop":
            wins = max(times[name]) < min(times["loop"])
            verdict = "   slowest repeat %s the loop's fastest (%.3f against %.3f): x %.2f .. %.2f" % (
                "beats" if wins else "DOES NOT beat", max(times[name]), min(times["loop"]),
                min(times["loop"]) / max(times[name]), max(times["loop"]) / min(times[name]))
        print("%-7s ms per 32 pairs %s   per pair %s   launches per 32 pairs %4d   waits %3d   looks at the hysteresis flags %3d%s"
              % (name, rng_of(times[name]), rng_of([x / N for x in times[name]]), launches[name], waits[name], looks[name], verdict))
    for b in (host_b, dev_b):
        b.close()
    for P in loop_p + host_p + dev_p:
        P.close()


if __name__ == "__main__":
    main()
