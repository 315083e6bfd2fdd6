"""What producing the Canny frames of a C4 batch costs, per-problem producers against ea_batch_set_frames_canny: same process,
same box, 32 pairs from synth.config_c4_specs(32) (bundled frames, 640 x 480), fp64.  Legs, each warmed up first:

  loop       Problem.set_ref_frame_canny + Problem.set_now_frame_canny for every problem (pageable numpy frames): the baseline
  host       Batch.set_frames_canny from the same pageable numpy frames
  device     Batch.set_frames_canny from torch tensors on the GPU (frames read in place: no upload inside the call)

Every timed call ends synchronised (the producers return with their work done), so a time is a host clock around the call.
`repeats` repeats of 20 calls of every leg, the legs alternating call by call; a repeat's figure is its mean call, reported as
min .. max over the repeats in milliseconds (ranges, not means of repeats), and for each batched leg whether its slowest
repeat beats the loop's fastest.  The legs' results are compared bit for bit once, before the timing.

Launches are counted, not traced: either form enqueues per side 3 launches, 8 hysteresis launches per look at the flags, the
finish, then count / scan / scatter (reference) or the chamfer's three and the store (current).  The looks of a batched call
are ea_batch_get_info("frames_hysteresis_rounds"); those of the loop follow from the hysteresis launches the per-problem debug
call reports for each frame (8 per look).
usage: python scripts/ab_batch_frames_canny.py [repeats]          > profiles/batch_frames_canny_ab.txt"""
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
N = 32
REPS = 20  # calls of every leg per repeat
repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
SIDE_FIXED = {"ref": 3 + 1 + 3, "now": 3 + 1 + 4}  # launches of a side besides the hysteresis (no depth weighting here)


def rng_of(xs):
    return "%8.3f .. %8.3f" % (min(xs), max(xs))


def main():
    frames = synth.load_bundled_frames(os.path.join(ROOT, "tests", "golden", "rgbd"))
    specs = synth.config_c4_specs(N)
    ref = [frames[s[0]][0] for s in specs]
    dep = [frames[s[0]][1] for s in specs]
    now = [frames[s[1]][0] for s in specs]
    H, W = dep[0].shape

    def problems():
        return [capi.Problem(*K, dtype=capi.EA_F64) for _ in range(N)]

    loop_p, host_p, dev_p = problems(), problems(), problems()
    host_b, dev_b = capi.Batch(host_p), capi.Batch(dev_p)
    u16 = torch.uint16 if hasattr(torch, "uint16") else torch.int16
    dev = [torch.from_numpy(np.stack(ref)).cuda(), torch.from_numpy(np.stack(dep).view(np.int16)).cuda().view(u16),
           torch.from_numpy(np.stack(now)).cuda()]
    torch.cuda.synchronize()

    def loop():
        for P, r, d, c in zip(loop_p, ref, dep, now):
            P.set_ref_frame_canny(r, d)
            P.set_now_frame_canny(c)

    legs = [("loop", loop), ("host", lambda: host_b.set_frames_canny(ref, dep, now)),
            ("device", lambda: dev_b.set_frames_canny(*dev))]
    for _ in range(3):  # warm-up: code objects, workspaces, point and image allocations
        for _, fn in legs:
            fn()
    for name, probs in (("host", host_p), ("device", dev_p)):
        for P, R in zip(probs, loop_p):
            assert P.num_points == R.num_points and np.array_equal(P.get_points(), R.get_points()), name
            assert np.array_equal(P.get_dt(), R.get_dt()), name
    looks = {"host": host_b.info("frames_hysteresis_rounds"), "device": dev_b.info("frames_hysteresis_rounds")}
    # the loop's hysteresis launches, per distinct frame from the debug call (the reference side runs the same chain on its frame)
    hyst = {}
    for k, (bgr, _) in frames.items():
        hyst[k] = loop_p[0].set_now_frame_canny(bgr, debug=True)["hysteresis_launches"]
    loop()  # (the debug calls went through problem 0)
    loop_looks = sum(-(-hyst[s[0]] // 8) - (-hyst[s[1]] // 8) for s in specs)
    launches = {"loop": N * (SIDE_FIXED["ref"] + SIDE_FIXED["now"]) + 8 * loop_looks}
    for name in ("host", "device"):
        launches[name] = SIDE_FIXED["ref"] + SIDE_FIXED["now"] + 8 * looks[name]
    looks["loop"] = loop_looks
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
    print("%d Canny pairs of config_c4_specs, %d x %d, fp64; %d .. %d points per problem; %d repeats of %d calls; results of every leg equal bits"
          % (N, W, H, min(pts), max(pts), repeats, REPS))
    print("upload per pair: %.2f MB (two colour frames and one depth frame)" % ((2 * H * W * 3 + H * W * 2) / 1e6))
    print("hysteresis launches that ran per distinct frame (per-problem debug call): %s" % sorted(hyst.values()))
    for name, _ in legs:
        verdict = ""
        if name != "loop":
            wins = max(times[name]) < min(times["loop"])
            verdict = "   slowest repeat %s the loop's fastest (%.3f against %.3f): x %.2f .. %.2f" % (
                "beats" if wins else "DOES NOT beat", max(times[name]), min(times["loop"]),
                min(times["loop"]) / max(times[name]), max(times["loop"]) / min(times[name]))
        print("%-7s ms per 32 pairs %s   per pair %s   launches per 32 pairs %4d   looks at the hysteresis flags %3d%s"
              % (name, rng_of(times[name]), rng_of([x / N for x in times[name]]), launches[name], looks[name], verdict))
    for b in (host_b, dev_b):
        b.close()
    for P in loop_p + host_p + dev_p:
        P.close()


if __name__ == "__main__":
    main()
