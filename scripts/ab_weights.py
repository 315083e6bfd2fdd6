"""What a weighted problem costs: same-process A/B on the C2 twin (640 x 480, 5e4 points, Cauchy 1.0), fp64 and fp32, of
ea_batch_eval (one synchronous evaluation of a one-problem batch) and ea_solve from the identity, in four forms:

  plain         no weights, no distortion: the plain kernels (what bench.py times)
  weights=1     per-point weights all 1: the weighted kernels of the variant translation unit, the plain functor
  distortion    a small Brown-Conrady distortion (k1 = 1e-4), no weights: the variant path as it was
  dist+weights  both

Wall time per call; the four forms alternate call by call inside a repeat, `repeats` repeats of `reps` calls each after a
warm-up of all four, reported as the range (min .. max over the repeats) in microseconds.  Weights of 1 change no sum
(x * 1 is exact), so the solves of a pair of forms run the same iterations: the difference is the path alone.
usage: python scripts/ab_weights.py [repeats] > profiles/weights_ab.txt"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402  (first: one HIP runtime in the process)

if torch.cuda.is_available():
    torch.cuda.init()
from edge_alignment_amd import capi, synth  # noqa: E402

repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 5
FORMS = ("plain", "weights=1", "distortion", "dist+weights")
Q0, T0 = np.array([1.0, 0, 0, 0]), np.zeros(3)


def build(cfg, dtype, form):
    P = capi.Problem(*cfg["K"], dtype=dtype)
    P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(capi.LOSS_CAUCHY, 1.0)
    if form in ("distortion", "dist+weights"):
        P.set_distortion(1e-4, 0.0, 0.0, 0.0, 0.0)
    if form in ("weights=1", "dist+weights"):
        P.set_weights(np.ones(cfg["xyz"].shape[0]))
    return P, capi.Batch([P])


def rng_of(xs):
    return "%8.2f .. %8.2f" % (min(xs), max(xs))


def main():
    cfg = synth.config_c2_twin()
    print("C2 twin: %d points, %s image; %d repeats" % (cfg["xyz"].shape[0], "x".join(str(s) for s in cfg["grid"].shape), repeats))
    for dtype, name in ((capi.EA_F64, "fp64"), (capi.EA_F32, "fp32")):
        built = {f: build(cfg, dtype, f) for f in FORMS}
        q, t = Q0.reshape(1, 4), T0.reshape(1, 3)
        for f in FORMS:  # warm-up: code objects, buffers, descriptors
            for _ in range(5):
                built[f][1].eval(q, t)
                built[f][0].solve(Q0, T0)
        for what, reps in (("ea_batch_eval", 200), ("ea_solve", 20)):
            times = {f: [] for f in FORMS}
            iters = {}
            for _ in range(repeats):
                acc = {f: 0.0 for f in FORMS}
                for _ in range(reps):
                    for f in FORMS:
                        P, B = built[f]
                        s = time.perf_counter()
                        if what == "ea_batch_eval":
                            B.eval(q, t)
                        else:
                            iters[f] = P.solve(Q0, T0)[2]["num_iterations"]
                        acc[f] += time.perf_counter() - s
                for f in FORMS:
                    times[f].append(acc[f] / reps * 1e6)
            for f in FORMS:
                print("%s %-14s %-13s us/call %s%s" % (name, what, f, rng_of(times[f]),
                                                      "   iterations %d" % iters[f] if iters else ""))
        w = built["weights=1"][1]
        print("%s info: weighted %d, fused_iterations (weights=1) %d, (plain) %d" % (
            name, w.info("weighted"), w.info("fused_iterations"), built["plain"][1].info("fused_iterations")))
        for P, B in built.values():
            B.close(); P.close()


if __name__ == "__main__":
    main()
