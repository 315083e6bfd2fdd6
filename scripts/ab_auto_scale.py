"""What the residual quantiles and an auto-scaled loss cost: same process, same box, on the C2 twin (640 x 480, 5e4 points,
fp64, Cauchy) as one problem and as a batch of 32 copies of it:

  quantiles     ea_batch_residual_quantiles, one probability (the median): device time between two events on the batch's
                stream around the call, and wall time of the call (it ends in its one synchronisation)
  solve off     ea_batch_solve from the identity, auto scale off, the loss scale set by hand to what auto scale estimates
                (so both forms run the same iterations: the difference is the estimate alone)
  solve on      the same with ea_problem_set_loss_auto_scale(2.385, 0.5, 1e-6)

The three alternate call by call inside a repeat; `repeats` repeats of `reps` calls after a warm-up of all three, reported as
min .. max over the repeats in microseconds, with the iterations of the solves and the wall time of one LM iteration
(solve off / iterations) to hold the quantile call against.  The launch count of a quantile call is fixed by the algorithm:
1 clear + 1 key pass + 6 x (histogram + scan) = 14.
usage: python scripts/ab_auto_scale.py [repeats]            > profiles/auto_scale_ab.txt
       python scripts/ab_auto_scale.py trace                (quantile calls only, for rocprofv3 --kernel-trace --stats)"""
import ctypes as C
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402  (first: one HIP runtime in the process)

if torch.cuda.is_available():
    torch.cuda.init()
from edge_alignment_amd import capi, synth  # noqa: E402

trace_only = len(sys.argv) > 1 and sys.argv[1] == "trace"
repeats = int(sys.argv[1]) if len(sys.argv) > 1 and not trace_only else 5
Q0, T0 = np.array([1.0, 0, 0, 0]), np.zeros(3)
FACTOR, PROB, A_MIN = 2.385, 0.5, 1e-6


def rng_of(xs):
    return "%9.2f .. %9.2f" % (min(xs), max(xs))


def batch_stream(B):
    L = capi.load()
    L.ea_internal_batch_stream.restype = C.c_void_p
    L.ea_internal_batch_stream.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    dev = C.c_int()
    return torch.cuda.ExternalStream(int(L.ea_internal_batch_stream(B._h, C.byref(dev))), device=torch.device("cuda", dev.value))


def build(cfg, count, auto):
    Ps = []
    for _ in range(count):
        P = capi.Problem(*cfg["K"], dtype=capi.EA_F64)
        P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(capi.LOSS_CAUCHY, 1.0)
        Ps.append(P)
    B = capi.Batch(Ps)
    q, t = np.tile(Q0, (count, 1)), np.tile(T0, (count, 1))
    v, m = B.residual_quantiles(q, t, [PROB])
    for i, P in enumerate(Ps):
        if auto:
            P.set_loss_auto_scale(FACTOR, PROB, A_MIN)
        else:
            P.set_loss(capi.LOSS_CAUCHY, max(A_MIN, FACTOR * v[i, 0]))
    return Ps, B, q, t


def main():
    cfg = synth.config_c2_twin()
    print("C2 twin: %d points, %s image, fp64; %d repeats" % (cfg["xyz"].shape[0], "x".join(str(s) for s in cfg["grid"].shape), repeats))
    for count in (1, 32):
        off, on = build(cfg, count, False), build(cfg, count, True)
        q, t = off[2], off[3]
        stream = batch_stream(off[1])
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        if trace_only:
            for _ in range(20):
                off[1].residual_quantiles(q, t, [PROB])
            continue
        for _ in range(5):  # warm-up: code objects, buffers, descriptors
            off[1].residual_quantiles(q, t, [PROB]); off[1].solve(q, t); on[1].solve(q, t)
        reps = 20
        dev_us, wall_us, off_us, on_us = [], [], [], []
        it_off = it_on = 0
        for _ in range(repeats):
            acc = [0.0, 0.0, 0.0, 0.0]
            for _ in range(reps):
                e0.record(stream)
                s = time.perf_counter()
                off[1].residual_quantiles(q, t, [PROB])
                acc[1] += time.perf_counter() - s
                e1.record(stream)
                e1.synchronize()
                acc[0] += e0.elapsed_time(e1) * 1e-3
                s = time.perf_counter()
                it_off = off[1].solve(q, t)[2][0]["num_iterations"]
                acc[2] += time.perf_counter() - s
                s = time.perf_counter()
                it_on = on[1].solve(q, t)[2][0]["num_iterations"]
                acc[3] += time.perf_counter() - s
            for xs, a in zip((dev_us, wall_us, off_us, on_us), acc):
                xs.append(a / reps * 1e6)
        a_on, a_off = on[0][0].get_loss()[1], off[0][0].get_loss()[1]
        assert a_on == a_off and it_on == it_off, (a_on, a_off, it_on, it_off)
        print("%2d x C2  quantiles device us %s   wall us %s   (14 launches)" % (count, rng_of(dev_us), rng_of(wall_us)))
        print("%2d x C2  solve off  wall us %s   iterations %d   us / iteration %s" % (
            count, rng_of(off_us), it_off, rng_of([x / max(it_off, 1) for x in off_us])))
        print("%2d x C2  solve on   wall us %s   iterations %d   a = %.6g" % (count, rng_of(on_us), it_on, a_on))
        for Ps, B, _, _ in (off, on):
            B.close()
            for P in Ps:
                P.close()


if __name__ == "__main__":
    main()
