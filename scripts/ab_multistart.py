"""Same-process A/B: K starts of one problem through ea_solve_starts (lock-step on the device) against the same K starts as
K sequential ea_solve calls -- an entry point the multi-start change does not touch.  Problem: C2-sized (the bench's
generator, 5e4 points, fp64, Cauchy 1.0); starts: drawn around the identity (up to 1.5 degrees / 3 cm), the identity first.
For K in {1, 8, 64, 512}: wall time per call, median over interleaved rounds after warm-up, with the spread (min .. max of
the rounds) of both; the evaluation launches of the call ("starts_launches") and, from an event pair around the queued
launches ("starts_events", in rounds of their own), the device time per queued iteration.
usage: python scripts/ab_multistart.py [rounds]"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402  (first: one HIP runtime in the process)

if torch.cuda.is_available():
    torch.cuda.init()
from edge_alignment_amd import capi, synth  # noqa: E402

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
cfg = synth.config_c2_twin(seed=2, n_points=50000)
P = capi.Problem(*cfg["K"], dtype=capi.EA_F64)
P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(capi.LOSS_CAUCHY, 1.0)
B = capi.Batch([P])


def starts(K, seed=5):
    rng = np.random.default_rng(seed)
    q = np.zeros((K, 4)); t = np.zeros((K, 3))
    for k in range(K):
        q[k] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0, 1.5)))
        t[k] = rng.uniform(-0.03, 0.03, 3)
    q[0] = [1.0, 0, 0, 0]; t[0] = 0.0
    return q, t


def stats(v):
    v = sorted(v)
    return {"median_ms": v[len(v) // 2] * 1e3, "min_ms": v[0] * 1e3, "max_ms": v[-1] * 1e3}


out = {}
for K in (1, 8, 64, 512):
    q0, t0 = starts(K)
    reps = max(1, 64 // K)
    new, old = [], []
    its_new = its_old = None
    for r in range(rounds + 1):            # (round 0 is the warm-up of both)
        t_ = time.perf_counter()
        for _ in range(reps):
            q, t, s, best = B.solve_starts(q0[:, None, :], t0[:, None, :])
        a = (time.perf_counter() - t_) / reps
        t_ = time.perf_counter()
        for _ in range(reps):
            seq = [B.solve(q0[k], t0[k]) for k in range(K)]
        b = (time.perf_counter() - t_) / reps
        if r:
            new.append(a); old.append(b)
        its_new = [x[0]["num_iterations"] for x in s]
        its_old = [x[2][0]["num_iterations"] for x in seq]
    launches = B.info("starts_launches")
    B.set_tuning("starts_events", 1)
    dev = []
    for r in range(3):
        B.solve_starts(q0[:, None, :], t0[:, None, :])
        dev.append(B.info("starts_device_ns") / max(1, B.info("starts_iterations")) / 1e3)
    B.set_tuning("starts_events", 0)
    a, b = stats(new), stats(old)
    out["K%d" % K] = {"solve_starts": a, "sequential_ea_solve": b, "speedup_median": b["median_ms"] / a["median_ms"],
                      "faster_beyond_baseline_spread": a["median_ms"] < b["min_ms"] - (b["max_ms"] - b["min_ms"]),
                      "starts_launches": launches, "device_us_per_queued_iteration": sorted(dev)[1], "device_us_per_queued_iteration_min_max": [min(dev), max(dev)],
                      "iterations_max_new": max(its_new), "iterations_sum_new": sum(its_new), "iterations_sum_old": sum(its_old),
                      "converged_new": sum(x[0]["termination"] == capi.CONVERGENCE for x in s),
                      "converged_old": sum(x[2][0]["termination"] == capi.CONVERGENCE for x in seq)}
    print("K", K, json.dumps(out["K%d" % K]), flush=True)
print(json.dumps(out))
