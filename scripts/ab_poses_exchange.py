"""Same-process A/B of the two reductions of the fp64 pose-batched evaluation (tuning key "poses_wave_exchange": 0 = one
32-value butterfly per wavefront and a cross-wave sum, 1 = the wave-exchange reduction of ea_wave_exchange.h) on the same
batch and the same poses, the key alternating 0 / 1 / 0 / 1 ...:

  launches  ms per run of the resident poses' launches between one event pair on the library's stream
            (ea_batch_bench_resident_poses, 5 runs per figure), with and without the fold launches
  calls     wall time per synchronous ea_batch_eval_resident_poses call that ends with the results in the caller's arrays

  c2      C2 (640 x 480, 5e4 points, fp64, Cauchy 1.0) at K = 2000 and K = 20
  batch   32 x C2 (fp64) at 8 poses

Per setting the range (min .. max) over `repeats` alternations; the results of the two settings are compared on the way
(cost to 1e-13 relative, failed-functor counts equal), and "poses_wave_exchange" of ea_batch_get_info must say which ran.
usage: python scripts/ab_poses_exchange.py [c2,batch] [repeats]"""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402  (first: one HIP runtime in the process)

if torch.cuda.is_available():
    torch.cuda.init()
from edge_alignment_amd import capi, synth  # noqa: E402
import bench  # noqa: E402

which = (sys.argv[1] if len(sys.argv) > 1 else "c2,batch").split(",")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5


def ab(name, cfgs, K, reps):
    probs = []
    for cfg in cfgs:
        P = capi.Problem(*cfg["K"], dtype=capi.EA_F64)
        P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(capi.LOSS_CAUCHY, 1.0)
        probs.append(P)
    B = capi.Batch(probs)
    n = len(probs)
    Q, T = bench.step_poses(K, 1000)
    Q = np.repeat(Q.reshape(K, 1, 4), n, axis=1); T = np.repeat(T.reshape(K, 1, 3), n, axis=1)
    ev = {0: [], 1: []}; evo = {0: [], 1: []}; wall = {0: [], 1: []}
    outs = {}
    launches = 0
    for r in range(repeats + 1):  # (alternation 0 warms both settings up)
        for key in (0, 1):
            B.set_tuning("poses_wave_exchange", key)
            B.set_poses(Q, T)
            out = B.eval_resident_poses()
            assert B.info("poses_wave_exchange") == key, (key, B.info("poses_wave_exchange"))
            outs[key] = {k: out[k].copy() for k in ("cost", "n_invalid")}
            ms, launches = B.bench_resident_poses(5)
            mse, _ = B.bench_resident_poses(5, evaluations_only=True)
            s = time.perf_counter()
            for _ in range(reps):
                B.eval_resident_poses(out=out)
            w = (time.perf_counter() - s) / reps
            if r:
                ev[key].append(ms * 1e3); evo[key].append(mse * 1e3 / launches); wall[key].append(w * 1e6)
    rel = float(np.abs(outs[0]["cost"] - outs[1]["cost"]).max() / np.abs(outs[0]["cost"]).max())
    assert rel <= 1e-13, rel
    assert np.array_equal(outs[0]["n_invalid"], outs[1]["n_invalid"])
    rng = lambda v: [min(v), max(v)]
    res = {"K": K, "problems": n, "evaluation_launches": launches, "poses_per_launch": B.info("poses_per_launch"),
           "launches_us_per_run": {"butterfly": rng(ev[0]), "exchange": rng(ev[1])},
           "evaluation_launch_us": {"butterfly": rng(evo[0]), "exchange": rng(evo[1])},
           "wall_us_per_call": {"butterfly": rng(wall[0]), "exchange": rng(wall[1])},
           "slowest_exchange_launch_faster_than_fastest_butterfly": max(evo[1]) < min(evo[0]),
           "slowest_exchange_call_faster_than_fastest_butterfly": max(wall[1]) < min(wall[0]),
           "median_ratio_exchange_over_butterfly": {"evaluation_launch": float(np.median(evo[1]) / np.median(evo[0])),
                                                    "wall": float(np.median(wall[1]) / np.median(wall[0]))},
           "max_rel_cost_difference": rel}
    print(name, json.dumps(res), flush=True)
    B.close()
    for P in probs:
        P.close()
    return res


results = {}
if "c2" in which:
    c2 = synth.config_c2_twin(seed=2, n_points=50000)
    results["c2_fp64_K2000"] = ab("c2_fp64_K2000", [c2], 2000, 30)
    results["c2_fp64_K20"] = ab("c2_fp64_K20", [c2], 20, 1000)
if "batch" in which:
    results["batch32_c2_fp64_K8"] = ab("batch32_c2_fp64_K8", [synth.config_c2_twin(seed=100 + i) for i in range(32)], 8, 200)
print(json.dumps(results))
