"""Same-process A/B on the same resident poses: ea_batch_cost_resident_poses (ea_cost_poses_kernel + ea_cost_fold_kernel)
against ea_batch_eval_resident_poses with only the cost and the failed-functor count fetched -- the full evaluation, whose
device code the cost-only change leaves as it was (scripts/compare_device_code.py).  Both are synchronous calls that end with
the results in the caller's arrays; wall time per call, the two alternating, `repeats` repeats of `reps` calls each after a
warm-up of both, reported as the range (min .. max over the repeats).

  c2      C2 (640 x 480, 5e4 points, fp64, Cauchy 1.0) at K = 2000 and K = 20
  c5      C5 (2048 x 1536, 1e6 points, fp32, trivial loss) at K = 2000
  batch   32 x C2 (fp64) at 8 poses
  search  K = 512 lattice candidates around the identity on C2: ea_batch_search_starts with M = 8 against
          ea_batch_solve_starts over all 512

Roofline fraction: G evaluations' algorithmic bytes (3 s per point + H W s per evaluation, s = element size: bench.py's
convention) over the call's wall time over the HBM peak -- a whole-call figure (launches, folds, synchronisation and unpack
included), not a kernel's.
usage: python scripts/ab_cost_poses.py [c2,c5,batch,search] [repeats]"""
import ctypes as C
import json
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402  (first: one HIP runtime in the process)

if torch.cuda.is_available():
    torch.cuda.init()
from edge_alignment_amd import capi, synth  # noqa: E402

HBM_PEAK_GBS = 8000.0
which = (sys.argv[1] if len(sys.argv) > 1 else "c2,c5,batch,search").split(",")
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
L = capi.load()


def poses(K, n, seed=7):
    rng = np.random.default_rng(seed)
    q = np.zeros((K, n, 4)); t = np.zeros((K, n, 3))
    for k in range(K):
        for i in range(n):
            q[k, i] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0.0, 0.2)))
            t[k, i] = rng.uniform(-0.005, 0.005, size=3)
    return q, t


def build(cfgs, dtype, loss):
    probs = []
    for cfg in cfgs:
        P = capi.Problem(*cfg["K"], dtype=dtype)
        P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(*loss)
        probs.append(P)
    return probs, capi.Batch(probs)


def ab(name, cfgs, dtype, loss, K, reps):
    probs, B = build(cfgs, dtype, loss)
    n = len(probs)
    q, t = poses(K, n)
    B.set_poses(q, t)
    cost_a, bad_a = np.zeros((K, n)), np.zeros((K, n), dtype=np.int64)
    cost_b, bad_b = np.zeros((K, n)), np.zeros((K, n), dtype=np.int64)
    pa = (capi._dp(cost_a), bad_a.ctypes.data_as(C.POINTER(C.c_int64)))
    pb = (capi._dp(cost_b), bad_b.ctypes.data_as(C.POINTER(C.c_int64)))

    def run_cost():
        assert L.ea_batch_cost_resident_poses(B._h, pa[0], pa[1]) == 0, L.ea_last_error()

    def run_eval():
        assert L.ea_batch_eval_resident_poses(B._h, pb[0], None, None, pb[1]) == 0, L.ea_last_error()

    for _ in range(3):   # warm-up of both shapes: code objects, buffers, the pinned result block
        run_cost(); run_eval()
    assert B.info("cost_form") == 1
    rel = float(np.abs(cost_a - cost_b).max() / np.abs(cost_b).max())
    assert np.array_equal(bad_a, bad_b)
    ta, tb = [], []
    for _ in range(repeats):
        s = time.perf_counter()
        for _ in range(reps):
            run_cost()
        ta.append((time.perf_counter() - s) / reps)
        s = time.perf_counter()
        for _ in range(reps):
            run_eval()
        tb.append((time.perf_counter() - s) / reps)
    esize = 8 if dtype == capi.EA_F64 else 4
    by = K * sum(3 * esize * c["xyz"].shape[0] + c["image"].shape[0] * c["image"].shape[1] * esize for c in cfgs)
    out = {"K": K, "problems": n, "poses_per_launch": B.info("poses_per_launch"), "reps_per_repeat": reps,
           "cost_only_us_per_call": [min(ta) * 1e6, max(ta) * 1e6], "full_eval_us_per_call": [min(tb) * 1e6, max(tb) * 1e6],
           "cost_only_us_per_evaluation": [min(ta) * 1e6 / K, max(ta) * 1e6 / K],
           "full_eval_us_per_evaluation": [min(tb) * 1e6 / K, max(tb) * 1e6 / K],
           "slowest_cost_only_faster_than_fastest_full_eval": max(ta) < min(tb),
           "ratio_full_over_cost_worst_to_best": [min(tb) / max(ta), max(tb) / min(ta)],
           "whole_call_roofline_frac_cost_only": [by / max(ta) / 1e9 / HBM_PEAK_GBS, by / min(ta) / 1e9 / HBM_PEAK_GBS],
           "whole_call_roofline_frac_full_eval": [by / max(tb) / 1e9 / HBM_PEAK_GBS, by / min(tb) / 1e9 / HBM_PEAK_GBS],
           "max_rel_cost_difference": rel}
    print(name, json.dumps(out), flush=True)
    B.close()
    for P in probs:
        P.close()
    return out


results = {}
if "c2" in which:
    c2 = synth.config_c2_twin(seed=2, n_points=50000)
    results["c2_fp64_K2000"] = ab("c2_fp64_K2000", [c2], capi.EA_F64, (capi.LOSS_CAUCHY, 1.0), 2000, 50)
    results["c2_fp64_K20"] = ab("c2_fp64_K20", [c2], capi.EA_F64, (capi.LOSS_CAUCHY, 1.0), 20, 2000)
if "c5" in which:
    results["c5_fp32_K2000"] = ab("c5_fp32_K2000", [synth.config_c5()], capi.EA_F32, (capi.LOSS_TRIVIAL, 1.0), 2000, 5)
if "batch" in which:
    batch = [synth.config_c2_twin(seed=100 + i) for i in range(32)]
    results["batch32_c2_fp64_K8"] = ab("batch32_c2_fp64_K8", batch, capi.EA_F64, (capi.LOSS_CAUCHY, 1.0), 8, 300)
if "search" in which:
    c2 = synth.config_c2_twin(seed=2, n_points=50000)
    probs, B = build([c2], capi.EA_F64, (capi.LOSS_CAUCHY, 1.0))
    q, t = synth.pose_lattice([1.0, 0, 0, 0], np.zeros(3), [0.02, 0.02, 0.02, 0.03, 0.03, 0.03], [2, 2, 2, 4, 4, 4])
    K, M = q.shape[0], 8
    assert K == 512
    q, t = q[:, None, :], t[:, None, :]
    ts, tf = [], []
    for r in range(repeats + 1):   # (round 0 warms both up)
        s = time.perf_counter()
        qo, to, picked, _, best = B.search_starts(q, t, M, summaries=False)
        a = time.perf_counter() - s
        s = time.perf_counter()
        qa, ta_, _, best_all = B.solve_starts(q, t, summaries=False)
        b = time.perf_counter() - s
        if r:
            ts.append(a); tf.append(b)
    ang = synth.rotation_angle_between(qo[best[0], 0], c2["q_true"]); dt = float(np.linalg.norm(to[best[0], 0] - c2["t_true"]))
    ang_all = synth.rotation_angle_between(qa[best_all[0], 0], c2["q_true"]); dt_all = float(np.linalg.norm(ta_[best_all[0], 0] - c2["t_true"]))
    results["search_c2_K512_M8"] = {"search_starts_ms": [min(ts) * 1e3, max(ts) * 1e3], "solve_starts_all_512_ms": [min(tf) * 1e3, max(tf) * 1e3],
                                    "picked": [int(x) for x in picked[:, 0]], "best_rank": int(best[0]),
                                    "best_pose_error_search": [ang, dt], "best_pose_error_all": [ang_all, dt_all]}
    print("search_c2_K512_M8", json.dumps(results["search_c2_K512_M8"]), flush=True)
    B.close(); probs[0].close()
print(json.dumps(results))
