"""Two builds of the library on one box, alternating processes: kernel time per evaluation of the pose-batched launches (C5 fp32,
C2 fp32, C2 fp64).  usage: python scripts/ab_two_builds_poses.py libA.so libB.so [--bits]
--bits: instead of timing, the results of 20 poses on C2 fp64 from both builds, (a) at threads = 1024, where both builds fold
with 1024-thread workgroups in the same order -- equal partial rows then mean equal bits -- and (b) at the default shape;
then the same poses through the other kernels that share the head of a work item, each at buffer_loads 1 and 0: cost_poses,
one solve_starts from the first four (poses, iteration counts, it_cost), and ea_solve from the first with fused_iterations
on and off; and the three forms of the LM step (fused, pair, K = 4 starts), lm / dogleg x {no side table, NormalPrior on t, held
coordinates}: pose, counts, costs and all seven trace arrays.  Every array must be array_equal between the builds: exit
status 1 otherwise.
--poses K: instead of timing, the results of K poses on C2 fp64 (Cauchy) at the default tuning from both builds -- the
one-pose-per-lane kernel from 1024 poses on, ea_eval_poses_kernel below -- and which kernel ran.  JtJ, Jtr and n_invalid must
be array_equal (exit status 1 otherwise); the cost is reported: equal bits, or the largest relative difference over the poses."""
import sys, os, json, subprocess
POSES = r'''
import sys, numpy as np
sys.path.insert(0, '.')
import torch; torch.cuda.init()
from edge_alignment_amd import capi, synth
capi.LIB_PATH = sys.argv[1]
import bench
cfg = synth.config_c2_twin(seed=2, n_points=50000)
P = capi.Problem(*cfg["K"], dtype=capi.EA_F64); P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(capi.LOSS_CAUCHY, 1.0)
B = capi.Batch([P])
Q, T = bench.step_poses(int(sys.argv[3]), 1000)
r = B.eval_poses(Q, T)
np.savez(sys.argv[2], lanes=np.array(B.info("poses_lane_per_pose")), **r)
B.close(); P.close()
'''
CHILD = r'''
import sys, numpy as np
sys.path.insert(0, '.')
import torch; torch.cuda.init()
from edge_alignment_amd import capi, synth
capi.LIB_PATH = sys.argv[1]
import bench
out = {}
def run(name, cfg, dtype, loss, K):
    P = capi.Problem(*cfg["K"], dtype=dtype); P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(*loss)
    B = capi.Batch([P])
    Q, T = bench.step_poses(K, 1000)
    B.set_poses(Q, T)
    ms, nl = min(B.bench_resident_poses(5, evaluations_only=True) for _ in range(4))
    out[name] = ms * 1e3 / K
    B.close(); P.close()
run("c5_f32_us_per_eval", synth.config_c5(), capi.EA_F32, (capi.LOSS_TRIVIAL, 1.0), 400)
run("c2_f32_us_per_eval", synth.config_c2_twin(seed=2, n_points=50000), capi.EA_F32, (capi.LOSS_CAUCHY, 1.0), 2000)
run("c2_f64_us_per_eval", synth.config_c2_twin(seed=2, n_points=50000), capi.EA_F64, (capi.LOSS_CAUCHY, 1.0), 2000)
import json; print(json.dumps(out))
'''
BITS = r'''
import sys, json, numpy as np
sys.path.insert(0, '.')
import torch; torch.cuda.init()
from edge_alignment_amd import capi, synth
capi.LIB_PATH = sys.argv[1]
import bench
cfg = synth.config_c2_twin(seed=2, n_points=50000)
out = {}
def pad(v):   # a trace, NaN-padded to 11 rows
    a = np.full(11, np.nan); v = np.asarray(v, dtype=np.float64)[:11]; a[:len(v)] = v
    return a
TRACE = ("it_cost", "it_cost_change", "it_gradient_max_norm", "it_step_norm", "it_relative_decrease", "it_radius", "it_successful")
def whole(r, name, q, t, s):   # a solve's whole result: pose, counts, costs, the seven trace arrays
    r.update({name + "_q": q, name + "_t": t})
    for k in ("termination", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost"):
        r[name + "_" + k] = np.array([x[k] for x in s], dtype=np.float64)
    for k in TRACE:
        r[name + "_" + k] = np.array([pad(x[k]) for x in s])
def step_cells(r, dtype, buf, Q, T):   # the three forms of the LM step: lm / dogleg x {no side table, prior on t, held coordinates}
    for strat, sname in ((capi.STRATEGY_LM, "lm"), (capi.STRATEGY_DOGLEG, "dogleg")):
        for side in ("none", "prior", "mask"):
            P = capi.Problem(*cfg["K"], dtype=dtype); P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(capi.LOSS_CAUCHY, 1.0)
            if side == "prior":
                P.set_normal_prior(1, 5.0 * np.eye(3), np.array([0.01, -0.005, 0.02]))
            elif side == "mask":
                P.set_constant_parameters([0, 0, 1, 0, 1, 0])
            B = capi.Batch([P])
            B.set_tuning("buffer_loads", buf)
            name = "step_%s_%s" % (sname, side)
            for fused in (-1, 0):
                B.set_tuning("fused_iterations", fused)
                q, t, s = B.solve(Q[0], T[0], max_num_iterations=10, strategy=strat)
                whole(r, name + ("_fused" if fused else "_pair"), q, t, s)
                r[name + ("_fused" if fused else "_pair") + "_form"] = np.array(B.info("fused_iterations"))
            q, t, s, best = B.solve_starts(Q[:4], T[:4], max_num_iterations=10, strategy=strat)
            whole(r, name + "_starts", q.reshape(-1, 4), t.reshape(-1, 3), [x for row in s for x in row])
            r[name + "_starts_best"] = best
            r[name + "_starts_form"] = np.array(B.info("starts_form"))
            B.close(); P.close()
for dtype, tag in ((capi.EA_F64, "f64"), (capi.EA_F32, "f32")):
    P = capi.Problem(*cfg["K"], dtype=dtype); P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(capi.LOSS_CAUCHY, 1.0)
    B = capi.Batch([P])
    Q, T = bench.step_poses(20, 1000)
    for nt in (1024, 256):
        B.set_tuning("threads", nt)
        for g in (0, 7):
            B.set_tuning("poses_per_launch", g)
            r = B.eval_poses(Q, T)
            np.savez(sys.argv[2] + "_%s_%d_%d.npz" % (tag, nt, g), **r)
    B.set_tuning("poses_per_launch", 0)
    for buf in (1, 0):
        B.set_tuning("buffer_loads", buf)
        r = {"eval_" + k: v for k, v in B.eval_poses(Q, T).items()}
        r.update({"cost_" + k: v for k, v in B.cost_poses(Q, T).items()})
        q, t, s, best = B.solve_starts(Q[:4], T[:4], max_num_iterations=10)
        r.update(starts_q=q, starts_t=t, starts_best=best, starts_iterations=np.array([[x["num_iterations"] for x in row] for row in s]),
                 starts_it_cost=np.array([[pad(x["it_cost"]) for x in row] for row in s]))
        for fused in (-1, 0):
            B.set_tuning("fused_iterations", fused)
            q, t, s = B.solve(Q[0], T[0], max_num_iterations=10)
            r.update({"solve%d_q" % fused: q, "solve%d_t" % fused: t, "solve%d_fused" % fused: np.array(B.info("fused_iterations")),
                      "solve%d_iterations" % fused: np.array([x["num_iterations"] for x in s]),
                      "solve%d_it_cost" % fused: np.array([pad(x["it_cost"]) for x in s])})
        step_cells(r, dtype, buf, Q, T)
        np.savez(sys.argv[2] + "_%s_paths_buf%d.npz" % (tag, buf), **r)
    B.close(); P.close()
'''
if "--poses" in sys.argv:
    import numpy as np, tempfile
    K = sys.argv[sys.argv.index("--poses") + 1]
    libs = sys.argv[1:3]
    tmp = tempfile.mkdtemp()
    for i, l in enumerate(libs):
        o = subprocess.run(["timeout", "-k", "10", "300", sys.executable, '-c', POSES, os.path.abspath(l), os.path.join(tmp, "p%d.npz" % i), K], capture_output=True, text=True)
        if o.returncode != 0:
            print(l, 'FAILED', o.returncode, o.stderr[-1500:]); sys.exit(1)
    a, b = (np.load(os.path.join(tmp, "p%d.npz" % i)) for i in (0, 1))
    same = {f: bool(np.array_equal(a[f], b[f])) for f in ("cost", "JtJ", "Jtr", "n_invalid")}
    rel = float((np.abs(a["cost"] - b["cost"]) / np.abs(a["cost"])).max())
    print("K", K, "poses_lane_per_pose", int(a["lanes"]), int(b["lanes"]), "array_equal", same, "largest relative cost difference %.3g" % rel)
    sys.exit(0 if same["JtJ"] and same["Jtr"] and same["n_invalid"] and np.all(np.isfinite(b["cost"])) else 1)
if "--bits" in sys.argv:
    import numpy as np, tempfile
    libs = [a for a in sys.argv[1:] if a != "--bits"][:2]
    tmp = tempfile.mkdtemp()
    for i, l in enumerate(libs):
        o = subprocess.run(["timeout", "-k", "10", "300", sys.executable, '-c', BITS, os.path.abspath(l), os.path.join(tmp, "r%d" % i)], capture_output=True, text=True)
        if o.returncode != 0:
            print(l, 'FAILED', o.returncode, o.stderr[-1500:]); sys.exit(1)
    for tag in ("f64", "f32"):
        for nt in (1024, 256):
            for g in (0, 7):
                a, b = (np.load(os.path.join(tmp, "r%d_%s_%d_%d.npz" % (i, tag, nt, g))) for i in (0, 1))
                print(tag, "threads", nt, "poses_per_launch", g, {f: ("equal bits" if np.array_equal(a[f], b[f]) else
                      "max |d| / max |.| = %.3g" % (np.abs(a[f] - b[f]).max() / np.abs(a[f]).max())) for f in ("cost", "JtJ", "Jtr", "n_invalid")})
    differ = []
    for tag in ("f64", "f32"):
        for buf in (1, 0):
            a, b = (np.load(os.path.join(tmp, "r%d_%s_paths_buf%d.npz" % (i, tag, buf))) for i in (0, 1))
            bad = [f for f in a.files if not np.array_equal(a[f], b[f], equal_nan=True)]
            differ += bad
            print(tag, "buffer_loads", buf, "%d arrays (eval_poses, cost_poses, solve_starts K = 4, ea_solve fused %s / %s):" %
                  (len(a.files), a["solve-1_fused"], a["solve0_fused"]), "DIFFER: %s" % bad if bad else "all equal bits")
            forms = {f: int(a[f]) for f in a.files if f.endswith("_form")}   # 18 step cells: fused 1, pair 0, starts 1
            wrong = [f for f, v in forms.items() if v != (0 if f.endswith("_pair_form") else 1)]
            differ += wrong
            print(tag, "buffer_loads", buf, "LM step cells (lm / dogleg x none / prior / mask x fused / pair / starts, whole result, 7 trace arrays):",
                  "%d, forms %s" % (len(forms), "NOT AS INTENDED: %s" % wrong if wrong else "as intended"))
    sys.exit(1 if differ else 0)
libs = sys.argv[1:3]
res = {l: [] for l in libs}
for r in range(3):
    for l in libs:
        o = subprocess.run(["timeout", "-k", "10", "300", sys.executable, '-c', CHILD, os.path.abspath(l)], capture_output=True, text=True)
        if o.returncode != 0:
            print(l, 'FAILED', o.stderr[-1500:]); sys.exit(1)
        res[l].append(json.loads(o.stdout.strip().splitlines()[-1]))
for l in libs:   # median of the three alternating runs, then (min, max)
    print(os.path.basename(l), {k: round(sorted(x[k] for x in res[l])[1], 4) for k in res[l][0]},
          "min/max", {k: (round(min(x[k] for x in res[l]), 4), round(max(x[k] for x in res[l]), 4)) for k in res[l][0]})
