"""The two item orders of the pose-batched work list (tuning key "poses_order": 0 = an XCD walks the poses of a row back to
back, 1 = the rows of a pose), alternating processes: kernel time per evaluation (evaluation launches only, one event pair)
and per evaluation with the folds, on C2 fp64 at K = 2000 and K = 20 and on C5 fp32 at K = 8.
usage: python scripts/ab_poses_order.py [rounds=3]"""
import json
import subprocess
import sys

CHILD = r'''
import sys, json
sys.path.insert(0, '.')
import torch; torch.cuda.init()
from edge_alignment_amd import capi, synth
import bench
order = int(sys.argv[1])
out = {}
def run(name, cfg, dtype, loss, K):
    P = capi.Problem(*cfg["K"], dtype=dtype); P.set_points(cfg["xyz"]); P.set_dt_grid(cfg["grid"]); P.set_loss(*loss)
    B = capi.Batch([P])
    B.set_tuning("poses_order", order)
    Q, T = bench.step_poses(K, 1000)
    B.set_poses(Q, T)
    ev = min(B.bench_resident_poses(5, evaluations_only=True)[0] for _ in range(4))
    al = min(B.bench_resident_poses(5)[0] for _ in range(4))
    out[name] = [round(ev * 1e3 / K, 4), round(al * 1e3 / K, 4)]
    B.close(); P.close()
c2 = synth.config_c2_twin(seed=2, n_points=50000)
run("c2_f64_K2000", c2, capi.EA_F64, (capi.LOSS_CAUCHY, 1.0), 2000)
run("c2_f64_K20", c2, capi.EA_F64, (capi.LOSS_CAUCHY, 1.0), 20)
run("c5_f32_K8", synth.config_c5(), capi.EA_F32, (capi.LOSS_TRIVIAL, 1.0), 8)
print(json.dumps(out))
'''
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 3
res = {0: [], 1: []}
for r in range(rounds):
    for order in (0, 1):
        o = subprocess.run(["timeout", "-k", "10", "180", sys.executable, "-c", CHILD, str(order)], capture_output=True, text=True)
        if o.returncode != 0:
            print("order", order, "FAILED", o.returncode, o.stderr[-1500:]); sys.exit(1)
        res[order].append(json.loads(o.stdout.strip().splitlines()[-1]))
print("us per evaluation [evaluation launches only, with folds], every round")
for order in (0, 1):
    print("order", order, {k: [x[k] for x in res[order]] for k in res[order][0]})
