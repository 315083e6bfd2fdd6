"""Two builds of the library on one box, alternating processes of bench.py itself (EA_HIP_LIB selects the build): every
`value` of the headline, the median and the spread (max - min) per build, and whether every run of B beats A's best run.
With --full, --full-runs more alternating pairs of `bench.py --full` runs at the end: of the last pair the kernel time per
evaluation launch, eval_poses_call_ms and the k_poses figures of the other workloads; of every pair the trust-region figures
(LM iterations per second at 1e5 points in the fused, pair and fp32 forms, the C4 batch's solve_ms) -- per build every value,
median, min and max, and whether B's median lies inside A's min .. max.  With --dump DIR, a pair of --dump-outputs runs
compared in max-norm.
usage: python scripts/ab_two_builds_bench.py libA.so libB.so [--steps 2000 --warmup 200 --runs 5 --full --full-runs 5 --dump DIR]
Every child runs under its own time limit; the first one that fails ends the script."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# figure -> the keys that lead to it in bench.py's result line (each looked up at any depth below the one before)
LM_KEYS = {"lm_iters_per_s_at_1e5_pts": ("lm_iters_per_s_at_1e5_pts",),
           "lm_iters_per_s_at_1e5_pts_pair_form": ("lm_iters_per_s_at_1e5_pts_pair_form", "iters_per_s"),
           "lm_fp32_at_1e5_pts_iters_per_s": ("lm_fp32_at_1e5_pts", "iters_per_s"),
           "c4_batch_solve_ms": ("c4_batch_32_pairs_per_gpu", "solve_ms")}


def bench(lib, extra, limit):
    env = dict(os.environ, EA_HIP_LIB=os.path.abspath(lib))
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + extra
    o = subprocess.run(cmd, capture_output=True, text=True, env=env, cwd=ROOT)
    if o.returncode != 0:
        print(lib, "FAILED", o.returncode, o.stdout[-800:], o.stderr[-1500:])
        sys.exit(1)
    return json.loads(o.stdout.strip().splitlines()[-1])


def find(d, key):
    if isinstance(d, dict):
        if key in d:
            return d[key]
        for v in d.values():
            r = find(v, key)
            if r is not None:
                return r
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs=2)
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--workload", default="c2")
    ap.add_argument("--full", action="store_true")
    ap.add_argument("--full-runs", type=int, default=1, help="with --full: so many alternating pairs of `bench.py --full` runs")
    ap.add_argument("--dump", default=None)
    a = ap.parse_args()
    shape = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--workload", a.workload]
    vals = {l: [] for l in a.libs}
    for _ in range(a.runs):
        for l in a.libs:
            vals[l].append(bench(l, shape, 120)["value"])
    out = {"steps": a.steps, "warmup": a.warmup, "workload": a.workload}
    for tag, l in zip("AB", a.libs):
        v = sorted(vals[l])
        out[tag] = {"lib": os.path.basename(l), "values": vals[l], "median": v[len(v) // 2], "spread": v[-1] - v[0]}
    if a.runs:
        out["every_B_run_beats_best_A"] = min(vals[a.libs[1]]) > max(vals[a.libs[0]])
        out["B_median_over_A_median"] = out["B"]["median"] / out["A"]["median"]
        out["B_median_inside_A_min_max"] = {"value": min(vals[a.libs[0]]) <= out["B"]["median"] <= max(vals[a.libs[0]])}
    if a.full:
        lm = {l: {k: [] for k in LM_KEYS} for l in a.libs}   # the trust-region solves only `bench.py --full` times
        for _ in range(a.full_runs):
            for tag, l in zip("AB", a.libs):
                d = bench(l, shape + ["--full", "--no-cpu-baseline"], 600)
                out[tag]["full"] = {"value": d["value"], "kernel_ms": find(d, "kernel_ms"), "eval_poses_call_ms": find(d, "eval_poses_call_ms"),
                                    "evaluation_launches": find(d, "evaluation_launches_in_timed_region"),
                                    "k_poses": {k: v.get("k_poses") for k, v in (find(d, "other_workloads") or {}).items() if isinstance(v, dict)}}
                for k, path in LM_KEYS.items():
                    x = d
                    for step in path:
                        x = find(x, step) if x is not None else None
                    if isinstance(x, (int, float)):
                        lm[l][k].append(x)
        for tag, l in zip("AB", a.libs):
            out[tag]["lm"] = {k: {"values": x, "median": sorted(x)[len(x) // 2], "min": min(x), "max": max(x)} for k, x in lm[l].items() if x}
        # per figure: does B's median lie inside A's own min .. max of this session?
        out.setdefault("B_median_inside_A_min_max", {}).update(
            {k: out["A"]["lm"][k]["min"] <= out["B"]["lm"][k]["median"] <= out["A"]["lm"][k]["max"] for k in out["A"]["lm"] if k in out["B"]["lm"]})
    if a.dump:
        import numpy as np
        dirs = []
        for tag, l in zip("AB", a.libs):
            d = os.path.join(a.dump, "%s_%d" % (tag, a.steps))
            os.makedirs(d, exist_ok=True)
            bench(l, shape + ["--dump-outputs", d], 120)
            dirs.append(d)
        cmp = {}
        for f in sorted(os.listdir(dirs[0])):
            if f.endswith(".npy"):
                x, y = np.load(os.path.join(dirs[0], f)), np.load(os.path.join(dirs[1], f))
                cmp[f] = {"equal": bool(np.array_equal(x, y)),
                          "max_abs_diff_over_max_abs": float(np.abs(x - y).max() / max(np.abs(x).max(), 1e-300))}
        out["dump_outputs_A_vs_B"] = cmp
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
