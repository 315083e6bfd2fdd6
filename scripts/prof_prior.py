"""Cost of a NormalPrior in the solve (profiles/LOG.md, pose priors): LM iterations/s of one fp64 problem of 1e5 points
(config_c2_twin, Cauchy(1)), without a prior and with weak priors on q and t (the prior-free kernels vs the SIDE
instantiations of ea_lm_iter_kernel / ea_lm_step_kernel).  The prior is centred on the start pose with sigmas large enough
that the solve takes the same path; iterations/s = iterations of one solve / best-of-rounds median solve time.  Alternating
rounds, so drift of the box hits both forms alike."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edge_alignment_amd import capi, synth  # noqa: E402


def _solve_us(P, q0, t0, reps=40):
    ts = []
    for _ in range(reps):
        t1 = time.perf_counter()
        _, _, s = P.solve(q0, t0)
        ts.append(time.perf_counter() - t1)
    return float(np.median(ts)) * 1e6, s


def main(rounds=5):
    cfg = synth.config_c2_twin(seed=7, n_points=100000)
    q0, t0 = np.array([1.0, 0, 0, 0]), np.zeros(3)
    P = capi.Problem(*cfg["K"], dtype=capi.EA_F64)
    P.set_points(cfg["xyz"])
    P.set_dt_grid(cfg["grid"])
    P.set_loss(capi.LOSS_CAUCHY, 1.0)
    best = {"none": 1e30, "prior": 1e30}
    iters = {}
    for _ in range(5):
        P.solve(q0, t0)
    for _ in range(rounds):
        for form in ("none", "prior"):
            if form == "prior":
                P.set_normal_prior(0, np.eye(4) / 10.0, q0)
                P.set_normal_prior(1, np.eye(3) / 10.0, t0)
            else:
                P.clear_normal_prior(0)
                P.clear_normal_prior(1)
            us, s = _solve_us(P, q0, t0)
            best[form] = min(best[form], us)
            iters[form] = s["num_iterations"]
    out = {f: {"lm_it_per_s": iters[f] / (best[f] * 1e-6), "solve_us": best[f], "iters": iters[f]} for f in best}
    print(json.dumps(out))
    P.close()


if __name__ == "__main__":
    main()
