"""Wall time of the covariance entry points next to the evaluation they are built on (profiles/LOG.md, covariance):
ea_problem_covariance vs ea_eval on C2 (5e4 points, fp64, Cauchy(1)), ea_batch_covariance vs ea_batch_eval on 32 C2-shaped
pairs, and the tracker's ms per frame on the bundled frames with covariance off and on.  Best of `rounds` medians."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from edge_alignment_amd import capi, synth  # noqa: E402


def _us(fn, reps=200, rounds=5):
    for _ in range(20):
        fn()
    best = 1e30
    for _ in range(rounds):
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        best = min(best, float(np.median(ts)))
    return best * 1e6


def c2_problem(seed):
    cfg = synth.config_c2_twin(seed=seed, n_points=50000)
    P = capi.Problem(*cfg["K"], dtype=capi.EA_F64)
    P.set_points(cfg["xyz"])
    P.set_dt_grid(cfg["grid"])
    P.set_loss(capi.LOSS_CAUCHY, 1.0)
    return P, cfg


def main():
    P, cfg = c2_problem(2)
    q, t, _ = P.solve([1, 0, 0, 0], [0, 0, 0])
    print("C2 ea_eval               %.1f us" % _us(lambda: P.eval(q, t)))
    print("C2 ea_problem_covariance %.1f us" % _us(lambda: P.covariance(q, t)))
    print("C2 ea_problem_covariance %.1f us (apply_loss_function = 0)" % _us(lambda: P.covariance(q, t, apply_loss_function=0)))
    Ps = [c2_problem(100 + i)[0] for i in range(32)]
    B = capi.Batch(Ps)
    qs, ts, _ = B.solve(np.tile([1.0, 0, 0, 0], (32, 1)), np.zeros((32, 3)))
    print("32 x C2 ea_batch_eval       %.1f us" % _us(lambda: B.eval(qs, ts), reps=100))
    print("32 x C2 ea_batch_covariance %.1f us" % _us(lambda: B.covariance(qs, ts), reps=100))
    B.close()
    for p in Ps:
        p.close()
    P.close()

    from oracle import preprocess_np as pp
    G = os.path.join(ROOT, "tests", "golden", "rgbd")
    frames = [(pp.load_rgb_as_bgr(os.path.join(G, "rgb_%d.png" % i)), pp.load_depth_u16(os.path.join(G, "depth_%d.png" % i)))
              for i in range(1, 6)]
    for on in (False, True, False, True):
        T = capi.Tracker(525.0, 525.0, 319.5, 239.5, dtype=capi.EA_F64, loss=(capi.LOSS_CAUCHY, 1.0))
        if on:
            T.set_covariance(True)
        for bgr, dep in frames:
            T.push_frame(bgr, dep)
        best = 1e9
        for _ in range(3):
            t0 = time.perf_counter()
            n = 0
            for rep in range(2):
                for bgr, dep in (frames if rep % 2 == 0 else frames[::-1]):
                    T.push_frame(bgr, dep)
                    n += 1
            best = min(best, (time.perf_counter() - t0) / n)
        print("tracker push_frame %.3f ms per frame (covariance %s, pageable frames)" % (best * 1e3, "on" if on else "off"))
        T.close()


if __name__ == "__main__":
    main()
