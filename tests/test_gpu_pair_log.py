"""One logarithm per lane in the fp64 two-point launches (loss_point / cost_point of ea_kernels.hip, pl_log_pair of
csrc/ea_pair_log.h) on the 120 x 160 synthetic problem of test_gpu_poses_flat.py: point counts at which a lane has no second
point (1, 255, 256, 257), a pair straddles the end of a chunk (511, 513, 1026) or fills it (2, 512); ea_batch_eval,
ea_batch_eval_poses (K = 3; pose 1 moves points into the z guard), ea_batch_cost_poses and one solve; the Cauchy loss at
a = 0.7, at a = 1e6 (x = r^2 / a^2 ~ 1e-13: the regime in which the product of the two sums loses what the error term
returns -- without it the cost is off by ~1e-7) and at a = 1e-140 (x ~ 1e278: the product of the two sums itself would
overflow), and the Huber and trivial losses (the unpaired text).

Bars: against the CPU oracle, cost 1e-11 relative (the bar of test_gpu_parity.py) and n_invalid exactly; against the same
batch at one point per lane (code the change does not touch) cost, JtJ and Jtr 1e-12 relative (the between-shapes bar of
test_gpu_poses_flat.py / test_gpu_parity.py) and n_invalid exactly.  A weighted problem takes the unpaired path and meets its
own one-point-per-lane result at 1e-12 as well."""
import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 255, 256, 257, 511, 512, 513, 1026)
LOSSES = [("cauchy_0.7", (1, 0.7)), ("cauchy_1e6", (1, 1e6)), ("cauchy_1e-140", (1, 1e-140)), ("huber", (2, 0.05)), ("trivial", (0, 1.0))]
TOL_ORACLE, TOL_SHAPE = 1e-11, 1e-12


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


@pytest.fixture(scope="module")
def base():
    pr = synth.make_problem(120, 160, 9000, 40, 1, 130.0, 130.0, 79.5, 59.5,
                            planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)),
                            planted_t=(0.01, -0.005, 0.02), normalize=True)
    rng = np.random.default_rng(61)
    pr["clouds"] = [pr["xyz"][rng.choice(9000, n, replace=False)].reshape(-1, 3) for n in SIZES]
    n = len(SIZES)
    q = np.zeros((3, n, 4)); t = np.zeros((3, n, 3))
    for k in range(3):
        for i in range(n):
            q[k, i] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0.0, 1.5)))
            t[k, i] = rng.uniform(-0.03, 0.03, size=3)
    # pose 1: the depth of the cloud's LAST point (the one a lane may hold alone) to zero -- it and its neighbours in depth
    # are inside the z guard
    for i, X in enumerate(pr["clouds"]):
        q[1, i] = [1.0, 0, 0, 0]; t[1, i] = [0.0, 0.0, -float(X[-1, 2])]
    pr["q"], pr["t"] = q, t
    return pr


def _batch(hip, base, loss, weights=None):
    probs = []
    for i, X in enumerate(base["clouds"]):
        P = hip.Problem(*base["K"], dtype=hip.EA_F64)
        P.set_points(X); P.set_dt_grid(base["grid"]); P.set_loss(*loss)
        if weights is not None:
            P.set_weights(weights[i])
        probs.append(P)
    return hip.Batch(probs), probs


def _all_paths(B, q, t):
    """eval at pose 0, eval_poses and cost_poses at the three poses"""
    return dict(eval=B.eval(q[0], t[0]), poses=B.eval_poses(q, t), cost=B.cost_poses(q, t))


def _against_one_point_per_lane(two, one, where):
    """every result of every path, per problem and per pose (each on its own scale)"""
    for i, n in enumerate(SIZES):
        pairs = [("eval", f, two["eval"][f][i], one["eval"][f][i]) for f in ("cost", "JtJ", "Jtr")]
        for k in range(two["poses"]["cost"].shape[0]):
            pairs += [("poses[%d]" % k, f, two["poses"][f][k, i], one["poses"][f][k, i]) for f in ("cost", "JtJ", "Jtr")]
            pairs.append(("cost_poses[%d]" % k, "cost", two["cost"]["cost"][k, i], one["cost"]["cost"][k, i]))
        for path, f, a, b in pairs:
            d = _rel(a, b)
            print(where, path, f, "n", n, "two points per lane against one:", d)
            assert d <= TOL_SHAPE, (where, path, f, n, d)
    for path in ("eval", "poses", "cost"):
        assert np.array_equal(two[path]["n_invalid"], one[path]["n_invalid"]), (where, path)


@pytest.mark.parametrize("name,loss", LOSSES)
def test_two_points_per_lane_against_oracle_and_one_point_per_lane(hip, oracle, base, name, loss):
    q, t = base["q"], base["t"]
    O = oracle.OracleProblem(base["grid"], *base["K"], loss=loss[0], loss_a=loss[1])
    B, probs = _batch(hip, base, loss)
    try:
        got = {}
        for ppt in (2, 1):
            B.set_tuning("points_per_thread", ppt)
            got[ppt] = _all_paths(B, q, t)
            assert B.info("points_per_thread") == ppt and B.info("poses_points_per_thread") == ppt
        two, one = got[2], got[1]
        for i, (n, X) in enumerate(zip(SIZES, base["clouds"])):
            for k in range(3):
                e = O.eval(X, q[k, i], t[k, i])
                for path, c, bad in (("poses", two["poses"]["cost"][k, i], two["poses"]["n_invalid"][k, i]),
                                     ("cost_poses", two["cost"]["cost"][k, i], two["cost"]["n_invalid"][k, i])) + \
                        ((("eval", two["eval"]["cost"][i], two["eval"]["n_invalid"][i]),) if k == 0 else ()):
                    d = abs(c - e["cost"]) / max(abs(e["cost"]), 1e-300)
                    print(name, path, "n", n, "pose", k, "cost", c, "oracle", e["cost"], "rel", d, "invalid", bad, e["n_invalid"])
                    assert bad == e["n_invalid"], (name, path, n, k)
                    assert d <= TOL_ORACLE, (name, path, n, k, d)
            assert two["poses"]["n_invalid"][1, i] > 0 and two["cost"]["n_invalid"][1, i] > 0   # (the pose inside the z guard)
        _against_one_point_per_lane(two, one, name)
    finally:
        B.close()
        for P in probs:
            P.close()


def test_weighted_problem_keeps_the_unpaired_path(hip, base):
    rng = np.random.default_rng(67)
    weights = [rng.uniform(0.1, 1.0, size=n) for n in SIZES]
    B, probs = _batch(hip, base, (1, 0.7), weights)
    try:
        got = {}
        for ppt in (2, 1):
            B.set_tuning("points_per_thread", ppt)
            got[ppt] = _all_paths(B, base["q"], base["t"])
        _against_one_point_per_lane(got[2], got[1], "weighted")
    finally:
        B.close()
        for P in probs:
            P.close()


def test_one_solve_at_two_points_per_lane(hip, oracle, base):
    """the fused iteration and the step pair share fused_chunk's text: three iterations of a solve of the 1026-point problem
    (the full solve ends at the planted pose, where the cost is exactly zero and says nothing) end where three iterations of
    the CPU oracle end (smoke's bar, 1e-9), every iteration's cost is the oracle's to 1e-7 (the trace bar of
    test_gpu_parity.py), and the final cost is the oracle's cost AT THAT POSE to 1e-11"""
    X = base["clouds"][-1]
    q0, t0 = np.array([1.0, 0, 0, 0]), np.zeros(3)
    O = oracle.OracleProblem(base["grid"], *base["K"], loss=1, loss_a=0.7)
    qo, to, so = O.solve(X, q0, t0, max_num_iterations=3)
    P = hip.Problem(*base["K"], dtype=hip.EA_F64)
    P.set_points(X); P.set_dt_grid(base["grid"]); P.set_loss(1, 0.7)
    B = hip.Batch([P])
    try:
        B.set_tuning("points_per_thread", 2)
        q, t, ss = B.solve(q0, t0, max_num_iterations=3)
        assert B.info("points_per_thread") == 2
        s = ss[0]
        assert s["num_iterations"] == so["num_iterations"] == 3 and s["why"] == so["why"], (s["why"], so["why"])
        assert synth.rotation_angle_between(q[0], qo) < 1e-9 and np.linalg.norm(t[0] - to) < 1e-9
        assert s["it_cost"] == pytest.approx(so["it_cost"], rel=1e-7)
        e = O.eval(X, q[0], t[0])
        print("solve: costs", s["it_cost"], "final", s["final_cost"], "oracle at that pose", e["cost"], "difference", s["final_cost"] - e["cost"])
        assert e["cost"] > 0 and e["n_invalid"] == 0 and abs(s["final_cost"] - e["cost"]) <= TOL_ORACLE * e["cost"]
    finally:
        B.close(); P.close()
