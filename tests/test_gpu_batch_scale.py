"""The pose-batched family at production-scale geometry: thousands of problems (batch M: 2 049 problems of 1 .. 512 points on the
60 x 80 pair of test_gpu_poses_lanes.py, one row each), thousands of rows (batch R: problems of 1 000, 1 040 and 8 rows of 512
points, a fourth of one point for the 2 049th row), the automatic one-pose-per-lane threshold at K = 1 024 and a batch solve of
600 problems.  tests/scale_cases.py draws the point sets once per module.

The host rules of ea_capi.hip are asserted through Batch.info before a number is compared:
  rows 2 048: with "poses_lane_per_pose" = 1 the lanes kernel runs (one group of 64 poses just fits 64 MB of rows:
              2 x 64 x 2 048 x 256 B) and G = 64, a whole group smaller than K = 130: launches of 64, 64 and 2 poses;
  rows 2 049: the same request runs the lanes-are-points kernel (kposes_lanes) with
              G = min(ceil(32768 / rows), 131072 / rows) = min(16, 63) = 16: nine launches of 15, 15, .. 10 poses (an even split).

Bars, all from the suite: against ea_batch_eval at the same pose 1e-13 fp64 / 2e-6 fp32 of the largest entry
(test_gpu_poses_flat.py), n_invalid equal; against the CPU oracle 1e-11 (test_gpu_poses_exchange.py; an all-zero reference,
a failed one-point problem, compared absolutely as _within_bars does); one pose per lane against key 0 by _within_bars of
test_gpu_poses_lanes.py (cost 1e-13, JtJ / Jtr 1e-12 per result); ea_batch_cost_poses against ea_batch_eval_poses' cost 1e-12
per result (test_gpu_cost_poses.py); any split over launches and either item order: the same bits.  The batch solve: bit for
bit against each problem's own batch of one and its Problem.solve at one point per lane, and against the oracle by the
assertions of test_gpu_lm_random.py.  The bar against ea_batch_eval is taken of the largest entry over all problems at a pose,
as test_gpu_poses_flat.py takes it: poses 100 and 129 put points of every third problem next to the z guard, where entries
are large; pose 0 has no planted failure, so that there the bar is scaled by an ordinary problem.

Measured on an MI355X, worst over the cases:
  against ea_batch_eval   M 5.4e-14 (in Jtr, at poses 100 and 129), R 3.6e-16, with the prior 5.3e-14, fp32 M 1.4e-7;
  against the oracle      M 3.4e-13, R 1.6e-12 (half a million terms summed one after the other on the CPU);
  one pose per lane against key 0   cost / JtJ / Jtr 1.0e-15 / 1.4e-15 / 1.9e-15 (M2048), 4.0e-16 / 4.7e-16 / 3.8e-16 (R2048),
                          8.2e-16 / 1.0e-15 / 1.0e-15 (K = 1 024, automatic);
  ea_batch_cost_poses against ea_batch_eval_poses   4.8e-16;
  the 600-problem solve   cost traces within 3.5e-11 of the oracle's while live, iterations and accept patterns equal.
The 13 cases take 5 s, 2.5 s of it the 2 053 problems of the module's fixture."""
import numpy as np
import pytest

import scale_cases as sc
from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

FIELDS = ("cost", "JtJ", "Jtr", "n_invalid")
K = 130
FLAT_G_2049 = 16     # min(ceil(32768 / 2049), 131072 // 2049) = min(16, 63)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _problem(hip, pair, X, dtype=None):
    P = hip.Problem(*pair["K"], dtype=hip.EA_F64 if dtype is None else dtype)
    P.set_points(X); P.set_dt_grid(pair["grid"]); P.set_loss(hip.LOSS_CAUCHY, 0.7)
    return P


def _same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in FIELDS)


@pytest.fixture(scope="module")
def batches(hip):
    """M2048, M2049, R2048, R2049 -> dict(B, clouds, rows, q, t); the two M batches and the two R batches share their problems"""
    pair = sc.lanes_base()
    mc, rc = sc.m_clouds(), sc.r_clouds()
    assert sum(len(X) for X in rc) == 512 * 2048 + 1
    mp = [_problem(hip, pair, X) for X in mc]
    rp = [_problem(hip, pair, X) for X in rc]
    out = {}
    for name, probs, clouds, rows, seed in (("M2048", mp[:2048], mc[:2048], 2048, 201), ("M2049", mp, mc, 2049, 202),
                                            ("R2048", rp[:3], rc[:3], 2048, 203), ("R2049", rp, rc, 2049, 204)):
        q, t = sc.scale_poses(clouds, seed, K)
        out[name] = dict(B=hip.Batch(probs), clouds=clouds, rows=rows, q=q, t=t, pair=pair, probs=probs)
    yield out
    for w in out.values():
        w["B"].close()
    for P in mp + rp:
        P.close()


def _geometry(B, rows, lanes_asked=1):
    """what the last eval_poses of K poses must report"""
    assert B.info("poses_tiles") == rows
    assert B.info("poses_threads") == 256 and B.info("poses_points_per_thread") == 2
    lanes = int(lanes_asked and rows <= 2048)
    assert B.info("poses_lane_per_pose") == lanes, rows
    assert B.info("poses_per_launch") == (64 if lanes else (32768 + rows - 1) // rows), rows
    return lanes


def _against_eval(B, q, t, got, tol, where):
    worst = (0.0, None, None)
    for k in sc.CHECKED:
        ref = B.eval(q[k], t[k])
        assert np.array_equal(got["n_invalid"][k], ref["n_invalid"]), where + (k,)
        for f in ("cost", "JtJ", "Jtr"):
            worst = max(worst, (_rel(got[f][k], ref[f]), k, f), key=lambda x: x[0])
            assert _rel(got[f][k], ref[f]) <= tol, where + (k, f, _rel(got[f][k], ref[f]))
    return worst


def _against_oracle(oracle, w, got, problems, where, tol=1e-11):
    O = oracle.OracleProblem(w["pair"]["grid"], *w["pair"]["K"], loss=oracle.LOSS_CAUCHY, loss_a=0.7)
    worst = 0.0
    for i in problems:
        for k in sc.CHECKED:
            e = O.eval(w["clouds"][i], w["q"][k, i], w["t"][k, i])
            assert got["n_invalid"][k, i] == e["n_invalid"], where + (k, i)
            for f in ("cost", "JtJ", "Jtr"):
                scale = np.abs(e[f]).max()
                err = np.abs(got[f][k, i] - e[f]).max() / (scale if scale > 0 else 1.0)
                worst = max(worst, err)
                assert err <= tol, where + (k, i, f, err)
    return worst


@pytest.mark.parametrize("name", ["M2048", "M2049", "R2048", "R2049"])
def test_geometry_then_every_problem(hip, oracle, batches, name):
    """the launch geometry through Batch.info, then the three CHECKED poses against ea_batch_eval (every problem) and the
    oracle (16 seeded problems of M, every problem of R), one pose per lane against key 0 at 2 048 rows, ea_batch_cost_poses"""
    w = batches[name]
    B, rows, q, t = w["B"], w["rows"], w["q"], w["t"]
    B.set_tuning("poses_per_launch", 0); B.set_tuning("poses_order", 0)
    B.set_tuning("poses_lane_per_pose", 0)
    old = B.eval_poses(q, t)
    assert _geometry(B, rows, lanes_asked=0) == 0
    B.set_tuning("poses_lane_per_pose", 1)
    new = B.eval_poses(q, t)
    lanes = _geometry(B, rows)
    assert lanes == (rows == 2048) and B.info("poses_per_launch") == (64 if lanes else FLAT_G_2049)
    # (K = 130 in launches of G with the remainder last: 64, 64, 2; or evenly over ceil(130 / 16) = 9 launches: 8 of 15 and one of 10)
    assert -(-K // B.info("poses_per_launch")) == (3 if lanes else 9)
    assert old["n_invalid"][list(sc.CHECKED)].sum() > 0 and (old["n_invalid"][100, 2::5] > 0).all() and not old["n_invalid"][[0, 1]].any()
    if lanes:
        print(name, "worst cost / JtJ / Jtr, one pose per lane against key 0:", sc.within_bars(old, new, name))
    else:
        assert _same(new, old)                            # the request is refused: the same kernel, the same bits
    for key, got in (("key 0", old), ("key 1", new)):
        print(name, key, "worst against ea_batch_eval:", _against_eval(B, q, t, got, 1e-13, (name, key)))
        problems = range(len(w["clouds"])) if name[0] == "R" else np.random.default_rng(5).choice(len(w["clouds"]), 16, replace=False)
        print(name, key, "worst against the oracle:", _against_oracle(oracle, w, got, [int(i) for i in problems], (name, key)))
    cost = B.cost_poses(q, t)
    assert B.info("cost_form") == 1 and np.array_equal(cost["n_invalid"], old["n_invalid"])
    d = np.abs(cost["cost"] - old["cost"])
    assert (d <= 1e-12 * np.abs(old["cost"])).all(), (name, float((d / np.maximum(np.abs(old["cost"]), 1e-300)).max()))
    print(name, "worst cost_poses against eval_poses:", float((d[old["cost"] != 0] / np.abs(old["cost"][old["cost"] != 0])).max()))


@pytest.mark.parametrize("name", ["M2048", "M2049", "R2048", "R2049"])
def test_same_bits_in_any_split_and_order(hip, batches, name):
    w = batches[name]
    B, rows, q, t = w["B"], w["rows"], w["q"], w["t"]
    B.set_tuning("poses_lane_per_pose", 1); B.set_tuning("poses_per_launch", 0); B.set_tuning("poses_order", 0)
    first = B.eval_poses(q, t)
    lanes = _geometry(B, rows)
    full = 64 if lanes else FLAT_G_2049
    try:
        for order in (0, 1):
            B.set_tuning("poses_order", order)
            for g in (7, 64, 0):
                B.set_tuning("poses_per_launch", g)
                got = B.eval_poses(q, t)
                assert B.info("poses_lane_per_pose") == lanes and B.info("poses_per_launch") == (min(g, full) if g else full), (order, g)
                assert _same(got, first), (name, order, g)
    finally:
        B.set_tuning("poses_order", 0); B.set_tuning("poses_per_launch", 0)


def test_a_prior_and_a_held_coordinate_among_thousands(hip, batches):
    """a NormalPrior on problem 1 500 and a held tangent coordinate on problem 2 047 of M: the side table has 2 048 entries"""
    w = batches["M2048"]
    B, q, t, probs = w["B"], w["q"], w["t"], w["probs"]
    B.set_tuning("poses_per_launch", 0); B.set_tuning("poses_order", 0)
    B.set_tuning("poses_lane_per_pose", 0)
    plain = B.eval_poses(q, t)
    probs[1500].set_normal_prior(1, np.diag([3.0, 2.0, 5.0]), [0.01, -0.02, 0.005])
    probs[2047].set_constant_parameters([0, 0, 0, 0, 1, 0])
    try:
        results = []
        for lanes in (0, 1):
            B.set_tuning("poses_lane_per_pose", lanes)
            got = B.eval_poses(q, t)
            assert _geometry(B, 2048, lanes_asked=lanes) == lanes
            print("prior, lanes", lanes, "worst against ea_batch_eval:", _against_eval(B, q, t, got, 1e-13, ("prior", lanes)))
            results.append(got)
        sc.within_bars(results[0], results[1], "prior")
        others = np.arange(2048) != 1500
        assert _same({f: results[0][f][:, others] for f in FIELDS}, {f: plain[f][:, others] for f in FIELDS})
        assert (results[0]["cost"][:, 1500] > plain["cost"][:, 1500]).all()
        assert len({float(c - p) for c, p in zip(results[0]["cost"][:, 1500], plain["cost"][:, 1500])}) > 100   # (each at its own pose)
    finally:
        probs[1500].clear_normal_prior(1)
        probs[2047].set_constant_parameters(None)
    B.set_tuning("poses_lane_per_pose", 0)
    assert _same(B.eval_poses(q, t), plain)


def test_fp32_many_problems(hip):
    """batch M in fp32 (2 049 rows) against ea_batch_eval at 2e-6, the fp32 bar of test_gpu_poses_flat.py"""
    pair, clouds = sc.lanes_base(), sc.m_clouds()
    probs = [_problem(hip, pair, X, dtype=hip.EA_F32) for X in clouds]
    B = hip.Batch(probs)
    try:
        q, t = sc.scale_poses(clouds, 202, K)
        got = B.eval_poses(q, t)
        assert B.info("poses_tiles") == 2049 and B.info("poses_lane_per_pose") == 0 and B.info("poses_per_launch") == FLAT_G_2049
        print("fp32 M2049 worst against ea_batch_eval:", _against_eval(B, q, t, got, 2e-6, ("fp32",)))
    finally:
        B.close()
        for P in probs:
            P.close()


def test_the_automatic_threshold(hip):
    """"poses_lane_per_pose" = -1 on a 3-row batch: K = 1 023 keeps the lanes-are-points kernel, K = 1 024 takes one pose per lane"""
    pair = sc.lanes_base()
    rng = np.random.default_rng(61)
    clouds = [pair["xyz"][rng.choice(1025, n, replace=False)] for n in (513, 129)]
    probs = [_problem(hip, pair, X) for X in clouds]
    B = hip.Batch(probs)
    try:
        q, t = sc.draw_poses(rng, 1024, 2)
        B.set_tuning("poses_lane_per_pose", -1)
        below = B.eval_poses(q[:1023], t[:1023])
        assert B.info("poses_tiles") == 3 and B.info("poses_lane_per_pose") == 0
        auto = B.eval_poses(q, t)
        assert B.info("poses_lane_per_pose") == 1 and B.info("poses_per_launch") == 1024
        B.set_tuning("poses_lane_per_pose", 0)
        old = B.eval_poses(q, t)
        assert B.info("poses_lane_per_pose") == 0
        assert _same({f: old[f][:1023] for f in FIELDS}, below)        # (below the threshold: key 0's bits)
        print("K = 1024 worst cost / JtJ / Jtr against key 0:", sc.within_bars(old, auto, "auto"))
        for k in (0, 1023):
            ref = B.eval(q[k], t[k])
            assert np.array_equal(auto["n_invalid"][k], ref["n_invalid"])
            for f in ("cost", "JtJ", "Jtr"):
                assert _rel(auto[f][k], ref[f]) <= 1e-13, (k, f, _rel(auto[f][k], ref[f]))
    finally:
        B.close()
        for P in probs:
            P.close()


@pytest.fixture(scope="module")
def six_hundred(hip):
    planted = sc.planted_clouds(600, 77)
    base = sc.starts_base()
    probs = [_problem(hip, base, p["xyz"]) for p in planted]
    B = hip.Batch(probs)
    yield dict(B=B, probs=probs, planted=planted, base=base)
    B.close()
    for P in probs:
        P.close()


def _summaries_same(a, b):
    return (all(a[f] == b[f] for f in ("termination", "why", "num_iterations", "num_successful_steps", "num_unsuccessful_steps",
                                        "initial_cost", "final_cost")) and
            all(np.array_equal(a[f], b[f]) for f in ("it_cost", "it_cost_change", "it_gradient_max_norm", "it_step_norm",
                                                     "it_relative_decrease", "it_radius", "it_successful")))


def test_batch_solve_of_600_equals_lone_solves(hip, six_hundred):
    """"points_per_thread" = 1 on the batch: every 16th problem's pose, summary and every trace column, bit for bit, against its
    own batch of one with the same key (Problem has no tuning keys: the same batch-solve path with count = 1, so this is
    independence of the 599 others) and against Problem.solve, the single-problem entry, whose automatic shape for a problem of
    this size is one point per lane"""
    w = six_hundred
    B, n = w["B"], 600
    q0 = np.tile([1.0, 0, 0, 0], (n, 1)); t0 = np.zeros((n, 3))
    B.set_tuning("points_per_thread", 1)
    try:
        q, t, s = B.solve(q0, t0)
        assert B.info("points_per_thread") == 1
        for i in range(0, n, 16):
            lone = hip.Batch([w["probs"][i]])
            try:
                lone.set_tuning("points_per_thread", 1)
                q1, t1, s1 = lone.solve(q0[i], t0[i])
                assert lone.info("points_per_thread") == 1
            finally:
                lone.close()
            assert np.array_equal(q[i], q1[0]) and np.array_equal(t[i], t1[0]) and _summaries_same(s[i], s1[0]), i
            q2, t2, s2 = w["probs"][i].solve(q0[i], t0[i])
            assert np.array_equal(q[i], q2) and np.array_equal(t[i], t2) and _summaries_same(s[i], s2), i
    finally:
        B.set_tuning("points_per_thread", -1)


def test_batch_solve_of_600_follows_the_oracle(hip, oracle, six_hundred):
    """the automatic shape (two points per lane: the batch holds more than 80 000 points); 24 seeded problems by the assertions
    of test_gpu_lm_random.py: same why, iterations and accept pattern, the cost trace within 1e-6 while it is live"""
    w = six_hundred
    B, n = w["B"], 600
    assert sum(len(p["xyz"]) for p in w["planted"]) > 80000
    q0 = np.tile([1.0, 0, 0, 0], (n, 1)); t0 = np.zeros((n, 3))
    q, t, s = B.solve(q0, t0)
    assert B.info("points_per_thread") == 2 and B.info("threads") == 256
    O = oracle.OracleProblem(w["base"]["grid"], *w["base"]["K"], loss=hip.LOSS_CAUCHY, loss_a=0.7)
    worst = 0.0
    for i in np.random.default_rng(9).choice(n, 24, replace=False):
        qo, to, so = O.solve(w["planted"][i]["xyz"], q0[i], t0[i])
        assert s[i]["why"] == so["why"] and s[i]["num_iterations"] == so["num_iterations"], i
        assert list(s[i]["it_successful"]) == list(so["it_successful"]), i
        live = so["it_cost"] > 1e-9 * so["initial_cost"]
        worst = max(worst, float(np.abs(s[i]["it_cost"][live] / so["it_cost"][live] - 1.0).max()))
        assert np.allclose(s[i]["it_cost"][live], so["it_cost"][live], rtol=1e-6, atol=0), i
        if live.all():
            assert synth.rotation_angle_between(q[i], qo) < 1e-6 and np.linalg.norm(t[i] - to) < 1e-6, i
    print("600-problem solve, worst live cost-trace deviation from the oracle:", worst)
