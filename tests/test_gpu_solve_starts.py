"""ea_batch_solve_starts / ea_solve_starts: K trust-region solves of every problem from K starting poses, in lock-step on the
device -- K independent ceres::Solve calls on the same problem from K initial values.

Against the CPU oracle's solve from each start (the bars test_gpu_parity.py uses for solves: angle < 1e-7, |dt| < 1e-7 in
fp64; 1e-4 rad / 1e-3 m of the planted pose in fp32), against ea_batch_eval_poses (it_cost[0] bit for bit: the same pose
kernel, rows and fold order; final_cost to 1e-12 relative, the bound for one sum reached by two routes), and against itself
bit for bit: a start's pose, iteration count, termination and whole cost trace must not depend on K, on the other starts, on
the split over launches or on the order of the starts.

The problem is the 120 x 160 synthetic pair of test_gpu_eval_poses.py with a Cauchy loss; starts are drawn around the
identity with scale s (s = 4: up to 6 degrees / 12 cm, where one start in twelve misses the basin on the oracle)."""
import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

SIZES = (9000, 257, 4097)


@pytest.fixture(scope="module")
def base():
    return synth.make_problem(120, 160, 9000, 40, 1, 130.0, 130.0, 79.5, 59.5,
                              planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)),
                              planted_t=(0.01, -0.005, 0.02), normalize=True)


def _starts(s, K=12, seed=5):
    rng = np.random.default_rng(seed)
    q = np.zeros((K, 4)); t = np.zeros((K, 3))
    for k in range(K):
        q[k] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(s * rng.uniform(0, 1.5)))
        t[k] = s * rng.uniform(-0.03, 0.03, 3)
    q[0] = [1.0, 0, 0, 0]; t[0] = 0.0
    return q, t


def _problem(hip, base, X, dtype=None):
    P = hip.Problem(*base["K"], dtype=hip.EA_F64 if dtype is None else dtype)
    P.set_points(X); P.set_dt_grid(base["grid"]); P.set_loss(hip.LOSS_CAUCHY, 0.7)
    return P


def _same(a, b):
    """two solves of one start: pose, iterations, termination and the whole cost trace, bit for bit"""
    (qa, ta, sa), (qb, tb, sb) = a, b
    return (np.array_equal(qa, qb) and np.array_equal(ta, tb) and sa["num_iterations"] == sb["num_iterations"] and
            sa["why"] == sb["why"] and sa["termination"] == sb["termination"] and np.array_equal(sa["it_cost"], sb["it_cost"]))


def _within(q, t, q_ref, t_ref, ang, dist):
    return synth.rotation_angle_between(q, q_ref) < ang and np.linalg.norm(np.asarray(t) - np.asarray(t_ref)) < dist


@pytest.fixture(scope="module")
def twelve(hip, base):
    """the 12 starts at s = 4 on the first 2500 points, solved in one call: (P, B, X, q0, t0, q, t, summaries, best)"""
    X = base["xyz"][:2500]
    P = _problem(hip, base, X)
    B = hip.Batch([P])
    q0, t0 = _starts(4.0)
    q, t, s, best = P.solve_starts(q0, t0)
    yield dict(P=P, B=B, X=X, q0=q0, t0=t0, q=q, t=t, s=s, best=best)
    B.close(); P.close()


def test_every_start_follows_the_oracle_and_the_best_is_the_planted_pose(hip, oracle, base, twelve):
    """Every start whose oracle solve ends in CONVERGENCE must converge on the device to the oracle's pose (1e-7 / 1e-7); at
    most 2 of the 12 may be left out.  On the oracle all twelve end in CONVERGENCE (iterations 9 .. 43): eleven at the planted
    pose, start 10 on function_tolerance after 26 iterations in a side minimum at cost 15.6 -- it is compared like the others."""
    w = twelve
    O = oracle.OracleProblem(base["grid"], *base["K"], loss=hip.LOSS_CAUCHY, loss_a=0.7)
    left_out = []
    for k in range(12):
        qo, to, so = O.solve(w["X"], w["q0"][k], w["t0"][k])
        if so["termination"] != 0:
            left_out.append(k)
            continue
        print("start", k, "oracle its", so["num_iterations"], "device its", w["s"][k]["num_iterations"], "angle",
              synth.rotation_angle_between(w["q"][k], qo), "dt", np.linalg.norm(w["t"][k] - to))
        assert w["s"][k]["termination"] == hip.CONVERGENCE, k
        assert _within(w["q"][k], w["t"][k], qo, to, 1e-7, 1e-7), k
    assert len(left_out) <= 2, left_out
    assert w["best"] not in left_out and 0 <= w["best"] < 12
    assert _within(w["q"][w["best"]], w["t"][w["best"]], base["q_true"], base["t_true"], 1e-7, 1e-7)
    at_start = w["B"].eval_poses(w["q0"][:, None, :], w["t0"][:, None, :])["cost"][:, 0]
    at_end = w["B"].eval_poses(w["q"][:, None, :], w["t"][:, None, :])["cost"][:, 0]
    for k in range(12):
        assert w["s"][k]["it_cost"][0] == at_start[k] == w["s"][k]["initial_cost"], k
        assert abs(w["s"][k]["final_cost"] - at_end[k]) <= 1e-12 * abs(at_end[k]), k
    ok = [k for k in range(12) if w["s"][k]["termination"] != hip.FAILURE]
    assert w["best"] == min(ok, key=lambda k: (w["s"][k]["final_cost"], k))


def test_a_start_does_not_depend_on_its_company(hip, base, twelve):
    w = twelve
    ref = [(w["q"][k], w["t"][k], w["s"][k]) for k in range(12)]
    its = sorted(s["num_iterations"] for _, _, s in ref)
    assert its[0] < its[-1]          # the starts end at different iterations: compaction happens
    for k in range(12):              # each start alone
        q, t, s, best = w["P"].solve_starts(w["q0"][k:k + 1], w["t0"][k:k + 1])
        assert _same((q[0], t[0], s[0]), ref[k]), k
        assert best == (0 if s[0]["termination"] != hip.FAILURE else -1)
    B = w["B"]
    for g in (1, 3, 0):              # any split of the live list over launch pairs
        B.set_tuning("poses_per_launch", g)
        q, t, s, best = B.solve_starts(w["q0"][:, None, :], w["t0"][:, None, :])
        assert B.info("starts_form") == 1 and B.info("starts_launches") >= max(x["num_iterations"] for x in w["s"])
        for k in range(12):
            assert _same((q[k, 0], t[k, 0], s[k][0]), ref[k]), (g, k)
        assert best[0] == w["best"]
    perm = np.random.default_rng(7).permutation(12)
    q, t, s, best = B.solve_starts(w["q0"][perm][:, None, :], w["t0"][perm][:, None, :], iterations_per_sync=4)
    for j, k in enumerate(perm):
        assert _same((q[j, 0], t[j, 0], s[j][0]), ref[k]), (j, k)
    # several starts reach the same final cost bit for bit (0.0 at the planted pose): a tie goes to the lowest index OF THE CALL
    assert best[0] == min(range(12), key=lambda j: (s[j][0]["final_cost"], j))
    assert s[best[0]][0]["final_cost"] == w["s"][w["best"]]["final_cost"]
    # without summaries: the same poses, the same choice
    q2, t2, none, best2 = B.solve_starts(w["q0"][perm][:, None, :], w["t0"][perm][:, None, :], summaries=False)
    assert none is None and np.array_equal(q2, q) and np.array_equal(t2, t) and np.array_equal(best2, best)


def test_resident_poses_survive(hip, base, twelve):
    B = twelve["B"]
    q, t = _starts(1.0, K=5, seed=11)
    first = B.eval_poses(q[:, None, :], t[:, None, :])
    B.solve_starts(twelve["q0"][:3, None, :], twelve["t0"][:3, None, :])
    again = B.eval_resident_poses()
    assert all(np.array_equal(again[f], first[f]) for f in ("cost", "JtJ", "Jtr", "n_invalid"))


def test_ragged_batch_equals_single_problem_calls(hip, base):
    rng = np.random.default_rng(23)
    clouds = [base["xyz"][rng.choice(9000, n, replace=False)] for n in SIZES]
    probs = [_problem(hip, base, X) for X in clouds]
    empty = _problem(hip, base, np.zeros((0, 3)))
    B, B4 = hip.Batch(probs), hip.Batch(probs + [empty])
    try:
        for K in (1, 2, 3, 8):
            q0 = np.zeros((K, 4, 4)); t0 = np.zeros((K, 4, 3))
            for i in range(4):
                q0[:, i], t0[:, i] = _starts(1.0, K=K, seed=40 + 10 * K + i)
            q, t, s, best = B.solve_starts(q0[:, :3], t0[:, :3])
            assert best.shape == (3,) and B.info("starts_form") == 1
            for i in range(3):
                for k in range(K):
                    q1, t1, s1, _ = probs[i].solve_starts(q0[k:k + 1, i], t0[k:k + 1, i])
                    assert _same((q[k, i], t[k, i], s[k][i]), (q1[0], t1[0], s1[0])), (K, k, i)
                ok = [k for k in range(K) if s[k][i]["termination"] != hip.FAILURE]
                assert best[i] == min(ok, key=lambda k: (s[k][i]["final_cost"], k))
            # a fourth problem without a single point ends at once (zero gradient) and does not disturb the others
            q4, t4, s4, best4 = B4.solve_starts(q0, t0)
            assert best4.shape == (4,) and np.array_equal(best4[:3], best)
            for k in range(K):
                for i in range(3):
                    assert _same((q4[k, i], t4[k, i], s4[k][i]), (q[k, i], t[k, i], s[k][i])), (K, k, i)
                assert s4[k][3]["why"] == "gradient_tolerance" and s4[k][3]["num_iterations"] == 0
                assert np.array_equal(q4[k, 3], q0[k, 3]) and np.array_equal(t4[k, 3], t0[k, 3])
    finally:
        B.close(); B4.close()
        for P in probs + [empty]:
            P.close()


def test_ends_together_and_ends_at_once(hip, base, twelve):
    w = twelve
    q, t, s, best = w["P"].solve_starts(w["q0"], w["t0"], max_num_iterations=3)
    for k in range(12):
        assert s[k]["termination"] == hip.NO_CONVERGENCE and s[k]["why"] == "max_iterations" and s[k]["num_iterations"] <= 3, k
    assert 0 <= best < 12
    # a start that puts the cloud's first point on the camera plane fails its first evaluation, alone
    q0, t0 = w["q0"][:4].copy(), w["t0"][:4].copy()
    without = w["P"].solve_starts(np.delete(q0, 2, axis=0), np.delete(t0, 2, axis=0))
    q0[2] = [1.0, 0, 0, 0]; t0[2] = [0.0, 0.0, -w["X"][0, 2]]
    q, t, s, best = w["P"].solve_starts(q0, t0)
    assert s[2]["termination"] == hip.FAILURE and s[2]["why"] == "initial_eval_failed" and s[2]["final_cost"] == -1.0
    assert np.array_equal(q[2], q0[2]) and np.array_equal(t[2], t0[2])
    for j, k in enumerate((0, 1, 3)):
        assert _same((q[k], t[k], s[k]), (without[0][j], without[1][j], without[2][j])), k
    assert best != 2 and best == (0, 1, 3)[without[3]]
    q, t, s, best = w["P"].solve_starts(q0[2:3], t0[2:3])   # nothing but the failing start: no best
    assert best == -1 and s[0]["why"] == "initial_eval_failed"


def test_priors_constant_coordinates_and_dogleg(hip, oracle, base):
    X = base["xyz"][:2500]
    A, Bp = _problem(hip, base, X), _problem(hip, base, base["xyz"][2500:5000])
    A.set_normal_prior(1, 5.0 * np.eye(3), np.asarray(base["t_true"], dtype=np.float64))
    A.set_constant_parameters([0, 0, 1, 0, 1, 0])
    both, alone = hip.Batch([A, Bp]), hip.Batch([Bp])
    try:
        q0 = np.zeros((3, 2, 4)); t0 = np.zeros((3, 2, 3))
        for i in range(2):
            q0[:, i], t0[:, i] = _starts(1.0, K=3, seed=70 + i)
        q, t, s, best = both.solve_starts(q0, t0)
        assert both.info("starts_form") == 1
        for k in range(3):
            q1, t1, s1, _ = both.solve_starts(q0[k:k + 1], t0[k:k + 1])
            for i in range(2):
                assert _same((q[k, i], t[k, i], s[k][i]), (q1[0, i], t1[0, i], s1[0][i])), (k, i)
            assert t[k, 0, 1] == t0[k, 0, 1]              # the held translation coordinate: its input bits
            assert s[k][0]["num_iterations"] > 0 and not np.array_equal(t[k, 0], t0[k, 0])
        qa, ta, sa, _ = alone.solve_starts(q0[:, 1:], t0[:, 1:])   # the problem without prior or mask: as in a batch without side table
        for k in range(3):
            assert _same((q[k, 1], t[k, 1], s[k][1]), (qa[k, 0], ta[k, 0], sa[k][0])), k
        # dogleg, against the oracle's dogleg from the same starts
        O = oracle.OracleProblem(base["grid"], *base["K"], loss=hip.LOSS_CAUCHY, loss_a=0.7)
        qd, td, sd, _ = alone.solve_starts(q0[:, 1:], t0[:, 1:], strategy=hip.STRATEGY_DOGLEG)
        compared = 0
        for k in range(3):
            qo, to, so = O.solve(base["xyz"][2500:5000], q0[k, 1], t0[k, 1], strategy=oracle.STRATEGY_DOGLEG)
            if so["termination"] != 0:
                continue
            compared += 1
            assert sd[k][0]["termination"] == hip.CONVERGENCE, k
            assert _within(qd[k, 0], td[k, 0], qo, to, 1e-7, 1e-7), k
        assert compared >= 2
    finally:
        both.close(); alone.close(); A.close(); Bp.close()


def test_fp32_starts_reach_the_planted_pose(hip, base):
    P = _problem(hip, base, base["xyz"], dtype=hip.EA_F32)
    q0, t0 = _starts(1.0, K=4)
    q, t, s, best = P.solve_starts(q0, t0)
    for k in range(4):
        assert s[k]["termination"] == hip.CONVERGENCE, k
        assert _within(q[k], t[k], base["q_true"], base["t_true"], 1e-4, 1e-3), k
    assert 0 <= best < 4
    P.close()


def test_variant_batches_fall_back_to_one_solve_per_start(hip, base):
    P = _problem(hip, base, base["xyz"][:2500])
    P.set_distortion(0.02, -0.01, 0.001, -0.0005, 0.003)
    B = hip.Batch([P])
    q0, t0 = _starts(1.0, K=3)
    q, t, s, best = B.solve_starts(q0[:, None, :], t0[:, None, :])
    assert B.info("starts_form") == 0
    for k in range(3):
        q1, t1, s1 = B.solve(q0[k], t0[k])
        assert _same((q[k, 0], t[k, 0], s[k][0]), (q1[0], t1[0], s1[0])), k
    ok = [k for k in range(3) if s[k][0]["termination"] != hip.FAILURE]
    assert best[0] == min(ok, key=lambda k: (s[k][0]["final_cost"], k))
    B.close(); P.close()


def test_deadline_returns_an_error_and_the_batch_recovers(hip, base, twelve):
    B = twelve["B"]
    q0, t0 = twelve["q0"][:3, None, :], twelve["t0"][:3, None, :]
    q_ref, t_ref, s_ref = B.solve(q0[1], t0[1])
    B.set_tuning("test_stall_ms", 300)
    with pytest.raises(hip.EAError) as ei:
        B.solve_starts(q0, t0, solve_timeout_ms=30.0)
    assert ei.value.code == hip.EA_ERR_HIP and "deadline" in str(ei.value)
    B.set_tuning("test_stall_ms", 0)
    q, t, s = B.solve(q0[1], t0[1])                  # drains the stalled launches first
    assert _same((q, t, s[0]), (q_ref, t_ref, s_ref[0]))
    q, t, s, best = B.solve_starts(q0, t0)           # and the multi-start call is itself again
    for k in range(3):
        assert _same((q[k, 0], t[k, 0], s[k][0]), (twelve["q"][k], twelve["t"][k], twelve["s"][k])), k
