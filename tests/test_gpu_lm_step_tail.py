"""The trust-region step is one text (ea_kernels.hip: lm_state_word / lm_step_park / EA_LM_STEP_LANE0 / lm_step_publish /
EA_LM_STEP_DELIVER) used by ea_lm_step_kernel (the pair form), ea_lm_step_starts_kernel (K starts in lock-step) and the writer
of ea_lm_iter_kernel (one launch per iteration).  This pins, in one place and in the WHOLE result -- pose, termination, counts,
costs and all seven trace arrays --, what used to rest on three copies of that text being the same, and runs the one arm of
the final delivery no other test reaches: a solve past the trace's end (kTrace = 128 rows), where lane 0 copies every row.

The 48 x 64 synthetic problem of test_gpu_item_head.py with Cauchy 0.7; a batch of two problems with 257 and 1 points: problem 0
takes its row range by value and the early point loads (257 points: two chunks and the writer), problem 1 reads groups[p].
LM and dogleg; no side table, a NormalPrior on t, a held-coordinate mask (both on problem 0: problem 1 then rides the side
instantiation with an empty record).

Bars.  Fused form against pair form, a start alone against the start in company, a solve against its own shorter run: bit
for bit.  The starts form folds in another order than ea_solve, so against the pair form of the same start the pose is held
to test_gpu_solve_starts.py's 1e-7 rad / 1e-7 and it_cost[0] to its 1e-12 relative."""
import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

TRACE = ("it_cost", "it_cost_change", "it_gradient_max_norm", "it_step_norm", "it_relative_decrease", "it_radius", "it_successful")
SCALARS = ("termination", "why", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost")
SIZES = (257, 1)
K = 3
PAST = dict(initial_trust_region_radius=1.0, max_trust_region_radius=1.0)   # the radius never grows: 140 small accepted steps


def assert_same_solve(a, b, where):
    """(q, t, summary) of one problem twice: the whole result, bit for bit"""
    (qa, ta, sa), (qb, tb, sb) = a, b
    assert np.array_equal(qa, qb) and np.array_equal(ta, tb), (where, qa, qb, ta, tb)
    for k in SCALARS:
        assert sa[k] == sb[k], (where, k, sa[k], sb[k])
    for k in TRACE:
        assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), (where, k)


def assert_leading_rows(long, short, rows, where):
    for k in TRACE:
        assert len(long[k]) >= rows and len(short[k]) >= rows, (where, k, len(long[k]), len(short[k]))
        assert np.array_equal(np.asarray(long[k])[:rows], np.asarray(short[k])[:rows]), (where, k)


@pytest.fixture(scope="module")
def base():
    return synth.make_problem(48, 64, 1100, 9, 11, 52.0, 52.0, 31.5, 23.5,
                              planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)),
                              planted_t=(0.01, -0.005, 0.02), normalize=True)


def _cloud(base, slot):
    n = SIZES[slot]
    return (base["xyz"][:n] if slot == 0 else base["xyz"][-n:]).copy()


def _problems(hip, base, side):
    out = []
    for slot in range(2):
        P = hip.Problem(*base["K"], dtype=hip.EA_F64)
        P.set_points(_cloud(base, slot)); P.set_dt_grid(base["grid"]); P.set_loss(hip.LOSS_CAUCHY, 0.7)
        out.append(P)
    if side == "prior":
        out[0].set_normal_prior(1, 5.0 * np.eye(3), np.asarray(base["t_true"], dtype=np.float64))
    elif side == "mask":
        out[0].set_constant_parameters([0, 0, 1, 0, 1, 0])
    return out


def _starts(seed):
    rng = np.random.default_rng(seed)
    q = np.zeros((K, 4)); t = np.zeros((K, 3))
    for k in range(K):
        q[k] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0, 1.5)))
        t[k] = rng.uniform(-0.03, 0.03, 3)
    q[0] = [1.0, 0, 0, 0]; t[0] = 0.0
    return q, t


def _solve(B, fused, q, t, **opts):
    B.set_tuning("fused_iterations", -1 if fused else 0)
    out = B.solve(q, t, **opts)
    assert B.info("fused_iterations") == (1 if fused else 0)
    return out


@pytest.mark.parametrize("side", ["none", "prior", "mask"])
@pytest.mark.parametrize("strategy_name", ["STRATEGY_LM", "STRATEGY_DOGLEG"])
def test_three_forms_one_step(hip, base, strategy_name, side):
    strategy = getattr(hip, strategy_name)
    probs = _problems(hip, base, side)
    B = hip.Batch(probs)
    try:
        q0 = np.zeros((K, 2, 4)); t0 = np.zeros((K, 2, 3))
        for i in range(2):
            q0[:, i], t0[:, i] = _starts(70 + i)
        # ---- fused form = pair form, from every start
        pair = []
        for k in range(K):
            qf, tf, sf = _solve(B, True, q0[k], t0[k], strategy=strategy)
            qp, tp, sp = _solve(B, False, q0[k], t0[k], strategy=strategy)
            for i in range(2):
                print(strategy_name, side, "start", k, "problem", i, "its", sp[i]["num_iterations"], sp[i]["why"], "cost",
                      sp[i]["initial_cost"], "->", sp[i]["final_cost"])
                assert_same_solve((qf[i], tf[i], sf[i]), (qp[i], tp[i], sp[i]), ("fused = pair", k, i))
            assert sp[0]["num_iterations"] > 0
            if side == "mask":
                assert tp[0, 1] == t0[k, 0, 1] and not np.array_equal(tp[0], t0[k, 0])   # the held coordinate: its input bits
            pair.append((qp, tp, sp))
        # ---- starts: in company, alone, without summaries; against the pair form of the same start
        q, t, s, best = B.solve_starts(q0, t0, strategy=strategy)
        assert B.info("starts_form") == 1
        for k in range(K):
            q1, t1, s1, _ = B.solve_starts(q0[k:k + 1], t0[k:k + 1], strategy=strategy)
            assert B.info("starts_form") == 1
            for i in range(2):
                assert_same_solve((q[k, i], t[k, i], s[k][i]), (q1[0, i], t1[0, i], s1[0][i]), ("alone = in company", k, i))
                qp, tp, sp = pair[k]
                ang = synth.rotation_angle_between(q[k, i], qp[i])
                dt = np.linalg.norm(t[k, i] - tp[i])
                c0, c0p = s[k][i]["it_cost"][0], sp[i]["it_cost"][0]
                print(strategy_name, side, "start", k, "problem", i, "starts against pair: angle", ang, "dt", dt, "it_cost[0]", c0, c0p)
                assert ang < 1e-7 and dt < 1e-7, (k, i, ang, dt)
                assert abs(c0 - c0p) <= 1e-12 * abs(c0p), (k, i, c0, c0p)
        q2, t2, none, best2 = B.solve_starts(q0, t0, summaries=False, strategy=strategy)
        assert none is None and np.array_equal(q2, q) and np.array_equal(t2, t) and np.array_equal(best2, best)
    finally:
        B.close()
        for P in probs:
            P.close()


def test_past_the_end_of_the_trace(hip, oracle, base):
    """140 iterations on 128 trace rows: trace_it >= kTrace never equals the last row, so lane 0 delivers all of them.  From
    the identity with the radius held at 1.0 the CPU oracle takes 140 successful LM steps and stops on max_iterations (final
    cost 1.3e-9); dogleg converges in 11 iterations under the same settings, so this is LM only."""
    X = _cloud(base, 0)
    O = oracle.OracleProblem(base["grid"], *base["K"], loss=hip.LOSS_CAUCHY, loss_a=0.7)
    _, _, so = O.solve(X, [1.0, 0, 0, 0], [0.0, 0, 0], max_num_iterations=140, **PAST)
    assert so["num_iterations"] == 140 and so["why"] == "max_iterations", so     # the input does what this test needs
    P = hip.Problem(*base["K"], dtype=hip.EA_F64)
    P.set_points(X); P.set_dt_grid(base["grid"]); P.set_loss(hip.LOSS_CAUCHY, 0.7)
    B = hip.Batch([P])
    try:
        q0, t0 = np.array([[1.0, 0, 0, 0]]), np.zeros((1, 3))

        def run(form, its):
            if form == "starts":
                q, t, s, _ = B.solve_starts(q0[None], t0[None], max_num_iterations=its, **PAST)
                assert B.info("starts_form") == 1
                return q[0, 0], t[0, 0], s[0][0]
            q, t, s = _solve(B, form == "fused", q0, t0, max_num_iterations=its, **PAST)
            return q[0], t[0], s[0]

        long = {}
        for form in ("fused", "pair", "starts"):
            long[form] = run(form, 140)
            s = long[form][2]
            print(form, "its", s["num_iterations"], s["why"], "successful", s["num_successful_steps"], "final cost", s["final_cost"],
                  "rows", len(s["it_cost"]))
            assert s["num_iterations"] == 140 and s["why"] == "max_iterations", (form, s["num_iterations"], s["why"])
            assert all(len(s[k]) == 128 for k in TRACE), form
            short = run(form, 120)[2]
            assert short["num_iterations"] == 120 and short["why"] == "max_iterations", form
            assert_leading_rows(s, short, 121, (form, "140 against 120"))
        assert_same_solve(long["fused"], long["pair"], "fused = pair, 140 iterations")   # (rows 0 .. 127 and everything else)
    finally:
        B.close(); P.close()
