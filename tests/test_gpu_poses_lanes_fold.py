"""The fold inside the launches of the one-pose-per-lane evaluation (ea_eval_poses_lanes_kernel, "poses_lane_per_pose" forced
to 1): lane-minor rows in one array, runs of R = 16 rows summed by the run's last arrival, the run partials by the problem's
last arrival, one pinned flag per (group of 64 poses, problem), results unpacked group by group.

Point counts put a problem at 1, R - 1, R, R + 1, 2R and 2R + 1 rows of 512 points (512, 7680, 8192, 8193, 16384, 16385),
alone and as one ragged batch together with 3 and 513 points; K on the group boundary (64, 65), one lane (1) and three groups
with a partly filled last (130).  Against the lanes-are-points kernel (key 0) on the same poses: n_invalid equal, cost within
1e-13, JtJ and Jtr within 1e-12 of the result's largest entry -- the bars tests/test_gpu_poses_lanes.py applies between the
two paths.  Within the path a pose's results are the same BITS in any lane, company, split into launches, item order and
call: the sums depend on the pose and the problem's row count only."""
import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

R = 16
ROWS = (1, R - 1, R, R + 1, 2 * R, 2 * R + 1)
SINGLES = (512, 7680, 8192, 8193, 16384, 16385)
RAGGED = SINGLES + (3, 513)
KS = (1, 64, 65, 130)
FIELDS = ("cost", "JtJ", "Jtr", "n_invalid")
assert tuple((n + 511) // 512 for n in SINGLES) == ROWS


@pytest.fixture(scope="module")
def base():
    # the 80 x 60 image of tests/test_gpu_poses_lanes.py (same segments), with as many points as the largest problem takes
    return synth.make_problem(60, 80, 16385, 12, 3, 65.0, 65.0, 39.5, 29.5, planted_q=synth.quat_from_axis_angle([1, 2, 3], 0.01),
                              planted_t=(0.004, -0.002, 0.006), normalize=True)


def _poses(rng, K, n, scale=1.0):
    q = np.zeros((K, n, 4)); t = np.zeros((K, n, 3))
    for k in range(K):
        for i in range(n):
            q[k, i] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(scale * rng.uniform(0.0, 1.5)))
            t[k, i] = scale * rng.uniform(-0.03, 0.03, size=3)
    return q, t


def _problems(hip, base, sizes, loss=None, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        P = hip.Problem(*base["K"], dtype=hip.EA_F64)
        P.set_points(base["xyz"][rng.choice(16385, n, replace=False)] if n else np.zeros((0, 3))); P.set_dt_grid(base["grid"])
        if loss is not None:
            P.set_loss(*loss)
        out.append(P)
    return out


def _both(B, q, t):
    """the same poses through key 0 and key 1"""
    B.set_tuning("poses_lane_per_pose", 0)
    old = B.eval_poses(q, t)
    assert B.info("poses_lane_per_pose") == 0
    B.set_tuning("poses_lane_per_pose", 1)
    new = B.eval_poses(q, t)
    assert B.info("poses_lane_per_pose") == 1
    return old, new


def _within_bars(old, new, where):
    assert np.array_equal(new["n_invalid"], old["n_invalid"]), where
    K, n = old["cost"].shape
    worst = [0.0, 0.0, 0.0]
    for k in range(K):
        for i in range(n):
            for j, (f, bar) in enumerate((("cost", 1e-13), ("JtJ", 1e-12), ("Jtr", 1e-12))):
                a, b = np.asarray(new[f][k, i]), np.asarray(old[f][k, i])
                scale = np.abs(b).max()
                err = np.abs(a - b).max() / scale if scale > 0 else np.abs(a - b).max()
                worst[j] = max(worst[j], err)
                assert err <= bar, (where, k, i, f, err)
    return worst


def _same_bits(a, b, where):
    for f in FIELDS:
        assert np.array_equal(a[f], b[f]), (where, f)


def _close(B, Ps):
    B.close()
    for P in Ps:
        P.close()


@pytest.mark.parametrize("sizes", [(n,) for n in SINGLES] + [RAGGED], ids=lambda s: "x".join(map(str, s)))
def test_run_boundaries_against_the_lanes_are_points_kernel(hip, base, sizes):
    """1, R - 1, R, R + 1, 2R and 2R + 1 rows as single problems (no row table) and as one ragged batch; every K"""
    Ps = _problems(hip, base, sizes, loss=(hip.LOSS_CAUCHY, 0.7))
    B = hip.Batch(Ps)
    try:
        rng = np.random.default_rng(101)
        worst = [0.0, 0.0, 0.0]
        for K in KS:
            q, t = _poses(rng, K, len(Ps))
            old, new = _both(B, q, t)
            assert B.info("poses_per_launch") == K
            w = _within_bars(old, new, (sizes, K))
            worst = [max(a, b) for a, b in zip(worst, w)]
        print("worst cost / JtJ / Jtr against key 0:", sizes, worst)
    finally:
        _close(B, Ps)


def test_a_pose_has_the_same_bits_in_any_lane_company_split_order_and_call(hip, base):
    Ps = _problems(hip, base, (16385, 8193, 3), loss=(hip.LOSS_CAUCHY, 0.7), seed=9)
    B = hip.Batch(Ps)
    try:
        B.set_tuning("poses_lane_per_pose", 1)
        rng = np.random.default_rng(31)
        q, t = _poses(rng, 130, len(Ps))
        pq, pt = _poses(rng, 1, len(Ps))
        alone = B.eval_poses(pq, pt)                     # K = 1: one live lane
        assert B.info("poses_lane_per_pose") == 1
        for at in (0, 37, 129):                          # lane 0, lane 37, lane 1 of the last, partly filled group
            qq, tt = q.copy(), t.copy()
            qq[at], tt[at] = pq[0], pt[0]
            got = B.eval_poses(qq, tt)
            for f in FIELDS:
                assert np.array_equal(got[f][at], alone[f][0]), (at, f)
        # three consecutive calls on the resident poses: counters and flags are armed again by every call
        for call in range(3):
            _same_bits(B.eval_resident_poses(), got, ("call", call))
        for order in (0, 1):
            B.set_tuning("poses_order", order)
            for g in (7, 64, 100, 0):
                B.set_tuning("poses_per_launch", g)
                split = B.eval_poses(qq, tt)
                assert B.info("poses_lane_per_pose") == 1
                assert B.info("poses_per_launch") == {7: 7, 64: 64, 100: 64, 0: 130}[g]
                _same_bits(split, got, (order, g))
        B.set_tuning("poses_order", -1)
        # K 130 -> 65 -> 130 on one batch: nothing of the larger call is left in rows, partials, counters or flags
        half = B.eval_poses(qq[:65], tt[:65])
        for f in FIELDS:
            assert np.array_equal(half[f], got[f][:65]), f
        _same_bits(B.eval_poses(qq, tt), got, "130 again")
    finally:
        _close(B, Ps)


@pytest.mark.parametrize("dt_f32,buffer_loads", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("loss", ["cauchy", "huber", "trivial"])
def test_losses_image_types_and_addressings_at_the_largest_batch(hip, base, loss, dt_f32, buffer_loads):
    spec = {"cauchy": (hip.LOSS_CAUCHY, 0.7), "huber": (hip.LOSS_HUBER, 0.2), "trivial": None}[loss]
    Ps = _problems(hip, base, RAGGED, loss=spec)
    B = hip.Batch(Ps)
    try:
        B.set_tuning("dt_f32", dt_f32); B.set_tuning("buffer_loads", buffer_loads)
        q, t = _poses(np.random.default_rng(103), 130, len(Ps))
        old, new = _both(B, q, t)
        print("worst cost / JtJ / Jtr against key 0:", loss, dt_f32, buffer_loads, _within_bars(old, new, (loss, dt_f32, buffer_loads)))
    finally:
        _close(B, Ps)


def test_a_problem_without_a_point_gets_zero_results(hip, base):
    """no work item belongs to it: the host writes its results and raises its flags"""
    Ps = _problems(hip, base, (8193, 0, 513), loss=(hip.LOSS_CAUCHY, 0.7), seed=5)
    B = hip.Batch(Ps)
    try:
        q, t = _poses(np.random.default_rng(7), 130, len(Ps))
        old, new = _both(B, q, t)
        _within_bars(old, new, "empty problem")
        for f in FIELDS:
            assert not np.any(new[f][:, 1]), f
        B.set_tuning("poses_per_launch", 64)
        _same_bits(B.eval_poses(q, t), new, "empty problem, three launches")
        _same_bits(B.eval_resident_poses(), new, "empty problem, again")
    finally:
        _close(B, Ps)


def test_priors_are_added_group_by_group(hip, base):
    Ps = _problems(hip, base, (16385, 127), loss=(hip.LOSS_CAUCHY, 0.7), seed=21)
    Ps[0].set_normal_prior(1, np.diag([3.0, 2.0, 5.0]), [0.01, -0.02, 0.005])
    B = hip.Batch(Ps)
    try:
        q, t = _poses(np.random.default_rng(41), 130, len(Ps))
        old, new = _both(B, q, t)
        _within_bars(old, new, "prior")
        B.set_tuning("poses_per_launch", 64)             # three launches, results unpacked group by group
        _same_bits(B.eval_poses(q, t), new, "prior, capped")
    finally:
        _close(B, Ps)


def test_one_launch_at_the_default_cap(hip, base):
    Ps = _problems(hip, base, (8193, 513), loss=(hip.LOSS_CAUCHY, 0.7), seed=3)
    B = hip.Batch(Ps)
    try:
        B.set_tuning("poses_lane_per_pose", 1)
        q, t = _poses(np.random.default_rng(43), 130, len(Ps))
        ref = B.eval_poses(q, t)
        assert B.bench_resident_poses(1)[1] == 1
        assert B.bench_resident_poses(1, evaluations_only=True)[1] == 1
        _same_bits(B.eval_resident_poses(), ref, "behind the hook")
        B.set_tuning("poses_per_launch", 64)
        B.set_poses(q, t)
        assert B.bench_resident_poses(1)[1] == -(-130 // 64)
        _same_bits(B.eval_resident_poses(), ref, "behind the hook, capped")
    finally:
        _close(B, Ps)
