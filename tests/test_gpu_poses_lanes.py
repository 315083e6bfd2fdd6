"""The pose-batched fp64 evaluation with one pose per lane (ea_eval_poses_lanes_kernel, tuning key "poses_lane_per_pose"):
a lane owns a pose, the wavefront walks the points of a 512-point row in four sub-runs of 128, two points per iteration.

Against the kernel it stands in for (key 0, lanes = points) on the same poses: n_invalid exactly equal, cost within 1e-13,
JtJ and Jtr within 1e-12 of the result's largest entry -- the same per-point expressions, another summation order; these
are the bars tests/test_gpu_eval_poses.py applies against ea_batch_eval.  Within the new path a pose's results are the
same BITS in any lane, alone or in company, under any split into launches and either item order.

Point counts sit on the pair (1, 2, 3), sub-run (127, 128, 129), row (511, 512, 513) and two-row (1025) boundaries; K on the
group boundary (63, 64, 65), one lane (1) and three groups with a partly filled last (130)."""
import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 127, 128, 129, 511, 512, 513, 1025)
KS = (1, 63, 64, 65, 130)
FIELDS = ("cost", "JtJ", "Jtr", "n_invalid")


@pytest.fixture(scope="module")
def base():
    return synth.make_problem(60, 80, 1025, 12, 3, 65.0, 65.0, 39.5, 29.5, planted_q=synth.quat_from_axis_angle([1, 2, 3], 0.01),
                              planted_t=(0.004, -0.002, 0.006), normalize=True)


def _poses(rng, K, n, scale=1.0):
    q = np.zeros((K, n, 4)); t = np.zeros((K, n, 3))
    for k in range(K):
        for i in range(n):
            q[k, i] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(scale * rng.uniform(0.0, 1.5)))
            t[k, i] = scale * rng.uniform(-0.03, 0.03, size=3)
    return q, t


def _problems(hip, base, sizes, loss=None, dtype=None, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        P = hip.Problem(*base["K"], dtype=hip.EA_F64 if dtype is None else dtype)
        P.set_points(base["xyz"][rng.choice(1025, n, replace=False)]); P.set_dt_grid(base["grid"])
        if loss is not None:
            P.set_loss(*loss)
        out.append(P)
    return out


def _both(B, q, t, expect_lanes=1):
    """the same poses through key 0 and key 1"""
    B.set_tuning("poses_lane_per_pose", 0)
    old = B.eval_poses(q, t)
    assert B.info("poses_lane_per_pose") == 0
    B.set_tuning("poses_lane_per_pose", 1)
    new = B.eval_poses(q, t)
    assert B.info("poses_lane_per_pose") == expect_lanes
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


def _close(B, Ps):
    B.close()
    for P in Ps:
        P.close()


@pytest.mark.parametrize("dt_f32,buffer_loads", [(1, 1), (1, 0), (0, 1), (0, 0)])
@pytest.mark.parametrize("loss", ["cauchy", "huber", "trivial"])
def test_against_the_lanes_are_points_kernel(hip, base, loss, dt_f32, buffer_loads):
    """every point count as one problem of a ragged batch, every K, three losses, both image types and addressings"""
    spec = {"cauchy": (hip.LOSS_CAUCHY, 0.7), "huber": (hip.LOSS_HUBER, 0.2), "trivial": None}[loss]
    Ps = _problems(hip, base, SIZES, loss=spec)
    B = hip.Batch(Ps)
    try:
        B.set_tuning("dt_f32", dt_f32); B.set_tuning("buffer_loads", buffer_loads)
        rng = np.random.default_rng(101)
        worst = [0.0, 0.0, 0.0]
        for K in KS:
            q, t = _poses(rng, K, len(Ps))
            old, new = _both(B, q, t)
            assert B.info("poses_per_launch") == K
            w = _within_bars(old, new, (loss, dt_f32, buffer_loads, K))
            worst = [max(a, b) for a, b in zip(worst, w)]
        print("worst cost / JtJ / Jtr against key 0:", loss, dt_f32, buffer_loads, worst)
    finally:
        _close(B, Ps)


@pytest.mark.parametrize("sizes", [(1,), (129,), (513,), (1025,), (1025, 3, 512)])
def test_single_problems_and_three_ragged_ones(hip, base, sizes):
    """a batch of one problem reads no row table; the batch of three does"""
    Ps = _problems(hip, base, sizes, loss=(hip.LOSS_CAUCHY, 0.7), seed=5)
    B = hip.Batch(Ps)
    try:
        rng = np.random.default_rng(7)
        for K in (1, 65, 130):
            q, t = _poses(rng, K, len(Ps))
            old, new = _both(B, q, t)
            _within_bars(old, new, (sizes, K))
    finally:
        _close(B, Ps)


def test_a_pose_has_the_same_bits_in_any_lane_company_split_and_order(hip, base):
    Ps = _problems(hip, base, (1025, 129, 3), loss=(hip.LOSS_CAUCHY, 0.7), seed=9)
    B = hip.Batch(Ps)
    try:
        B.set_tuning("poses_lane_per_pose", 1)
        rng = np.random.default_rng(31)
        q, t = _poses(rng, 130, len(Ps))
        pq, pt = _poses(rng, 1, len(Ps))
        alone = B.eval_poses(pq, pt)                     # K = 1: one live lane
        assert B.info("poses_lane_per_pose") == 1
        for at in (0, 37, 64 + 37, 129):                 # lane 0, lane 37, lane 37 of the second group, the last group's lane 1
            qq, tt = q.copy(), t.copy()
            qq[at], tt[at] = pq[0], pt[0]
            got = B.eval_poses(qq, tt)
            for f in FIELDS:
                assert np.array_equal(got[f][at], alone[f][0]), (at, f)
            if at != 37:
                continue
            again = B.eval_resident_poses()
            assert all(np.array_equal(again[f], got[f]) for f in FIELDS)
            for order in (0, 1):
                B.set_tuning("poses_order", order)
                for g in (7, 64, 100, 0):
                    B.set_tuning("poses_per_launch", g)
                    split = B.eval_poses(qq, tt)
                    assert B.info("poses_lane_per_pose") == 1
                    assert B.info("poses_per_launch") == {7: 7, 64: 64, 100: 64, 0: 130}[g]
                    assert all(np.array_equal(split[f], got[f]) for f in FIELDS), (order, g)
            B.set_tuning("poses_order", 0)
    finally:
        _close(B, Ps)


def test_failed_functors_off_image_and_non_unit_quaternions_in_some_lanes(hip, base):
    """lanes of one wavefront take different branches: points inside the z guard, points far off the image, a quaternion
    that is not a unit one -- each in some lanes only"""
    Ps = _problems(hip, base, (1025, 513), loss=(hip.LOSS_CAUCHY, 0.7), seed=13)
    B = hip.Batch(Ps)
    try:
        rng = np.random.default_rng(17)
        K = 130
        q, t = _poses(rng, K, len(Ps))
        zmean = float(np.mean(base["xyz"][:, 2]))
        for k in range(K):
            if k % 5 == 1:
                t[k, :, 2] = -zmean                      # points inside the z guard: failed functors
            if k % 7 == 2:
                t[k, :, 0] = 40.0                        # far off the image: replicated border texels
            if k % 3 == 0:
                q[k] *= 1.02                             # not a unit quaternion: the general Jacobian
            if k % 11 == 4:
                q[k, 0] = [1.02, 0.01, -0.02, 0.005]
        old, new = _both(B, q, t)
        assert old["n_invalid"][1::5].sum() > 0 and old["n_invalid"][0, 0] == 0
        print("worst cost / JtJ / Jtr against key 0:", _within_bars(old, new, "branches"))
    finally:
        _close(B, Ps)


def test_batches_and_calls_that_keep_their_kernel(hip, base):
    """a weighted term, an fp32 batch and K below the automatic threshold run what they ran: info 0, the same bits"""
    rng = np.random.default_rng(23)
    Ps = _problems(hip, base, (513, 129), loss=(hip.LOSS_CAUCHY, 0.7), seed=3)
    B = hip.Batch(Ps)
    try:
        q, t = _poses(rng, 100, len(Ps))
        B.set_tuning("poses_lane_per_pose", 0)
        old = B.eval_poses(q, t)
        B.set_tuning("poses_lane_per_pose", -1)          # automatic: no threshold below 128 poses
        auto = B.eval_poses(q, t)
        assert B.info("poses_lane_per_pose") == 0
        assert all(np.array_equal(auto[f], old[f]) for f in FIELDS)
        B.set_tuning("poses_lane_per_pose", 101)         # from 101 poses on: 100 stay
        assert all(np.array_equal(B.eval_poses(q, t)[f], old[f]) for f in FIELDS) and B.info("poses_lane_per_pose") == 0
        B.set_tuning("poses_lane_per_pose", 100)
        B.eval_poses(q, t)
        assert B.info("poses_lane_per_pose") == 1
        Ps[0].set_weights(rng.uniform(0.2, 1.0, size=513))
        old, new = _both(B, q, t, expect_lanes=0)
        assert all(np.array_equal(new[f], old[f]) for f in FIELDS)
    finally:
        _close(B, Ps)
    Ps = _problems(hip, base, (513, 129), loss=(hip.LOSS_CAUCHY, 0.7), dtype=hip.EA_F32, seed=3)
    B = hip.Batch(Ps)
    try:
        old, new = _both(B, q, t, expect_lanes=0)
        assert all(np.array_equal(new[f], old[f]) for f in FIELDS)
    finally:
        _close(B, Ps)


def test_priors_are_added_at_each_results_own_pose(hip, base):
    Ps = _problems(hip, base, (1025, 127), loss=(hip.LOSS_CAUCHY, 0.7), seed=21)
    Ps[0].set_normal_prior(1, np.diag([3.0, 2.0, 5.0]), [0.01, -0.02, 0.005])
    B = hip.Batch(Ps)
    try:
        q, t = _poses(np.random.default_rng(41), 130, len(Ps))
        old, new = _both(B, q, t)
        _within_bars(old, new, "prior")
        B.set_tuning("poses_per_launch", 64)             # results unpacked launch by launch
        split = B.eval_poses(q, t)
        assert all(np.array_equal(split[f], new[f]) for f in FIELDS)
    finally:
        _close(B, Ps)
