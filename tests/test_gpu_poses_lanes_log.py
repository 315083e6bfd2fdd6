"""The cost of the one-pose-per-lane evaluation (ea_eval_poses_lanes_kernel, "poses_lane_per_pose" forced to 1) under the
unweighted Cauchy loss: a lane multiplies the factors s = 1 + r^2 / a^2 of the 128 points of its sub-run up (pl_run_*,
ea_pair_log.h) and takes ONE logarithm behind the sub-run, where the lanes-are-points kernel (key 0) takes one per pair of points.

Against key 0 on the same poses, with the bars tests/test_gpu_poses_lanes.py applies between the two paths: n_invalid equal,
cost within 1e-13, JtJ and Jtr within 1e-12 of the result's largest entry.  80 x 60 image; 1, 2, 127, 128, 129 and 513 points
(one point, an odd sub-run, a sub-run's edge, a second row) as single problems and as one ragged batch; K = 1 and 65;
a = 1 (s of order 1 .. 1e3), a = 1e-3 (s ~ 2^31 per point: the product passes 2^400 every dozen points and is renormalised
within a sub-run) and a = 1e3 (s - 1 ~ 1e-6 and below).  Huber and the trivial loss keep their statements and must agree on the
same points; so must lanes with failed functors, off-image points and non-unit quaternions, in wavefronts of unit
quaternions only and in mixed ones.  A second run gives the same bits."""
import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

SINGLES = (1, 2, 127, 128, 129, 513)
KS = (1, 65)
FIELDS = ("cost", "JtJ", "Jtr", "n_invalid")


@pytest.fixture(scope="module")
def base():
    # the 80 x 60 image of tests/test_gpu_poses_lanes.py (same segments)
    return synth.make_problem(60, 80, 1025, 12, 3, 65.0, 65.0, 39.5, 29.5, planted_q=synth.quat_from_axis_angle([1, 2, 3], 0.01),
                              planted_t=(0.004, -0.002, 0.006), normalize=True)


def _poses(rng, K, n):
    q = np.zeros((K, n, 4)); t = np.zeros((K, n, 3))
    for k in range(K):
        for i in range(n):
            q[k, i] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0.0, 1.5)))
            t[k, i] = rng.uniform(-0.03, 0.03, size=3)
    return q, t


def _problems(hip, base, sizes, loss, seed=11):
    rng = np.random.default_rng(seed)
    out = []
    for n in sizes:
        P = hip.Problem(*base["K"], dtype=hip.EA_F64)
        P.set_points(base["xyz"][rng.choice(1025, n, replace=False)]); P.set_dt_grid(base["grid"])
        if loss is not None:
            P.set_loss(*loss)
        out.append(P)
    return out


def _both(B, q, t):
    """the same poses through key 0 and key 1, the latter twice: equal bits"""
    B.set_tuning("poses_lane_per_pose", 0)
    old = B.eval_poses(q, t)
    assert B.info("poses_lane_per_pose") == 0
    B.set_tuning("poses_lane_per_pose", 1)
    new = B.eval_poses(q, t)
    assert B.info("poses_lane_per_pose") == 1
    again = B.eval_poses(q, t)
    for f in FIELDS:
        assert np.array_equal(again[f], new[f]), ("second run", f)
    return old, new


def _within_bars(old, new, where):
    assert np.array_equal(new["n_invalid"], old["n_invalid"]), where
    K, n = old["cost"].shape
    worst = [0.0, 0.0, 0.0]
    for k in range(K):
        for i in range(n):
            for j, (f, bar) in enumerate((("cost", 1e-13), ("JtJ", 1e-12), ("Jtr", 1e-12))):
                a, b = np.asarray(new[f][k, i]), np.asarray(old[f][k, i])
                assert np.all(np.isfinite(a)), (where, k, i, f)
                scale = np.abs(b).max()
                err = np.abs(a - b).max() / scale if scale > 0 else np.abs(a - b).max()
                worst[j] = max(worst[j], err)
                assert err <= bar, (where, k, i, f, err)
    return worst


def _close(B, Ps):
    B.close()
    for P in Ps:
        P.close()


@pytest.mark.parametrize("a", [1.0, 1e-3, 1e3])
@pytest.mark.parametrize("sizes", [(n,) for n in SINGLES] + [SINGLES], ids=lambda s: "x".join(map(str, s)))
def test_cauchy_cost_against_the_lanes_are_points_kernel(hip, base, sizes, a):
    Ps = _problems(hip, base, sizes, (hip.LOSS_CAUCHY, a))
    B = hip.Batch(Ps)
    try:
        rng = np.random.default_rng(101)
        worst = [0.0, 0.0, 0.0]
        for K in KS:
            q, t = _poses(rng, K, len(Ps))
            old, new = _both(B, q, t)
            if a == 1e-3 and max(sizes) >= 127:
                # the factors really are large: the product of a sub-run is far past the range of a double
                assert old["cost"].max() > 0.5 * a * a * 401 * np.log(2.0)
            w = _within_bars(old, new, (sizes, a, K))
            worst = [max(x, y) for x, y in zip(worst, w)]
        print("worst cost / JtJ / Jtr against key 0:", sizes, a, worst)
    finally:
        _close(B, Ps)


@pytest.mark.parametrize("loss", ["huber", "trivial"])
def test_huber_and_trivial_on_the_same_points(hip, base, loss):
    spec = {"huber": (hip.LOSS_HUBER, 0.2), "trivial": None}[loss]
    Ps = _problems(hip, base, SINGLES, spec)
    B = hip.Batch(Ps)
    try:
        rng = np.random.default_rng(101)
        for K in KS:
            q, t = _poses(rng, K, len(Ps))
            old, new = _both(B, q, t)
            print("worst cost / JtJ / Jtr against key 0:", loss, K, _within_bars(old, new, (loss, K)))
    finally:
        _close(B, Ps)


@pytest.mark.parametrize("a", [1.0, 1e-3])
def test_failed_functors_off_image_and_non_unit_quaternions_in_some_lanes(hip, base, a):
    """poses 0 .. 63 (one wavefront's lanes) mix unit and non-unit quaternions: the general form, which keeps the paired
    logarithm; poses 64 .. 127 are unit quaternions, some with every point inside the z guard or far off the image: the
    running product takes a factor of exactly 1 from a lane without a valid point"""
    Ps = _problems(hip, base, (513, 129), (hip.LOSS_CAUCHY, a), seed=13)
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
            if k < 64 and k % 3 == 0:
                q[k] *= 1.02                             # not a unit quaternion: the general Jacobian
        old, new = _both(B, q, t)
        assert old["n_invalid"][1:64:5].sum() > 0 and old["n_invalid"][66:128:5].sum() > 0 and old["n_invalid"][0, 0] == 0
        print("worst cost / JtJ / Jtr against key 0:", a, _within_bars(old, new, ("branches", a)))
    finally:
        _close(B, Ps)
