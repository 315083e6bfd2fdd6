"""The point loop of the one-pose-per-lane evaluation (ea_eval_poses_lanes_kernel, "poses_lane_per_pose" forced to 1) at every
length a wavefront's sub-run can end on: the coordinates of a pair arrive one pair ahead through 16-byte scalar loads while
both points lie inside the sub-run and through clamped 8-byte loads at its end (ea_lanes_stream.h), the pose and t_x, t_y are
read from LDS under the sums of the point in front.

Against key 0 on the same poses, with the bars tests/test_gpu_poses_lanes.py applies between the two paths: n_invalid equal,
cost within 1e-13, JtJ and Jtr within 1e-12 of the result's largest entry.  80 x 60 image; point counts that give sub-runs of
1, 2 and 3 points and odd and even lengths in every wavefront position (1, 2, 3, 4, 5, 127 .. 131, 255, 257, 385, 511, 512, 513,
515), each alone and all as one ragged batch; K = 1 and 65; Cauchy, Huber and the trivial loss; fp32- and fp64-stored images with
buffer and global addressing (the kernel's four instantiations); lanes with failed functors, off-image points and non-unit
quaternions among the others.  Every call is made twice and gives the same bits."""
import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

COUNTS = (1, 2, 3, 4, 5, 127, 128, 129, 130, 131, 255, 257, 385, 511, 512, 513, 515)
KS = (1, 65)
FORMS = ((1, 1), (1, 0), (0, 1), (0, 0))  # (dt_f32, buffer_loads)
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


def _spec(hip, loss):
    return {"cauchy": (hip.LOSS_CAUCHY, 0.7), "huber": (hip.LOSS_HUBER, 0.2), "trivial": None}[loss]


@pytest.mark.parametrize("sizes", [(n,) for n in COUNTS] + [COUNTS], ids=lambda s: "x".join(map(str, s)) if len(s) == 1 else "ragged")
def test_every_sub_run_length_in_all_four_instantiations(hip, base, sizes):
    """each count alone and all of them as one ragged batch, unit quaternions under the Cauchy loss: the pipelined loop"""
    Ps = _problems(hip, base, sizes, _spec(hip, "cauchy"))
    B = hip.Batch(Ps)
    try:
        rng = np.random.default_rng(101)
        worst = [0.0, 0.0, 0.0]
        for K in KS:
            q, t = _poses(rng, K, len(Ps))
            for dt_f32, buffer_loads in FORMS:
                B.set_tuning("dt_f32", dt_f32); B.set_tuning("buffer_loads", buffer_loads)
                old, new = _both(B, q, t)
                w = _within_bars(old, new, (sizes, K, dt_f32, buffer_loads))
                worst = [max(x, y) for x, y in zip(worst, w)]
        print("worst cost / JtJ / Jtr against key 0:", sizes, worst)
    finally:
        _close(B, Ps)


@pytest.mark.parametrize("dt_f32,buffer_loads", FORMS)
@pytest.mark.parametrize("loss", ["cauchy", "huber", "trivial"])
def test_losses_and_mixed_lanes_on_the_ragged_batch(hip, base, loss, dt_f32, buffer_loads):
    """the ragged batch under every loss in every instantiation; K = 1 and 65 of unit quaternions, then 130 poses of which
    0 .. 63 (one wavefront's lanes) mix unit and non-unit quaternions -- the general form -- and some lanes of both wavefronts
    have every point inside the z guard (failed functors) or far off the image"""
    Ps = _problems(hip, base, COUNTS, _spec(hip, loss), seed=13)
    B = hip.Batch(Ps)
    try:
        B.set_tuning("dt_f32", dt_f32); B.set_tuning("buffer_loads", buffer_loads)
        rng = np.random.default_rng(17)
        worst = [0.0, 0.0, 0.0]
        for K in KS:
            q, t = _poses(rng, K, len(Ps))
            old, new = _both(B, q, t)
            w = _within_bars(old, new, (loss, dt_f32, buffer_loads, K))
            worst = [max(x, y) for x, y in zip(worst, w)]
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
        w = _within_bars(old, new, (loss, dt_f32, buffer_loads, "mixed lanes"))
        worst = [max(x, y) for x, y in zip(worst, w)]
        print("worst cost / JtJ / Jtr against key 0:", loss, dt_f32, buffer_loads, worst)
    finally:
        _close(B, Ps)
