"""The head of a work item (EA_ITEM_HEAD in ea_kernels.hip: term 0's early point loads, descriptor and pose as one batch of
scalar loads, the early exit, the late point loads) is one text shared by ea_eval_fused_kernel, ea_eval_poses_kernel,
ea_cost_poses_kernel and ea_eval_starts_kernel, and its pieces by ea_lm_iter_kernel.  This walks its branch matrix at the
smallest shapes where it can go wrong and pins, in one place, the agreement between those kernels that used to rest on five
copies of the text being the same.

A batch of two single-term problems: problem 0 takes the early loads (its arrays and count arrive with the wave), problem 1
the late ones.  Point counts around the chunk c = poses_threads x poses_points_per_thread the batch reports: problem 0 in
{1, c - 1, c, c + 1} (one lane; the last lane clamped; a full chunk; a second workgroup of one point), problem 1 in
{c + 1, 1}.  buffer_loads 1 and 0, fp64 and fp32, a 64 x 48 image, three poses per problem.  The first point of every cloud is
moved along its ray to depth 0.25, in front of all the others (0.5 .. 5); the third pose pulls the cloud towards the camera by
exactly that, so this one point lands on the camera plane and fails the functor (n_invalid = 1) while every other point keeps
a depth of 0.25 or more -- no valid point comes near the singularity, which fp32 could not follow to 1e-4.

Bars: against the oracle 1e-11 (fp64) / 1e-4 (fp32) relative, those of test_gpu_eval_poses.py.  cost_poses against eval_poses
1e-13 in fp64 (at most 513 terms of one sign summed in another order: a few ulp) and test_gpu_cost_poses.py's 1e-5 in fp32.
Everything else is bit for bit."""
import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

FIELDS = ("cost", "JtJ", "Jtr", "n_invalid")
K = 3
NEAR = 0.25   # depth of every cloud's first point


@pytest.fixture(scope="module")
def base():
    return synth.make_problem(48, 64, 1100, 9, 11, 52.0, 52.0, 31.5, 23.5,
                              planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)),
                              planted_t=(0.01, -0.005, 0.02), normalize=True)


def _cloud(base, slot, n):
    """problem 0 reads the front of the cloud, problem 1 the back: a mixed-up descriptor or count shows"""
    X = (base["xyz"][:n] if slot == 0 else base["xyz"][-n:]).copy()
    X[0] *= NEAR / X[0, 2]
    return X


def _poses(base, slot, n):
    """two small poses of the slot's own and the one that puts the cloud's first point on the camera plane"""
    rng = np.random.default_rng(100 + slot)
    q = np.zeros((K, 4)); t = np.zeros((K, 3))
    for k in range(2):
        q[k] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0.2, 1.5)))
        t[k] = rng.uniform(-0.03, 0.03, size=3)
    q[2] = [1.0, 0, 0, 0]; t[2] = [0.0, 0.0, -NEAR]
    return q, t


@pytest.fixture(scope="module")
def oracle_at(hip, base, oracle):
    """(slot, n) -> the oracle's K evaluations, computed once"""
    O = oracle.OracleProblem(base["grid"], *base["K"], loss=hip.LOSS_CAUCHY, loss_a=0.7)
    cache = {}

    def at(slot, n):
        if (slot, n) not in cache:
            q, t = _poses(base, slot, n)
            cache[(slot, n)] = [O.eval(_cloud(base, slot, n), q[k], t[k]) for k in range(K)]
        return cache[(slot, n)]
    return at


@pytest.mark.parametrize("buf", [1, 0])
@pytest.mark.parametrize("dtype_name,tol,tol_cost", [("EA_F64", 1e-11, 1e-13), ("EA_F32", 1e-4, 1e-5)])
def test_branch_matrix(hip, base, oracle_at, dtype_name, tol, tol_cost, buf):
    dtype = getattr(hip, dtype_name)

    def problem(slot, n):
        P = hip.Problem(*base["K"], dtype=dtype)
        P.set_points(_cloud(base, slot, n)); P.set_dt_grid(base["grid"]); P.set_loss(hip.LOSS_CAUCHY, 0.7)
        return P

    # the chunk, as a batch of this dtype reports it
    probe = problem(0, 1)
    B = hip.Batch([probe])
    B.eval_poses(np.array([[[1.0, 0, 0, 0]]]), np.zeros((1, 1, 3)))
    c = B.info("poses_threads") * B.info("poses_points_per_thread")
    B.close(); probe.close()
    assert 1 < c and c + 1 <= base["xyz"].shape[0] // 2
    first = {n: problem(0, n) for n in (1, c - 1, c, c + 1)}
    second = {n: problem(1, n) for n in (c + 1, 1)}
    try:
        for n0, P0 in first.items():
            for n1, P1 in second.items():
                where = (dtype_name, buf, n0, n1)
                sizes = (n0, n1)
                q = np.zeros((K, 2, 4)); t = np.zeros((K, 2, 3))
                for i in range(2):
                    q[:, i], t[:, i] = _poses(base, i, sizes[i])
                B = hip.Batch([P0, P1])
                try:
                    B.set_tuning("buffer_loads", buf)
                    got = B.eval_poses(q, t)
                    assert B.info("buffer_loads") == buf, where
                    assert B.info("poses_threads") * B.info("poses_points_per_thread") == c, where
                    for k in range(K):
                        for i in range(2):
                            e = oracle_at(i, sizes[i])[k]
                            print(where, k, i, "cost", got["cost"][k, i], "oracle", e["cost"], "bad", got["n_invalid"][k, i], e["n_invalid"])
                            assert abs(got["cost"][k, i] - e["cost"]) <= tol * abs(e["cost"]), where + (k, i)
                            assert np.abs(got["JtJ"][k, i] - e["JtJ"]).max() <= tol * np.abs(e["JtJ"]).max(), where + (k, i)
                            assert np.abs(got["Jtr"][k, i] - e["Jtr"]).max() <= tol * np.abs(e["Jtr"]).max(), where + (k, i)
                            assert got["n_invalid"][k, i] == e["n_invalid"], where + (k, i)
                    assert (got["n_invalid"][2] == 1).all() and not got["n_invalid"][:2].any(), where
                    # a pose alone = the pose in company
                    for k in range(K):
                        alone = B.eval_poses(q[k:k + 1], t[k:k + 1])
                        assert all(np.array_equal(alone[f][0], got[f][k]) for f in FIELDS), where + (k,)
                    # the cost-only kernel: the same work items, two sums instead of 28
                    cost = B.cost_poses(q, t)
                    assert B.info("cost_form") == 1 and B.info("buffer_loads") == buf, where
                    assert (np.abs(cost["cost"] - got["cost"]) <= tol_cost * np.abs(got["cost"])).all(), where
                    assert np.array_equal(cost["n_invalid"], got["n_invalid"]), where
                    # a start's first evaluation = the pose-batched evaluation of that pose (a failed one ends the start)
                    qs, ts, s, best = B.solve_starts(q, t, max_num_iterations=4)
                    assert B.info("buffer_loads") == buf, where
                    for k in range(K):
                        for i in range(2):
                            if got["n_invalid"][k, i]:
                                assert s[k][i]["why"] == "initial_eval_failed", where + (k, i)
                            else:
                                assert s[k][i]["it_cost"][0] == got["cost"][k, i], where + (k, i)
                    # one launch per LM iteration = the (evaluate, step) pairs
                    runs = []
                    for fused in (-1, 0):
                        B.set_tuning("fused_iterations", fused)
                        runs.append(B.solve(q[0], t[0], max_num_iterations=4))
                        assert B.info("fused_iterations") == (1 if fused else 0) and B.info("buffer_loads") == buf, where
                    (qa, ta, sa), (qb, tb, sb) = runs
                    assert np.array_equal(qa, qb) and np.array_equal(ta, tb), where
                    for i in range(2):
                        assert sa[i]["num_iterations"] == sb[i]["num_iterations"] and sa[i]["why"] == sb[i]["why"], where + (i,)
                        assert np.array_equal(np.asarray(sa[i]["it_cost"]), np.asarray(sb[i]["it_cost"]), equal_nan=True), where + (i,)
                finally:
                    B.close()
    finally:
        for P in list(first.values()) + list(second.values()):
            P.close()
