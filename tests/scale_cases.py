"""What tests/test_gpu_starts_scale.py, tests/test_gpu_batch_scale.py and tests/test_scale_catalogue.py share: the catalogue of
starting poses the big multi-start calls are indexed from, the patterns that lay it out over the positions of a call, and the
point sets of the many-problem / many-row batches.  Nothing here touches a device; the oracle is handed in.

The start catalogue sits on the 120 x 160 synthetic pair of test_gpu_solve_starts.py, Cauchy 0.7, first 300 points (one partial
row per pose, so that thousands of starts cost milliseconds):

  F  identity rotation, t = (0, 0, -z of point 0): point 0 on the camera plane, the first evaluation fails
     (initial_eval_failed) -- the planted failure of test_gpu_cost_poses.py;
  Q  the pose the oracle's solve from the identity converged to: ends within 2 iterations;
  S  N_S starts drawn as _starts(4.0) of test_gpu_solve_starts.py draws them (the first is the identity): iteration counts
     that spread widely, so that the live list shrinks a little at a time.

SEED was chosen on the CPU, for the oracle alone (test_scale_catalogue.py states what it rests on)."""
import functools

import numpy as np

from edge_alignment_amd import synth

LOSS_CAUCHY_A = 0.7
N_ROW = 300          # points of the catalogue's problem: one row
N_S = 24
SEED = 3
F, Q, S0 = 0, 1, 2   # catalogue indices: F, Q, then the S starts


@functools.lru_cache(maxsize=None)
def starts_base():
    """the synthetic pair of test_gpu_solve_starts.py"""
    return synth.make_problem(120, 160, 9000, 40, 1, 130.0, 130.0, 79.5, 59.5,
                              planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)),
                              planted_t=(0.01, -0.005, 0.02), normalize=True)


def draw_starts(s, K, seed):
    """_starts of test_gpu_solve_starts.py, restated (test_gpu_starts_scale.py holds the two to the same bits): rotations of up to
    1.5 s degrees about random axes, translations of up to 3 s cm, the first start the identity"""
    rng = np.random.default_rng(seed)
    q = np.zeros((K, 4)); t = np.zeros((K, 3))
    for k in range(K):
        q[k] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(s * rng.uniform(0, 1.5)))
        t[k] = s * rng.uniform(-0.03, 0.03, 3)
    q[0] = [1.0, 0, 0, 0]; t[0] = 0.0
    return q, t


def catalogue(oracle, X, grid=None, cam=None, n_s=N_S, seed=SEED):
    """(q (2 + n_s, 4), t (2 + n_s, 3)) for the cloud X: F, Q, S..."""
    base = starts_base()
    O = oracle.OracleProblem(base["grid"] if grid is None else grid, *(base["K"] if cam is None else cam), loss=1, loss_a=LOSS_CAUCHY_A)
    q = np.zeros((2 + n_s, 4)); t = np.zeros((2 + n_s, 3))
    q[F] = [1.0, 0, 0, 0]; t[F] = [0.0, 0.0, -X[0, 2]]
    q[Q], t[Q], _ = O.solve(X, [1.0, 0, 0, 0], [0.0, 0, 0])
    q[S0:], t[S0:] = draw_starts(4.0, n_s, seed)
    return q, t


# ---- patterns: catalogue index per position of a call of K starts -----------------------------------------------------------
def _s(i):
    return S0 + np.asarray(i) % N_S


def all_s(K, slowest=None):
    return _s(np.arange(K))


def first_round_f(K, slowest=None):
    """positions 0..255 F, the rest S"""
    idx = _s(np.arange(K)); idx[:256] = F
    return idx


def second_round_f(K, slowest=None):
    """positions 256..511 F, the rest S"""
    idx = _s(np.arange(K)); idx[256:512] = F
    return idx


def lone_slowest_at(pos):
    def pattern(K, slowest):
        idx = np.where(np.arange(K) % 3 == 0, F, Q)
        idx[pos] = slowest
        return idx
    pattern.__name__ = "lone_slowest_at_%d" % pos
    return pattern


def alternating(K, slowest=None):
    """S on even positions, F on odd ones"""
    i = np.arange(K)
    return np.where(i % 2 == 0, _s(i), F)


def alternating_wavefronts(K, slowest=None):
    """S and F by blocks of 64 positions: whole wavefronts of the compaction keep everything or nothing"""
    i = np.arange(K)
    return np.where((i // 64) % 2 == 0, _s(i), F)


def permuted(K, seed):
    """every catalogue entry about equally often, in a seeded permutation"""
    return (np.random.default_rng(seed).permutation(K) % (2 + N_S)).astype(np.int64)


# ---- the many-problem / many-row batches of test_gpu_batch_scale.py -----------------------------------------------------------
M_COUNTS = (1, 2, 3, 127, 129, 300, 511, 512)   # points per problem of batch M, cycled: one row each
M_PROBLEMS = 2049
R_ROWS = (1000, 1040, 8)                          # rows of 512 points of batch R's three problems; a fourth of one point makes 2049
CHECKED = (0, 100, 129)                           # of K = 130 poses: the first, one inside a middle launch, the last


@functools.lru_cache(maxsize=None)
def lanes_base():
    """the 60 x 80 synthetic pair of test_gpu_poses_lanes.py"""
    return synth.make_problem(60, 80, 1025, 12, 3, 65.0, 65.0, 39.5, 29.5, planted_q=synth.quat_from_axis_angle([1, 2, 3], 0.01),
                              planted_t=(0.004, -0.002, 0.006), normalize=True)


def m_clouds(seed=11):
    """2 049 sub-samples of the 1 025-point cloud, sizes cycling over M_COUNTS"""
    xyz = lanes_base()["xyz"]
    rng = np.random.default_rng(seed)
    return [xyz[rng.choice(1025, M_COUNTS[i % len(M_COUNTS)], replace=False)] for i in range(M_PROBLEMS)]


def r_clouds(seed=13):
    """the three clouds of batch R and the one-point fourth: the 1 025-point cloud resampled, every copy moved by less than half
    a pixel at its own depth"""
    base = lanes_base()
    xyz, (fx, fy, _, _) = base["xyz"], base["K"]
    rng = np.random.default_rng(seed)
    n = 512 * sum(R_ROWS) + 1
    X = xyz[rng.integers(0, 1025, n)].copy()
    X[:, 0] += X[:, 2] * rng.uniform(-0.5, 0.5, n) / fx
    X[:, 1] += X[:, 2] * rng.uniform(-0.5, 0.5, n) / fy
    cuts = np.cumsum([512 * r for r in R_ROWS])
    return [X[:cuts[0]], X[cuts[0]:cuts[1]], X[cuts[1]:cuts[2]], X[cuts[2]:]]


def draw_poses(rng, K, n, scale=1.0):
    """_poses of test_gpu_poses_lanes.py -- a rotation of up to 1.5 degrees x scale about a random axis, up to 3 cm x scale --
    drawn with array operations (K x n quaternions in a Python loop cost seconds at n = 2 049)"""
    axis = rng.normal(size=(K, n, 3))
    axis /= np.linalg.norm(axis, axis=-1, keepdims=True)
    half = 0.5 * np.deg2rad(scale * rng.uniform(0.0, 1.5, size=(K, n, 1)))
    q = np.concatenate([np.cos(half), np.sin(half) * axis], axis=-1)
    t = scale * rng.uniform(-0.03, 0.03, size=(K, n, 3))
    return np.ascontiguousarray(q), t


def scale_poses(clouds, seed, K=130):
    """K poses per problem; at the CHECKED poses 100 and 129 some problems get failed functors: t_z = -mean z of the whole cloud
    on every third problem (points inside the z guard where the problem has some near the mean, large terms next to it), and at
    pose 100 every fifth problem has its own first point on the camera plane under the identity rotation (certain).  Pose 0
    is left as drawn: there the largest entry a deviation is measured against is an ordinary problem's"""
    n = len(clouds)
    q, t = draw_poses(np.random.default_rng(seed), K, n)
    zmean = float(np.mean(np.concatenate([X[:, 2] for X in clouds])))
    for k in CHECKED[1:]:
        t[k, 1::3, 2] = -zmean
    for i in range(2, n, 5):
        q[100, i] = [1.0, 0, 0, 0]; t[100, i] = [0.0, 0.0, -clouds[i][0, 2]]
    return q, t


def within_bars(old, new, where):
    """_within_bars of test_gpu_poses_lanes.py with array operations: n_invalid equal; per (pose, problem) cost within 1e-13, JtJ
    and Jtr within 1e-12 of the reference's largest entry (absolute where that is 0) -> the worst of each"""
    assert np.array_equal(new["n_invalid"], old["n_invalid"]), where
    K, n = old["cost"].shape
    worst = []
    for f, bar in (("cost", 1e-13), ("JtJ", 1e-12), ("Jtr", 1e-12)):
        a, b = np.asarray(new[f]).reshape(K, n, -1), np.asarray(old[f]).reshape(K, n, -1)
        scale = np.abs(b).max(axis=-1)
        err = np.abs(a - b).max(axis=-1) / np.where(scale > 0, scale, 1.0)
        k, i = np.unravel_index(np.argmax(err), err.shape)
        assert err[k, i] <= bar, (where, int(k), int(i), f, float(err[k, i]))
        worst.append(float(err[k, i]))
    return worst


def planted_clouds(n_problems, seed):
    """n_problems clouds of 200 .. 513 points on the image of starts_base(), each with a planted pose of its own drawn as
    test_gpu_lm_random.py draws them (0.2 .. 3 degrees, up to 4 cm): the pair's edge points in frame B taken back through
    the problem's own pose"""
    base = starts_base()
    b = base["xyz"] @ synth.quat_to_R(base["q_true"]).T + base["t_true"]
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_problems):
        q_pl = synth.quat_from_axis_angle(rng.standard_normal(3), np.deg2rad(rng.uniform(0.2, 3.0)))
        t_pl = rng.uniform(-0.04, 0.04, 3)
        n = int(rng.integers(200, 514))
        pick = np.sort(rng.choice(len(b), n, replace=False))
        out.append(dict(xyz=(b[pick] - t_pl) @ synth.quat_to_R(q_pl), q_true=q_pl, t_true=t_pl))
    return out


def scrub(idx):
    """the call that goes in front of a checked call: F wherever the pattern has anything but F, Q where it has F.  Run with
    max_num_iterations = 0 every start ends in the first step launch -- F on its failed evaluation, Q on the iteration limit --
    which reads the list the HOST wrote, so every slot of the pinned delivery block is rewritten whatever the compaction does, with
    a result that differs from the checked call's at every position: a start the checked call never delivers cannot pass on what
    an earlier call left in its slot"""
    return np.where(np.asarray(idx) == F, Q, F)


def expected_best(idx, failed, final_cost):
    """the lowest position among the non-failed starts of minimal final cost (failed, final_cost: per catalogue entry); -1 if none"""
    ok = [j for j, c in enumerate(idx) if not failed[c]]
    return min(ok, key=lambda j: (final_cost[idx[j]], j)) if ok else -1
