"""Expected values for the per-point weights tests (the oracle has no weights):
(a) sums -- from the oracle's raw residuals and rows (OracleProblem.eval(..., materialize=True)) and the loss's closed form:
    cost = 1/2 sum w rho(r^2), JtJ = sum w rho' J^T J, Jtr = sum w rho' J^T r;
(b) solves -- integer weights w_i in {0..3} are the problem with point i repeated w_i times, so OracleProblem.solve on
    np.repeat(xyz, w, axis=0) is the oracle of the weighted solve.
(a) agrees with the oracle's own evaluation of the repeated cloud to <= 7e-15 relative (tests/test_weights_ref.py asserts 1e-13).
Failed blocks (|b_z| < z_guard: the functor returns false, the oracle's raw rows are NaN) are left out of the sums and counted
once each whatever their weight -- a block with ScaledLoss(..., 0) whose functor fails is still a failed block; `plant_failed`
puts such blocks into a cloud."""
import numpy as np

from edge_alignment_amd import synth

LOSS_TRIVIAL, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2
PLANTED_Q = synth.quat_from_axis_angle([0.3, -1.0, 0.5], np.deg2rad(0.6))
PLANTED_T = (0.004, -0.003, 0.005)
# (H, W, points, seed): the oracle's weighted solve from the identity ends on FUNCTION_TOLERANCE after 10, 14, 30 iterations
SOLVE_PROBLEMS = ((96, 128, 513, 11), (96, 128, 257, 12), (120, 160, 1025, 13))
Q0, T0 = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def loss_pair(kind, a, s):
    """rho(s), rho'(s) of TrivialLoss / CauchyLoss(a) / HuberLoss(a) (Ceres' definitions)"""
    s = np.asarray(s, dtype=np.float64)
    if kind == LOSS_TRIVIAL:
        return s.copy(), np.ones_like(s)
    b = a * a
    if kind == LOSS_CAUCHY:
        return b * np.log1p(s / b), 1.0 / (1.0 + s / b)
    r = np.sqrt(np.maximum(s, 1e-300))
    out = s > b
    return np.where(out, 2.0 * a * r - b, s), np.where(out, a / r, 1.0)


def n_failed(e):
    """failed blocks of a materialised oracle evaluation: each counts once, whatever its weight"""
    bad = np.isnan(e["raw_r"])
    assert int(bad.sum()) == e["n_invalid"] and np.array_equal(bad, np.isnan(e["raw_J"]).any(axis=1))
    return int(bad.sum())


def weighted_sums(e, w, kind=LOSS_CAUCHY, a=1.0):
    """(cost, JtJ, Jtr) of the weighted problem from a materialised oracle evaluation `e`; failed blocks (NaN raw rows, see
    n_failed) are left out of the sums"""
    ok = ~np.isnan(e["raw_r"])
    assert n_failed(e) == int((~ok).sum())
    r, J, w = e["raw_r"][ok], e["raw_J"][ok], np.asarray(w, dtype=np.float64)[ok]
    assert np.isfinite(r).all() and np.isfinite(J).all()
    rho, rho1 = loss_pair(kind, a, r * r)
    wr = w * rho1
    return 0.5 * np.sum(w * rho), (J * wr[:, None]).T @ J, J.T @ (wr * r)


# failed blocks: b = R X + t with |b_z| in [0.003, 0.008] -- fp32 storage of X (relative 6e-8 of coordinates below 0.1)
# cannot move it across the 0.01 guard
FAILED_BZ = (0.005, -0.004, 0.007)
FAILED_W = (2, 3, 0)


def failed_indices(n):
    """where the failed blocks go: point 0, point n - 1 (the last lane of a partial chunk) and one index with
    256 <= i mod 512, the k = 1 half of a two-point lane (300; for n <= 301 point n - 1 is that already when n > 256 and the
    third block goes to the middle).  Distinct and ascending; fewer than three for n < 3."""
    return sorted({0, n - 1, 300 if n > 301 else n // 2})


def plant_failed(xyz, q, t, idx=None, bz=FAILED_BZ):
    """a copy of the cloud with X_i = R^T (b - t), b = (0.02 (j + 1), -0.015, bz[j]), at the j-th index of idx: the functor
    fails on these blocks at pose (q, t) -> (cloud, idx)"""
    xyz = np.array(xyz, dtype=np.float64)
    idx = failed_indices(len(xyz)) if idx is None else list(idx)
    q = np.asarray(q, dtype=np.float64)
    R = synth.quat_to_R(q / np.linalg.norm(q))
    for j, i in enumerate(idx):
        b = np.array([0.02 * (j + 1), -0.015, bz[j]])
        xyz[i, :3] = (b - np.asarray(t, dtype=np.float64)) @ R
    return xyz, idx


def solve_problem(H, W, n, seed):
    """one of SOLVE_PROBLEMS: Cauchy(1), 24 segments, fx = fy = 130, principal point at the image centre, integer weights
    from default_rng(seed), then the same generator's N(0, 0.01 m) perturbation of the points (the fit is not exact)"""
    pr = synth.make_problem(H, W, n, 24, seed, 130.0, 130.0, (W - 1) / 2.0, (H - 1) / 2.0, planted_q=PLANTED_Q, planted_t=PLANTED_T)
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 4, n)
    xyz = pr["xyz"] + rng.normal(0.0, 0.01, (n, 3))
    return dict(xyz=xyz, grid=pr["grid"], K=pr["K"], w=w, repeated=np.repeat(xyz, w, axis=0))


def real_weights(n, seed):
    """real-valued weights in [0, 2] with exact zeros (every fifth, never the first)"""
    w = np.random.default_rng(seed).uniform(0.0, 2.0, n)
    w[2::5] = 0.0
    return w
