"""The pose-batched evaluation in its flat launch form (ea_eval_poses_kernel: one XCD-balanced work list per launch, the fold
of launch i riding in launch i + 1, a closing fold, results unpacked launch by launch) on the 120 x 160 synthetic problem of
test_gpu_eval_poses.py: chunk counts at the edges of the deal (1, 2, 8, 9, 13 chunks; rows x poses mostly no multiple of 8),
every split of K over launches, a two-term problem beside a one-term one (grid form), a NormalPrior across three launches,
every launch shape, and failed functors in the middle launch of a split.

Bars: against ea_batch_eval at the same pose 1e-13 (fp64) / 2e-6 (fp32) relative, the bars of test_gpu_eval_poses.py (same
chunks, folded in another order; pose constants built on the device); between launch shapes 1e-12 / 1e-5; the same pose
evaluated alone, in any split, or twice: the same bits."""
import ctypes as C

import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

FIELDS = ("cost", "JtJ", "Jtr", "n_invalid")
DTYPES = [("EA_F64", 1e-13, 1e-12), ("EA_F32", 2e-6, 1e-5)]


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _poses(rng, K, n, scale=1.0):
    q = np.zeros((K, n, 4)); t = np.zeros((K, n, 3))
    for k in range(K):
        for i in range(n):
            q[k, i] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(scale * rng.uniform(0.0, 1.5)))
            t[k, i] = scale * rng.uniform(-0.03, 0.03, size=3)
    return q, t


@pytest.fixture(scope="module")
def base():
    return synth.make_problem(120, 160, 9000, 40, 1, 130.0, 130.0, 79.5, 59.5,
                              planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)),
                              planted_t=(0.01, -0.005, 0.02), normalize=True)


def _problem(hip, base, dtype, n, rng=None):
    X = base["xyz"][:n] if rng is None else base["xyz"][rng.choice(9000, n, replace=False)]
    P = hip.Problem(*base["K"], dtype=dtype)
    P.set_points(X.reshape(-1, 3)); P.set_dt_grid(base["grid"]); P.set_loss(hip.LOSS_CAUCHY, 0.7)
    return P


def _same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in FIELDS)


def _against_eval(B, q, t, got, tol):
    for k in range(q.shape[0]):
        ref = B.eval(q[k], t[k])
        for f in ("cost", "JtJ", "Jtr"):
            assert _rel(got[f][k], ref[f]) <= tol, (k, f, _rel(got[f][k], ref[f]))
        assert np.array_equal(got["n_invalid"][k], ref["n_invalid"]), k


@pytest.mark.parametrize("dtype_name,tol,tol_shape", DTYPES)
def test_chunk_counts_at_the_edges_of_the_deal(hip, base, dtype_name, tol, tol_shape):
    dtype = getattr(hip, dtype_name)
    rng = np.random.default_rng(41)
    sizes = (1, 511, 512, 513, 3585, 4097, 6145)
    probs = [_problem(hip, base, dtype, n, rng) for n in sizes]
    empty = _problem(hip, base, dtype, 0)
    batches = [hip.Batch([P]) for P in probs] + [hip.Batch(probs[:3] + [empty] + probs[3:])]
    try:
        for B, chunks in zip(batches, (1, 1, 1, 2, 8, 9, 13, 35)):
            n = len(B)
            for K in (1, 3, 8, 11):
                q, t = _poses(rng, K, n)
                got = B.eval_poses(q, t)
                assert B.info("poses_tiles") == chunks and B.info("poses_threads") == 256 and B.info("poses_points_per_thread") == 2
                _against_eval(B, q, t, got, tol)
                for k in range(K):   # the pose alone in a call of its own: the same bits
                    one = B.eval_poses(q[k:k + 1], t[k:k + 1])
                    assert all(np.array_equal(one[f][0], got[f][k]) for f in FIELDS), (n, K, k)
            if n > 1:
                e = 3
                assert not got["cost"][:, e].any() and not got["JtJ"][:, e].any() and not got["n_invalid"][:, e].any()
    finally:
        for B in batches:
            B.close()
        for P in probs + [empty]:
            P.close()


@pytest.mark.parametrize("dtype_name,tol,tol_shape", DTYPES)
def test_every_split_over_launches_gives_the_same_bits(hip, base, dtype_name, tol, tol_shape):
    dtype = getattr(hip, dtype_name)
    rng = np.random.default_rng(43)
    probs = [_problem(hip, base, dtype, n, rng) for n in (4097, 700)]
    B = hip.Batch(probs)
    L = hip.load()
    try:
        for K in (5, 20):
            q, t = _poses(rng, K, 2)
            first = None
            for g in (1, 2, 3, 0):
                B.set_tuning("poses_per_launch", g)
                B.set_poses(q, t)
                out = B.eval_resident_poses()
                for f in FIELDS:   # filled again over NaN: every result of every launch is unpacked
                    out[f][...] = np.nan if out[f].dtype == np.float64 else -1
                B.eval_resident_poses(out=out)
                assert not any(np.isnan(out[f]).any() for f in ("cost", "JtJ", "Jtr")) and (out["n_invalid"] >= 0).all(), (K, g)
                first = first or {f: out[f].copy() for f in FIELDS}
                assert _same(out, first), (K, g)
                again = B.eval_resident_poses()
                assert _same(again, first), (K, g)
                # cost alone through the C entry point
                cost = np.full((K, 2), np.nan)
                assert L.ea_batch_eval_resident_poses(B._h, hip._dp(cost), None, None, None) == 0
                assert np.array_equal(cost, first["cost"]), (K, g)
                # nothing fetched, then fetched
                B.eval_resident_poses(fetch=False)
                assert _same(B.eval_resident_poses(), first), (K, g)
            _against_eval(B, q, t, first, tol)
    finally:
        B.close()
        for P in probs:
            P.close()


def test_two_terms_beside_one_term(hip, base):
    rng = np.random.default_rng(47)
    P = _problem(hip, base, hip.EA_F64, 5000)
    T = _problem(hip, base, hip.EA_F64, 1500)
    S = _problem(hip, base, hip.EA_F64, 2100, rng)
    P.add_term(T)
    B = hip.Batch([P, S])
    try:
        q, t = _poses(rng, 7, 2)
        B.set_tuning("poses_per_launch", 3)
        _against_eval(B, q, t, B.eval_poses(q, t), 1e-13)
    finally:
        B.close(); P.close(); T.close(); S.close()


def test_normal_prior_across_three_launches(hip, base):
    rng = np.random.default_rng(53)
    P = _problem(hip, base, hip.EA_F64, 4097)
    S = _problem(hip, base, hip.EA_F64, 900, rng)
    P.set_normal_prior(0, 3.0 * np.eye(4), np.array([1.0, 0.002, -0.001, 0.003]))
    P.set_normal_prior(1, np.diag([5.0, 7.0, 9.0]), np.array([0.01, -0.02, 0.005]))
    B = hip.Batch([P, S])
    try:
        q, t = _poses(rng, 8, 2)
        B.set_tuning("poses_per_launch", 3)   # launches of 3, 3, 2 poses
        got = B.eval_poses(q, t)
        _against_eval(B, q, t, got, 1e-13)
        assert len({float(c) for c in got["cost"][:, 0]}) == 8   # (each result carries the prior at its own pose)
    finally:
        B.close(); P.close(); S.close()


@pytest.mark.parametrize("dtype_name,tol,tol_shape", DTYPES)
def test_launch_shapes_agree(hip, base, dtype_name, tol, tol_shape):
    dtype = getattr(hip, dtype_name)
    rng = np.random.default_rng(59)
    probs = [_problem(hip, base, dtype, n, rng) for n in (9000, 257)]
    B = hip.Batch(probs)
    try:
        q, t = _poses(rng, 5, 2)
        B.set_tuning("poses_per_launch", 2)
        first = None
        for ppt in ((1, 2) if dtype_name == "EA_F64" else (1, 2, 4)):
            for nt in (256, 1024):
                B.set_tuning("points_per_thread", ppt); B.set_tuning("threads", nt)
                got = B.eval_poses(q, t)
                first = first or got
                for f in ("cost", "JtJ", "Jtr"):
                    assert _rel(got[f], first[f]) <= tol_shape, (ppt, nt, f)
                assert np.array_equal(got["n_invalid"], first["n_invalid"])
        for order in (1, 0):   # the other item order of the work list: the same rows, the same bits
            B.set_tuning("poses_order", order)
            assert _same(B.eval_poses(q, t), got), order
    finally:
        B.close()
        for P in probs:
            P.close()


def test_failed_functors_in_the_middle_launch(hip, base):
    P = _problem(hip, base, hip.EA_F64, 3000)
    B = hip.Batch([P])
    try:
        zmean = float(np.mean(base["xyz"][:3000, 2]))
        K = 6
        q = np.tile([1.0, 0, 0, 0], (K, 1, 1)); t = 0.002 * np.arange(K * 3, dtype=np.float64).reshape(K, 1, 3)
        t[3, 0] = [0.0, 0.0, -zmean]   # pose 3 = the second pose of the middle launch: points inside the z guard
        B.set_tuning("poses_per_launch", 2)
        got = B.eval_poses(q, t)
        for k in range(K):
            assert got["n_invalid"][k, 0] == B.eval(q[k], t[k])["n_invalid"][0], k
        assert got["n_invalid"][3, 0] > 0 and not got["n_invalid"][[0, 1, 2, 4, 5], 0].any()
    finally:
        B.close(); P.close()
