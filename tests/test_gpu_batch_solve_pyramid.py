"""ea_batch_solve_pyramid / solve_pyramid_batch: ea_solve_pyramid for every problem of the levels' batches -- one batch solve
per level, the coarsest first, the poses carried down.  The levels come from set_frames_ros_pyramid on four pairs of the bundled
640 x 480 frames: halvings = 1, three levels (320 x 240, 160 x 120, 80 x 60), the camera scaled per level (one level further up, at
40 x 30, a point or two of these pairs project outside the image, which fails the initial evaluation).  Compared bit for bit
(np.array_equal; costs through an integer view) against the loop of Batch.solve over the levels and against hip.solve_pyramid
per problem: at these sizes a batch resolves to a lone problem's launch shape, so the three agree to the bit.

One problem is forced to EA_FAILURE the way tests/test_gpu_tracker_batch.py reaches a failed solve with the ROS flavour -- a
NaN depth, whose points fail their functors: its full-size reference depth alternates +inf and -inf from column to column, so
every 2 x 2 mean is NaN on every level (the NaN -> 0 of the first step sees no NaN yet) -- so its coarsest level ends in
FAILURE at the start pose: it stops there, its finer summaries are zero and its pose is the one it came
with, while its neighbours get what they get without it."""
import numpy as np
import pytest

import test_gpu_batch_frames_ros as ros

pytestmark = pytest.mark.gpu
PAIRS = ((1, 2), (2, 3), (3, 4), (4, 5))
HALVINGS, LEVELS = 1, 3
KEYS = ("termination", "why", "num_iterations")
OPTS = dict(max_num_iterations=10)


@pytest.fixture(scope="module")
def frames():
    from edge_alignment_amd import synth
    full = {k: (bgr, dep.astype(np.float32) / np.float32(5000.0)) for k, (bgr, dep) in synth.load_bundled_frames(ros.G).items()}
    return [full[a][0] for a, _ in PAIRS], [full[a][1] for a, _ in PAIRS], [full[b][0] for _, b in PAIRS]


def _levels(hip, frames, dep=None):
    ref, dep0, now = frames
    probs = [[hip.Problem(*(k / (1 << (HALVINGS + l)) for k in ros.K)) for _ in PAIRS] for l in range(LEVELS)]
    batches = [hip.Batch(p) for p in probs]
    hip.set_frames_ros_pyramid(batches, ref, dep if dep is not None else dep0, now, halvings=HALVINGS)
    return probs, batches


def _same_summary(a, b, where):
    for key in KEYS:
        assert a[key] == b[key], (where, key, a[key], b[key])
    for key in ("initial_cost", "final_cost"):
        assert ros._same_bits(np.atleast_1d(a[key]), np.atleast_1d(b[key])), (where, key, a[key], b[key])


def _zero(s):
    return s["num_iterations"] == 0 and s["initial_cost"] == 0.0 and s["final_cost"] == 0.0 and s["termination"] == 0


def test_equals_the_loop_of_batch_solves_and_the_per_problem_pyramid(hip, frames):
    n = len(PAIRS)
    probs, batches = _levels(hip, frames)
    try:
        q0, t0 = np.tile([1.0, 0, 0, 0], (n, 1)), np.zeros((n, 3))
        q, t, sums = hip.solve_pyramid_batch(batches, q0, t0, **OPTS)
        assert len(sums) == LEVELS and all(len(s) == n for s in sums)
        lq, lt, lsums = q0.copy(), t0.copy(), [None] * LEVELS
        for l in range(LEVELS - 1, -1, -1):
            lq, lt, lsums[l] = batches[l].solve(lq, lt, **OPTS)
        assert np.array_equal(q, lq) and np.array_equal(t, lt)
        for l in range(LEVELS):
            for i in range(n):
                _same_summary(sums[l][i], lsums[l][i], ("loop", l, i))
        for i in range(n):
            pq, pt, ps = hip.solve_pyramid([probs[l][i] for l in range(LEVELS)], q0[i], t0[i], **OPTS)
            assert np.array_equal(q[i], pq) and np.array_equal(t[i], pt), (i, q[i], pq)
            for l in range(LEVELS):
                _same_summary(sums[l][i], ps[l], ("per problem", l, i))
        print("iterations per level (coarsest last):", [[s["num_iterations"] for s in lv] for lv in sums])
        assert all(s["termination"] != hip.FAILURE for lv in sums for s in lv)
        assert any(s["num_iterations"] > 1 for s in sums[LEVELS - 1]) and not np.array_equal(q, q0)
        # the start poses are the caller's, per problem
        q1 = q0.copy()
        q1[2] = [np.cos(0.01), np.sin(0.01), 0, 0]
        g = hip.solve_pyramid_batch(batches, q1, t0, **OPTS)
        p2 = hip.solve_pyramid([probs[l][2] for l in range(LEVELS)], q1[2], t0[2], **OPTS)
        assert np.array_equal(g[0][2], p2[0]) and np.array_equal(g[1][2], p2[1]) and np.array_equal(g[0][0], q[0])
    finally:
        ros._close(batches, *probs)


def test_a_problem_that_fails_at_the_coarsest_level_stops_there(hip, frames):
    n, bad = len(PAIRS), 1
    dep = [d.copy() for d in frames[1]]
    dep[bad][:, 0::2], dep[bad][:, 1::2] = np.inf, -np.inf     # every 2 x 2 mean is NaN, on every level
    probs, batches = _levels(hip, frames, dep)
    try:
        rng = np.random.default_rng(3)
        q0 = np.tile([1.0, 0, 0, 0], (n, 1))
        t0 = rng.normal(0, 0.003, (n, 3))
        q, t, sums = hip.solve_pyramid_batch(batches, q0, t0, **OPTS)
        assert sums[LEVELS - 1][bad]["termination"] == hip.FAILURE, sums[LEVELS - 1][bad]
        assert all(_zero(sums[l][bad]) for l in range(LEVELS - 1)), [sums[l][bad] for l in range(LEVELS - 1)]
        for i in range(n):
            pq, pt, ps = hip.solve_pyramid([probs[l][i] for l in range(LEVELS)], q0[i], t0[i], **OPTS)
            assert np.array_equal(q[i], pq) and np.array_equal(t[i], pt), (i, q[i], pq, t[i], pt)
            for l in range(LEVELS):
                _same_summary(sums[l][i], ps[l], ("per problem", l, i))
            if i != bad:
                assert all(s[i]["termination"] != hip.FAILURE for s in sums) and sums[0][i]["num_iterations"] >= 1
        # NULL summaries, and misuse
        q2, t2, _ = hip.solve_pyramid_batch(batches, q0, t0, **OPTS)
        assert np.array_equal(q2, q) and np.array_equal(t2, t)
        import ctypes as C
        L = hip.load()
        hs = (C.c_void_p * LEVELS)(*[b._h for b in batches])
        qq, tt = q0.copy(), t0.copy()
        assert L.ea_batch_solve_pyramid(hs, LEVELS, None, hip._dp(qq), hip._dp(tt), None) == hip.EA_OK
        assert L.ea_batch_solve_pyramid(hs, 0, None, hip._dp(qq), hip._dp(tt), None) == hip.EA_ERR_INVALID_ARG
        assert L.ea_batch_solve_pyramid(None, LEVELS, None, hip._dp(qq), hip._dp(tt), None) == hip.EA_ERR_INVALID_ARG
        assert L.ea_batch_solve_pyramid(hs, LEVELS, None, None, hip._dp(tt), None) == hip.EA_ERR_INVALID_ARG
        short = hip.Batch(probs[0][:2])
        try:
            mixed = (C.c_void_p * 2)(batches[1]._h, short._h)
            assert L.ea_batch_solve_pyramid(mixed, 2, None, hip._dp(qq), hip._dp(tt), None) == hip.EA_ERR_INVALID_ARG
        finally:
            short.close()
    finally:
        ros._close(batches, *probs)
