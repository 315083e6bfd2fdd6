"""ea_tracker_batch / TrackerBatch: N streams pushed in lock-step through the batched producers -- every frame processed once
for both sides -- and one batch solve.  The reference is always the single-stream form on the same frames: a hip.Tracker per
stream for flavours 0 and 1, and for flavour 2 (ROS, which ea_tracker does not have) the manual loop set_now_frame_ros ->
solve from the prior -> set_ref_frame_ros on a problem per stream.  Everything is compared with np.array_equal (floats through
an integer view, so that NaN compares equal to itself): poses, aligned flags, iteration counts, final costs, terminations, the
streams' points and depth weights, covariances.  Bit equality holds because the batched producers are bit for bit their
per-problem forms, and ea_batch_solve is too for problems of one kernel family at these sizes -- the streams here have
settings of their own (`_knobs`: one with depth weighting, whose variant kernels a plain neighbour must not be moved to), so
the tracker's grouping of the aligned streams by family is under test as well.

Streams of one call differ in kind and in camera, so that a stream reading its neighbour's slot, counts or workspace cannot go
unnoticed: stream 0 sees a `_random_frame` scene of tests/test_gpu_preprocess.py a pixel further on in every push, the others
the kinds of tests/test_gpu_batch_frames_ros.py (noise, lines, dot, flat).  Working shapes are the smallest at which the
indexing can go wrong: (17, 61) one count block; (37, 70) two hysteresis tiles and a partial 1024-pixel scan block; (130, 257)
past a 256-lane row block, several scan blocks.  Flavour 2 runs at these without halvings and from (74, 140) halved once."""
import numpy as np
import pytest

import test_gpu_batch_frames_ros as ros
from test_gpu_preprocess import _random_frame

pytestmark = pytest.mark.gpu
SHAPES = ((17, 61), (37, 70), (130, 257))
ROS_CASES = (((17, 61), 0), ((37, 70), 0), ((130, 257), 0), ((37, 70), 1))
IDENTITY = (np.array([1.0, 0, 0, 0]), np.zeros(3))
SIGMAS = (0.05, 0.2)


def _bits(a, b):
    return ros._same_bits(np.atleast_1d(a), np.atleast_1d(b))


def _knobs(P, i):
    """settings of its own per stream: loss scale, depth weighting (stream 0), auto-scaled loss (1), a constant mask (2)"""
    P.set_loss(1, 1.0 - 0.25 * (i % 3))                        # EA_LOSS_CAUCHY
    if i % 3 == 0:
        P.set_depth_weighting(2.0, 1)
    if i % 3 == 1:
        P.set_loss_auto_scale(3.536)
    if i % 3 == 2:
        P.set_constant_parameters([0, 0, 1, 0, 0, 0])


class _SingleTracker:
    """stream i as ea_tracker drives it"""

    def __init__(self, hip, i, cam, dtype, flavour, cov, prior):
        self.hip, self.T = hip, hip.Tracker(*cam, dtype=dtype, flavour=flavour)
        self.P = hip._StreamProblem(hip.load().ea_tracker_problem(self.T._h), dtype, 0)
        _knobs(self.P, i)
        self.cov = cov
        if cov:
            self.T.set_covariance(True)
        if prior:
            self.T.set_motion_prior(*SIGMAS)

    def push(self, bgr, depth):
        q, t, s = self.T.push_frame(bgr, depth)
        return dict(q=q, t=t, s=s, cov=self.T.last_covariance() if self.cov and s is not None else None)

    def close(self):
        self.T.close()


class _ManualRos:
    """stream i as a caller of the per-problem ROS producers drives it"""

    def __init__(self, hip, i, cam, dtype, halvings, cov, prior):
        self.hip, self.P, self.halvings = hip, hip.Problem(*cam, dtype=dtype), halvings
        _knobs(self.P, i)
        self.cov, self.prior, self.frames = cov, prior, 0
        self.q, self.t = IDENTITY

    def push(self, bgr, depth):
        hip, P = self.hip, self.P
        has_edge = True
        try:
            P.set_now_frame_ros(bgr, halvings=self.halvings)
        except hip.EAError as e:
            assert e.code == hip.EA_ERR_STATE, e
            has_edge = False
        s = cov = None
        if self.frames > 0 and P.num_points > 0 and has_edge:
            if self.prior:
                P.set_normal_prior(0, np.eye(4) / SIGMAS[0], self.q)
                P.set_normal_prior(1, np.eye(3) / SIGMAS[1], self.t)
            q, t, s = P.solve(self.q, self.t)
            if s["termination"] != hip.FAILURE:
                self.q, self.t = q, t
                if self.cov:
                    cov = P.covariance(q, t)
            elif self.cov:
                cov = dict(ok=False, why=4, tangent=np.zeros((6, 6)), eigenvalues=np.zeros(6))
        P.set_ref_frame_ros(bgr, depth, halvings=self.halvings)
        self.frames += 1
        return dict(q=self.q, t=self.t, s=s, cov=cov)

    def close(self):
        self.P.close()


def _compare_push(hip, tb, refs, bgr, depth, where, log=None, poses=None):
    """one push of the batch against one push of every reference -> the aligned flags"""
    q, t, sums, aligned = tb.push_frames(bgr, depth)
    if poses is not None:
        poses.append((q.copy(), t.copy()))
    assert tb.info("edge_passes") == 1, where                 # the shared frame: one N-frame edge-detection chain per push
    for i, R in enumerate(refs):
        w = R.push(bgr[i], depth[i])
        at = (where, "stream", i)
        assert bool(aligned[i]) == (w["s"] is not None), at
        assert np.array_equal(q[i], w["q"]) and np.array_equal(t[i], w["t"]), (at, q[i], w["q"], t[i], w["t"])
        if w["s"] is None:
            assert sums[i] is None, at
        else:
            for key in ("termination", "why", "num_iterations"):
                assert sums[i][key] == w["s"][key], (at, key, sums[i][key], w["s"][key])
            assert _bits(sums[i]["final_cost"], w["s"]["final_cost"]), (at, sums[i]["final_cost"], w["s"]["final_cost"])
            if log is not None:
                log.append((i, w["s"]["termination"], w["s"]["why"], w["s"]["num_iterations"]))
        got_p = tb.problem(i)
        assert got_p.num_points == R.P.num_points, (at, got_p.num_points, R.P.num_points)
        assert _bits(got_p.get_points(), R.P.get_points()), at
        gw, ww = got_p.get_weights(), R.P.get_weights()
        assert (gw is None) == (ww is None) and (gw is None or _bits(gw, ww)), at
        if w["cov"] is not None:
            c = tb.last_covariance(i)
            assert (c["ok"], c["why"]) == (w["cov"]["ok"], w["cov"]["why"]), (at, c["ok"], c["why"], w["cov"]["ok"], w["cov"]["why"])
            assert _bits(c["tangent"], w["cov"]["tangent"]) and _bits(c["eigenvalues"], w["cov"]["eigenvalues"]), at
        elif getattr(R, "cov", False):
            with pytest.raises(hip.EAError) as ei:
                tb.last_covariance(i)
            assert ei.value.code == hip.EA_ERR_STATE, at
    assert tb.info("aligned") == int(np.sum(aligned)), where
    return aligned


def _u16_depth(H, W, rng, low):
    """low = 0: the depths of the workspace-riding test of tests/test_gpu_preprocess.py -- values below 50 are points nearer
    than the functor's z guard (z = depth / 5000 < 0.01), which fail it: with enough points the solve ends in EA_FAILURE at
    the start; low = 500: every point valid"""
    d = rng.integers(low, 30000, (H, W)).astype(np.uint16)
    d[rng.random((H, W)) < 0.15] = 0
    return d


def _u16_pushes(H, W, n, pushes, seed, zero_depth=(), near_depth=()):
    """[(bgr x n, depth x n)] per push.  Stream 0: one scene a pixel further on per push; the others: noise and lines in turn.
    Stream 1 has the riding test's depths, the others valid ones.  zero_depth: (push, stream) pairs with an all-zero depth
    frame -- a reference without a point; near_depth: pairs whose depth is 10 everywhere -- every point fails its functor"""
    rng = np.random.default_rng(seed)
    scene = _random_frame(seed, H + pushes, W + pushes)
    out = []
    for k in range(pushes):
        bgr = [scene[k:k + H, k:k + W].copy()]
        for i in range(1, n):
            bgr.append(ros._frame(("noise", "lines")[(i + k) % 2], H, W, 0, rng)[0])
        depth = [np.zeros((H, W), np.uint16) if (k, i) in zero_depth else np.full((H, W), 10, np.uint16) if (k, i) in near_depth
                 else _u16_depth(H, W, rng, 0 if i == 1 else 500) for i in range(n)]
        out.append((bgr, depth))
    return out


def _clean_depth(H, W, rng):
    return (rng.random((H, W)) * 4.0 + 0.4).astype(np.float32)


def _ros_pushes(H, W, halvings, n, pushes, seed, flat=(), nan_depth=()):
    """the same for flavour 2, at the full extent: stream 0 a scene a pixel (of the full extent) further on per push, the
    others noise, lines and dot in turn; flat: (push, stream) pairs that receive a frame without any edge; nan_depth: pairs
    whose depth has zeros, negatives and NaN sprinkled in (the points of a NaN depth fail their functors)"""
    rng = np.random.default_rng(seed)
    s = 1 << halvings
    scene = _random_frame(seed, H * s + pushes, W * s + pushes)
    out = []
    for k in range(pushes):
        bgr = [scene[k:k + H * s, k:k + W * s].copy()]
        for i in range(1, n):
            kind = "flat" if (k, i) in flat else ("noise", "lines", "dot")[(i + k) % 3]
            bgr.append(ros._frame(kind, H, W, halvings, rng)[0])
        depth = [ros._depth(H * s, W * s, rng) if (k, i) in nan_depth else _clean_depth(H * s, W * s, rng) for i in range(n)]
        out.append((bgr, depth))
    return out


def _make(hip, n, H, W, dtype, flavour, halvings=0, cov=False, prior=False):
    cams = [ros._camera(i, H, W) for i in range(n)]
    tb = hip.TrackerBatch(cams, dtype=dtype, flavour=flavour, halvings=halvings)
    assert len(tb) == n
    for i in range(n):
        _knobs(tb.problem(i), i)
    if cov:
        tb.set_covariance(True)
    if prior:
        tb.set_motion_prior(*SIGMAS)
    if flavour == 2:
        refs = [_ManualRos(hip, i, cams[i], dtype, halvings, cov, prior) for i in range(n)]
    else:
        refs = [_SingleTracker(hip, i, cams[i], dtype, flavour, cov, prior) for i in range(n)]
    return tb, refs


@pytest.mark.parametrize("dtype_name", ["EA_F64", "EA_F32"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("flavour", [0, 1])
def test_laplacian_and_canny_streams_equal_single_trackers(hip, flavour, shape, dtype_name):
    """three streams, four pushes; stream 2 receives an all-zero depth frame at push 2, so its reference has no point and it
    is not aligned at push 3 (the other two are solved as a batch of their own) and aligned again at push 4"""
    (H, W), n = shape, 3
    tb, refs = _make(hip, n, H, W, getattr(hip, dtype_name), flavour)
    log = []
    try:
        flags = []
        for k, (bgr, depth) in enumerate(_u16_pushes(H, W, n, 4, 500 + 10 * flavour + H, zero_depth={(1, 2)})):
            flags.append([int(a) for a in _compare_push(hip, tb, refs, bgr, depth, (flavour, H, W, dtype_name, "push", k + 1), log)])
            assert tb.info("frames_without_edges") == 0
            assert (tb.info("hysteresis_rounds") >= 1) == (flavour == 1)
        print("TRACKER_BATCH flavour %d %dx%d %s: aligned %s, (stream, termination, why, iterations) %s"
              % (flavour, H, W, dtype_name, flags, log))
        assert flags == [[0, 0, 0], [1, 1, 1], [1, 1, 0], [1, 1, 1]]
        assert tb.problem(0).get_weights() is not None and tb.problem(1).get_weights() is None
    finally:
        ros._close(tb, refs)


@pytest.mark.parametrize("flavour", [0, 1])
def test_one_stream_equals_a_lone_tracker(hip, flavour):
    H, W = 37, 70
    tb, refs = _make(hip, 1, H, W, hip.EA_F64, flavour)
    try:
        flags = [int(_compare_push(hip, tb, refs, bgr, depth, (flavour, "push", k + 1))[0])
                 for k, (bgr, depth) in enumerate(_u16_pushes(H, W, 1, 3, 77 + flavour))]
        assert flags == [0, 1, 1]
    finally:
        ros._close(tb, refs)


@pytest.mark.parametrize("dtype_name", ["EA_F64", "EA_F32"])
@pytest.mark.parametrize("case", ROS_CASES, ids=lambda c: "%dx%d_h%d" % (c[0] + (c[1],)))
def test_ros_streams_equal_the_manual_loop(hip, case, dtype_name):
    """three streams, four pushes; stream 2 receives a frame without any edge at push 2: the push returns OK, the stream is
    not aligned and keeps its prior, its new reference is empty -- so it is not aligned at push 3 either -- and it is aligned
    again at push 4; the other streams are unaffected to the bit"""
    ((H, W), halvings), n = case, 3
    tb, refs = _make(hip, n, H, W, getattr(hip, dtype_name), 2, halvings=halvings)
    log = []
    try:
        flags, bare = [], []
        for k, (bgr, depth) in enumerate(_ros_pushes(H, W, halvings, n, 4, 900 + H + halvings, flat={(1, 2)})):
            prior = refs[2].q.copy(), refs[2].t.copy()
            flags.append([int(a) for a in _compare_push(hip, tb, refs, bgr, depth, (H, W, halvings, dtype_name, "push", k + 1), log)])
            bare.append(tb.info("frames_without_edges"))
            assert tb.info("hysteresis_rounds") >= 1
            if k == 1:
                assert tb.problem(2).num_points == 0
                assert np.array_equal(refs[2].q, prior[0]) and np.array_equal(refs[2].t, prior[1])
        print("TRACKER_BATCH ros %dx%d h%d %s: aligned %s, (stream, termination, why, iterations) %s"
              % (H, W, halvings, dtype_name, flags, log))
        assert flags == [[0, 0, 0], [1, 1, 0], [1, 1, 0], [1, 1, 1]] and bare == [0, 1, 0, 0]
    finally:
        ros._close(tb, refs)


@pytest.mark.parametrize("flavour", [0, 1, 2])
def test_covariance_and_motion_prior(hip, flavour):
    """covariance and motion prior on: every aligned stream's last_covariance equals the single tracker's (flavour 2: the
    manual loop's Problem.covariance under the same NormalPriors); a stream that was not aligned has none"""
    H, W, n = 37, 70, 3
    tb, refs = _make(hip, n, H, W, hip.EA_F64, flavour, cov=True, prior=True)
    try:
        pushes = (_ros_pushes(H, W, 0, n, 3, 41, flat={(1, 2)}) if flavour == 2 else
                  _u16_pushes(H, W, n, 3, 41 + flavour, zero_depth={(0, 2)}))
        flags = [list(_compare_push(hip, tb, refs, bgr, depth, (flavour, "push", k + 1))) for k, (bgr, depth) in enumerate(pushes)]
        assert flags == ([[0, 0, 0], [1, 1, 0], [1, 1, 0]] if flavour == 2 else [[0, 0, 0], [1, 1, 0], [1, 1, 1]])
        assert tb.last_covariance(0)["ok"]
        tb.set_covariance(False)
        with pytest.raises(hip.EAError):
            tb.last_covariance(0)
    finally:
        ros._close(tb, refs)


def test_reset_restarts_only_that_stream(hip):
    H, W, n, flavour = 37, 70, 3, 1
    tb, refs = _make(hip, n, H, W, hip.EA_F64, flavour)
    try:
        pushes = _u16_pushes(H, W, n, 4, 5)
        for k in range(2):
            _compare_push(hip, tb, refs, *pushes[k], where=("push", k + 1))
        tb.reset(1)
        assert tb.problem(1).num_points == 0 and tb.problem(0).num_points > 0
        refs[1].close()
        refs[1] = _SingleTracker(hip, 1, ros._camera(1, H, W), hip.EA_F64, flavour, False, False)   # a fresh chain
        flags = [list(_compare_push(hip, tb, refs, *pushes[k], where=("push", k + 1))) for k in (2, 3)]
        assert flags == [[1, 0, 1], [1, 1, 1]]
        tb.reset()
        q, t, sums, aligned = tb.push_frames(*pushes[0])
        assert not aligned.any() and sums == [None] * n
        assert np.array_equal(q, np.tile(IDENTITY[0], (n, 1))) and not t.any()
    finally:
        ros._close(tb, refs)


@pytest.mark.parametrize("flavour", [0, 1, 2])
def test_failed_solve_keeps_the_prior(hip, flavour):
    """Stream 0's second frame has a depth whose points fail their functors (nearer than the z guard; flavour 2: NaN): the
    solve of push 3 ends in EA_FAILURE at the start, and the stream keeps the prior push 2 gave it -- aligned all the same,
    covariance why = 4 -- while its neighbours go on; the single tracker (flavour 2: the manual loop) says the same."""
    H, W, n = 37, 70, 3
    tb, refs = _make(hip, n, H, W, hip.EA_F64, flavour, cov=True)
    try:
        pushes = (_ros_pushes(H, W, 0, n, 4, 63, nan_depth={(1, 0)}) if flavour == 2 else
                  _u16_pushes(H, W, n, 4, 63 + flavour, near_depth={(1, 0)}))
        log, after = [], []
        for k, (bgr, depth) in enumerate(pushes):
            aligned = _compare_push(hip, tb, refs, bgr, depth, (flavour, "push", k + 1), log if k == 2 else None, after)
            assert list(aligned) == [int(k > 0)] * n
        print("TRACKER_BATCH failed solve, flavour %d: push 3 (stream, termination, why, iterations) %s" % (flavour, log))
        assert dict((i, term) for i, term, _, _ in log)[0] == hip.FAILURE, log
        assert tb.last_covariance(0)["why"] in (0, 1, 2, 3)           # push 4 solved again
        assert np.array_equal(after[2][0][0], after[1][0][0]) and np.array_equal(after[2][1][0], after[1][1][0])
        assert not np.array_equal(after[1][0][0], IDENTITY[0])       # (a prior worth keeping)
    finally:
        ros._close(tb, refs)


@pytest.mark.parametrize("flavour,halvings", [(0, 0), (1, 0), (2, 0), (2, 1)])
def test_device_frames_equal_host_frames(hip, flavour, halvings):
    import torch
    H, W, n = 37, 70, 3
    cams = [ros._camera(i, H, W) for i in range(n)]
    host = hip.TrackerBatch(cams, dtype=hip.EA_F64, flavour=flavour, halvings=halvings)
    dev = hip.TrackerBatch(cams, dtype=hip.EA_F64, flavour=flavour, halvings=halvings)
    try:
        pushes = _ros_pushes(H, W, halvings, n, 3, 8) if flavour == 2 else _u16_pushes(H, W, n, 3, 8)
        for k, (bgr, depth) in enumerate(pushes):
            d_bgr = [torch.from_numpy(f).cuda() for f in bgr]
            d_depth = [torch.from_numpy(f if flavour == 2 else f.view(np.int16)).cuda() for f in depth]
            a, b = host.push_frames(bgr, depth), dev.push_frames(d_bgr, d_depth)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]), k
            assert list(a[3]) == [int(k > 0)] * n
            for i in range(n):
                assert (a[2][i] is None) == (b[2][i] is None), (k, i)
                if a[2][i] is not None:
                    assert a[2][i]["num_iterations"] == b[2][i]["num_iterations"], (k, i)
                    assert _bits(a[2][i]["final_cost"], b[2][i]["final_cost"]), (k, i)
                assert _bits(host.problem(i).get_points(), dev.problem(i).get_points()), (k, i)
                assert np.array_equal(host.problem(i).get_dt(), dev.problem(i).get_dt()), (k, i)
            assert dev.info("edge_passes") == 1
    finally:
        ros._close(host, dev)


def test_rejected_pushes_leave_the_tracker_as_it_was(hip):
    """every invalid argument of a push is refused before a stream is touched: the next push aligns as if nothing had been"""
    H, W, n = 37, 70, 2
    for flavour, halvings in ((1, 0), (2, 1)):
        s = 1 << halvings
        tb, refs = _make(hip, n, H, W, hip.EA_F64, flavour, halvings=halvings)
        try:
            pushes = _ros_pushes(H, W, halvings, n, 2, 3) if flavour == 2 else _u16_pushes(H, W, n, 2, 3)
            _compare_push(hip, tb, refs, *pushes[0], where="push 1")
            bgr, depth = pushes[1]
            bad = [((bgr[:1] + [None], depth), {}), ((bgr, [None] + depth[1:]), {})]
            bad.append((([f[:2 * s, :2 * s] for f in bgr], [f[:2 * s, :2 * s] for f in depth]), {}))   # a 2 x 2 working extent
            if flavour == 2:
                bad.append((([f[:-1] for f in bgr], [f[:-1] for f in depth]), {}))                     # not divisible by 2
            else:
                bad += [((bgr, depth), dict(z_scaling=0.0)), ((bgr, depth), dict(z_scaling=float("nan")))]
            for args, kw in bad:
                with pytest.raises(hip.EAError) as ei:
                    tb.push_frames(*args, **kw)
                assert ei.value.code == hip.EA_ERR_INVALID_ARG, ei.value
            # host memory handed to the _device form
            C, L = hip.C, hip.load()
            ptrs = [(C.c_void_p * n)(*[f.ctypes.data for f in side]) for side in (bgr, depth)]
            q, t = np.zeros((n, 4)), np.zeros((n, 3))
            assert L.ea_tracker_batch_push_frames_device(tb._h, ptrs[0], ptrs[1], H * s, W * s, 5000.0, None, hip._dp(q), hip._dp(t),
                                                         None, None) == hip.EA_ERR_INVALID_ARG
            assert b"device" in L.ea_last_error()
            assert list(_compare_push(hip, tb, refs, bgr, depth, where="push 2")) == [1] * n
        finally:
            ros._close(tb, refs)


def test_the_c_demo_prints_the_poses_of_the_python_class(hip, tmp_path):
    """examples/multi_tracker_demo (plain C99 on the C-ABI): three streams cut from the bundled frames, cropped to 120 x 160;
    its printed poses are TrackerBatch's on the same frames"""
    import os
    import subprocess
    from edge_alignment_amd import synth
    subprocess.check_call(["make", "-s", "-C", os.path.join(ros.ROOT, "examples"), "multi_tracker_demo"])
    frames = synth.load_bundled_frames(ros.G)
    H, W, y0, x0, nf = 120, 160, 100, 200, 5
    bgr = [np.ascontiguousarray(frames[k][0][y0:y0 + H, x0:x0 + W]) for k in range(1, nf + 1)]
    depth = [np.ascontiguousarray(frames[k][1][y0:y0 + H, x0:x0 + W]) for k in range(1, nf + 1)]
    cam = (ros.K[0], ros.K[1], ros.K[2] - x0, ros.K[3] - y0)
    np.stack(bgr).tofile(tmp_path / "bgr.u8")
    np.stack(depth).tofile(tmp_path / "depth.u16")
    out = subprocess.check_output([os.path.join(ros.ROOT, "examples", "multi_tracker_demo"), str(H), str(W)] + ["%r" % v for v in cam] +
                                  [str(nf), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16")], text=True).splitlines()
    assert len(out) == 3 * nf + 1
    tb = hip.TrackerBatch([cam] * 3, dtype=hip.EA_F64, flavour=1, loss=(hip.LOSS_CAUCHY, 1.0))
    try:
        for k in range(nf):
            pick = [k, nf - 1 - k, (k + 1) % nf]
            q, t, sums, aligned = tb.push_frames([bgr[i] for i in pick], [depth[i] for i in pick])
            for i in range(3):
                f = out[3 * k + i].split()
                assert [int(f[0]), int(f[1]), int(f[2])] == [k + 1, i, int(aligned[i])]
                assert np.array_equal(np.array(f[3:10], dtype=np.float64), np.concatenate([q[i], t[i]])), (k, i)
                assert int(f[10]) == (sums[i]["num_iterations"] if aligned[i] else 0)
        assert [int(v) for v in out[-1].split()] == [1, tb.info("hysteresis_rounds"), 3]
    finally:
        tb.close()


# ---- a camera of its own per stream, against the restatement ------------------------------------------------------------------

@pytest.mark.parametrize("flavour,halvings", [(0, 0), (1, 0), (2, 0), (2, 1)])
def test_per_stream_cameras_against_the_restatement(hip, flavour, halvings):
    """two streams with two different anisotropic, off-centre cameras, two pushes: the reference-side points of stream i are
    oracle/preprocess_np's with camera i, bit for bit; the solved pose is that of a hand-built Problem with camera i (and,
    for the Laplacian and Canny flavours, of the single Tracker) -- the equalities of _compare_push"""
    from oracle import preprocess_np as pp
    H, W = 37, 70
    cams = ros.AXES_CAMERAS
    s = 1 << halvings
    rng = np.random.default_rng(40 + flavour + halvings)
    scenes = [_random_frame(90 + 5 * i + flavour, H * s + 2, W * s + 2) for i in range(2)]
    tb = hip.TrackerBatch(cams, dtype=hip.EA_F64, flavour=flavour, halvings=halvings)
    hand = [hip.Problem(*cam, dtype=hip.EA_F64) for cam in cams]
    single = [hip.Tracker(*cam, dtype=hip.EA_F64, flavour=flavour) for cam in cams] if flavour < 2 else []
    try:
        for i in range(2):
            tb.problem(i).set_loss(hip.LOSS_CAUCHY, 1.0); hand[i].set_loss(hip.LOSS_CAUCHY, 1.0)
            if single:
                hip._StreamProblem(hip.load().ea_tracker_problem(single[i]._h), hip.EA_F64, 0).set_loss(hip.LOSS_CAUCHY, 1.0)
        for k in range(2):
            bgr = [sc[k:k + H * s, k:k + W * s].copy() for sc in scenes]
            depth = [_clean_depth(H * s, W * s, rng) if flavour == 2 else _u16_depth(H, W, rng, 500) for _ in range(2)]
            q, t, sums, aligned = tb.push_frames(bgr, depth)
            for i, cam in enumerate(cams):
                at = (flavour, halvings, "push", k + 1, "stream", i)
                P = hand[i]
                if k > 0:
                    if flavour == 2:
                        P.set_now_frame_ros(bgr[i], halvings=halvings)
                    else:
                        (P.set_now_frame if flavour == 0 else P.set_now_frame_canny)(bgr[i])
                    qm, tm, sm = P.solve(*IDENTITY)
                    assert aligned[i] and sm["termination"] != hip.FAILURE, at
                    assert sm["num_successful_steps"] > 0 and not np.array_equal(qm, IDENTITY[0]), at   # (a pose that moved)
                    assert np.array_equal(q[i], qm) and np.array_equal(t[i], tm), (at, q[i], qm, t[i], tm)
                    assert sums[i]["num_iterations"] == sm["num_iterations"] and _bits(sums[i]["final_cost"], sm["final_cost"]), at
                if flavour == 2:
                    P.set_ref_frame_ros(bgr[i], depth[i], halvings=halvings)
                else:
                    (P.set_ref_frame if flavour == 0 else P.set_ref_frame_canny)(bgr[i], depth[i])
                if flavour == 2:
                    want = ros._ros_restatement(pp, bgr[i], depth[i], halvings, cam)
                    swapped = ros._ros_restatement(pp, bgr[i], depth[i], halvings, (cam[1], cam[0], cam[2], cam[3]))
                else:
                    f = pp.get_aX if flavour == 0 else pp.get_aX_canny
                    want = f(bgr[i], depth[i], *cam)[0][:3].T
                    swapped = f(bgr[i], depth[i], cam[1], cam[0], cam[2], cam[3])[0][:3].T
                got = tb.problem(i).get_points()
                assert got.shape == want.shape and want.shape[0] > 50 and _bits(got, want), at
                assert not np.array_equal(swapped[:, 0], want[:, 0]) and not np.array_equal(swapped[:, 1], want[:, 1]), at
                if single:
                    qs, ts, ss = single[i].push_frame(bgr[i], depth[i])
                    assert np.array_equal(q[i], qs) and np.array_equal(t[i], ts), at
                    sp = hip._StreamProblem(hip.load().ea_tracker_problem(single[i]._h), hip.EA_F64, 0)
                    assert _bits(sp.get_points(), want), at
    finally:
        ros._close(tb, hand, single)
