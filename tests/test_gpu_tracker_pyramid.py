"""ea_tracker_batch_create_pyramid / TrackerBatch(levels=L): the multi-stream ROS tracker over L pyramid levels -- per push the
frames go up once, one halving chain gives every level its frame, every level's frame passes the edge detection once and
serves both sides, and every aligned stream is solved coarse to fine over its usable levels.  The reference is a per-stream
manual loop on problems of its own (`_ManualPyramid`, tests/test_gpu_tracker_batch.py's `_ManualRos` with levels): per level
set_now_frame_ros(halvings + l), then hip.solve_pyramid over the usable levels -- those whose reference has points and whose
frame has an edge -- from the stream's prior, then per level set_ref_frame_ros.  Everything is compared with np.array_equal
(floats through an integer view): aligned flags, poses, the returned summary and last_summaries (termination, why,
iterations, final-cost bits), every level's points, depth weights and image, covariances.

Four streams of different kinds and cameras (stream 0: a scene a pixel further on per push; noise, lines, dot in turn for the
others), each level's problems with the settings of `_knobs` (one family with depth weighting, one auto-scaled, one with a
constant mask), four pushes.  All in fp64, the first two in fp32 as well.  Cases of (full extent, halvings, levels): ((74, 140), 0, 2), ((296, 560), 1, 3),
((272, 1040), 1, 3) -- level 0 wider than a row block -- and ((24, 48), 0, 4), down to 3 x 6, where only the scene of stream 0 has an edge left."""
import numpy as np
import pytest

import test_gpu_batch_frames_ros as ros
from test_gpu_tracker_batch import IDENTITY, SIGMAS, _bits, _knobs, _ros_pushes

pytestmark = pytest.mark.gpu
CASES = (((74, 140), 0, 2), ((296, 560), 1, 3), ((272, 1040), 1, 3), ((24, 48), 0, 4))
N = 4


def _id(c):
    return "%dx%d_h%d_l%d" % (c[0] + c[1:])


PARAMS = [(c, "EA_F64") for c in CASES] + [(c, "EA_F32") for c in CASES[:2]]


def _image(hip, P):
    """the problem's image, None while it has none (a level whose frames never had an edge)"""
    try:
        return P.get_dt()
    except hip.EAError as e:
        assert e.code == hip.EA_ERR_STATE, e
        return None


def _state(hip, P):
    return dict(n=P.num_points, points=P.get_points(), weights=P.get_weights(), dt=_image(hip, P))


def _cams(full, halvings, levels, n=N):
    return [[ros._camera(i, full[0] >> (halvings + l), full[1] >> (halvings + l)) for i in range(n)] for l in range(levels)]


class _ManualPyramid:
    """stream i as a caller of the per-problem ROS producers and ea_solve_pyramid drives it"""

    def __init__(self, hip, i, cams, dtype, halvings, cov, prior):
        self.hip, self.halvings = hip, halvings
        self.Ps = [hip.Problem(*lv[i], dtype=dtype) for lv in cams]
        for P in self.Ps:
            _knobs(P, i)
        self.cov, self.prior, self.frames = cov, prior, 0
        self.q, self.t = IDENTITY

    def push(self, bgr, depth):
        hip, L = self.hip, len(self.Ps)
        edge = []
        for l, P in enumerate(self.Ps):
            try:
                P.set_now_frame_ros(bgr, halvings=self.halvings + l)
                edge.append(True)
            except hip.EAError as e:
                assert e.code == hip.EA_ERR_STATE, e
                edge.append(False)
        usable = [l for l in range(L) if self.Ps[l].num_points > 0 and edge[l]]
        s = cov = None
        sums = [None] * L
        if self.frames > 0 and 0 in usable:
            if self.prior:
                for l in usable:
                    self.Ps[l].set_normal_prior(0, np.eye(4) / SIGMAS[0], self.q)
                    self.Ps[l].set_normal_prior(1, np.eye(3) / SIGMAS[1], self.t)
            q, t, ss = hip.solve_pyramid([self.Ps[l] for l in usable], self.q, self.t)
            failed = False
            for k in range(len(usable) - 1, -1, -1):          # coarsest first; behind a failed level nothing was solved
                sums[usable[k]] = s = ss[k]
                if ss[k]["termination"] == hip.FAILURE:
                    failed = True
                    break
            if not failed:
                self.q, self.t = q, t
                if self.cov:
                    cov = self.Ps[0].covariance(q, t)
            elif self.cov:
                cov = dict(ok=False, why=4, tangent=np.zeros((6, 6)), eigenvalues=np.zeros(6))
        for l, P in enumerate(self.Ps):
            P.set_ref_frame_ros(bgr, depth, halvings=self.halvings + l)
        self.frames += 1
        return dict(q=self.q, t=self.t, s=s, sums=sums, cov=cov, usable=usable)

    def close(self):
        for P in self.Ps:
            P.close()


def _make(hip, full, halvings, levels, dtype, cov=False, prior=False, n=N):
    cams = _cams(full, halvings, levels, n)
    tb = hip.TrackerBatch(cams, dtype=dtype, flavour=2, halvings=halvings, levels=levels)
    assert len(tb) == n and tb.info("levels") == levels
    for l in range(levels):
        for i in range(n):
            _knobs(tb.level_problem(l, i), i)
    if cov:
        tb.set_covariance(True)
    if prior:
        tb.set_motion_prior(*SIGMAS)
    return tb, [_ManualPyramid(hip, i, cams, dtype, halvings, cov, prior) for i in range(n)]


def _same_summary(a, b, at):
    assert (a is None) == (b is None), (at, a is None, b is None)
    if a is not None:
        for key in ("termination", "why", "num_iterations"):
            assert a[key] == b[key], (at, key, a[key], b[key])
        assert _bits(a["final_cost"], b["final_cost"]), (at, a["final_cost"], b["final_cost"])


def _compare_push(hip, tb, refs, bgr, depth, where, log=None):
    q, t, sums, aligned = tb.push_frames(bgr, depth)
    assert tb.info("edge_passes") == tb.levels, where
    for i, R in enumerate(refs):
        w = R.push(bgr[i], depth[i])
        at = (where, "stream", i)
        assert bool(aligned[i]) == (w["s"] is not None), (at, aligned[i], w["usable"])
        assert np.array_equal(q[i], w["q"]) and np.array_equal(t[i], w["t"]), (at, q[i], w["q"], t[i], w["t"])
        _same_summary(sums[i], w["s"], at)
        last = tb.last_summaries(i)
        for l in range(tb.levels):
            _same_summary(last[l], w["sums"][l], at + ("level", l))
            got_p, want_p = tb.level_problem(l, i), R.Ps[l]
            ros._assert_same(_state(hip, got_p), _state(hip, want_p), at + ("level", l))
        if log is not None:
            log.append((i, w["usable"], [None if x is None else (x["termination"], x["num_iterations"]) for x in w["sums"]]))
        if w["cov"] is not None:
            c = tb.last_covariance(i)
            assert (c["ok"], c["why"]) == (w["cov"]["ok"], w["cov"]["why"]), (at, c["ok"], c["why"], w["cov"]["ok"], w["cov"]["why"])
            assert _bits(c["tangent"], w["cov"]["tangent"]) and _bits(c["eigenvalues"], w["cov"]["eigenvalues"]), at
        elif R.cov:
            with pytest.raises(hip.EAError) as ei:
                tb.last_covariance(i)
            assert ei.value.code == hip.EA_ERR_STATE, at
    assert tb.info("aligned") == int(np.sum(aligned)), where
    return [int(a) for a in aligned]


def _close(tb, refs):
    ros._close(tb, refs)


@pytest.mark.parametrize("case,dtype_name", PARAMS, ids=lambda v: v if isinstance(v, str) else _id(v))
def test_streams_equal_the_manual_pyramid_loop(hip, case, dtype_name):
    """stream 2 receives a frame without any edge at push 2: not aligned there (its images are left alone on every level) nor,
    with an empty reference, at push 3; aligned again at push 4"""
    full, halvings, levels = case
    H, W = full[0] >> halvings, full[1] >> halvings
    tb, refs = _make(hip, full, halvings, levels, getattr(hip, dtype_name))
    try:
        flags, log = [], []
        for k, (bgr, depth) in enumerate(_ros_pushes(H, W, halvings, N, 4, 900 + H + halvings, flat={(1, 2)})):
            images = [_image(hip, tb.level_problem(l, 2)) for l in range(levels)] if k == 1 else None
            flags.append(_compare_push(hip, tb, refs, bgr, depth, (_id(case), dtype_name, "push", k + 1), log))
            if k == 1:
                assert tb.info("frames_without_edges") == 1
                assert images[0] is not None
                for l in range(levels):
                    now = _image(hip, tb.level_problem(l, 2))
                    assert (now is None) == (images[l] is None) and (now is None or np.array_equal(now, images[l])), l
                assert all(tb.level_problem(l, 2).num_points == 0 for l in range(levels))
        print("TRACKER_PYRAMID %s %s: aligned %s, (stream, usable levels, (termination, iterations) per level) %s"
              % (_id(case), dtype_name, flags, log))
        assert flags == [[0, 0, 0, 0], [1, 1, 0, 1], [1, 1, 0, 1], [1, 1, 1, 1]]
        solved = [entry for entry in log if entry[2][0] is not None]
        assert any(all(x is not None for x in s) for _, _, s in solved)         # a descent over every level
        if levels >= 3:
            # averaged noise, lines and the dot lose their edges on the coarsest levels: such a stream skips the levels it
            # cannot use and is solved on the ones below
            assert any(levels - 1 not in u and s[levels - 1] is None and s[levels - 2] is not None for _, u, s in solved)
    finally:
        _close(tb, refs)


def test_covariance_and_motion_prior(hip):
    full, halvings, levels = (74, 140), 0, 2
    tb, refs = _make(hip, full, halvings, levels, hip.EA_F64, cov=True, prior=True)
    try:
        pushes = _ros_pushes(full[0], full[1], halvings, N, 3, 41, flat={(1, 2)}, nan_depth={(0, 1)})
        flags = [_compare_push(hip, tb, refs, bgr, depth, ("cov", "push", k + 1)) for k, (bgr, depth) in enumerate(pushes)]
        assert flags == [[0, 0, 0, 0], [1, 1, 0, 1], [1, 1, 0, 1]]
        assert tb.last_covariance(0)["ok"]
        tb.set_covariance(False)
        with pytest.raises(hip.EAError):
            tb.last_covariance(0)
    finally:
        _close(tb, refs)


def test_failed_descent_keeps_the_prior(hip):
    """A descent that stops above level 0.  The input is the single-level test_failed_solve_keeps_the_prior's -- stream 0's
    second frame has zeros, negatives and NaN sprinkled into its depth -- with that frame's NaN replaced by +inf: at full
    extent and halvings 0 the NaN fails level 0 alone (measured: level 1 solved in 39 iterations, level 0 FAILURE), because
    the halving step that makes level 1 turns NaN into 0; an infinite depth passes it, its 2 x 2 mean is infinite, and a
    point at infinity projects to NaN on every level.  So the solve of push 3 ends in EA_FAILURE on the coarsest level, which
    the descent reaches first: nothing is solved below it, the stream keeps the prior push 2 gave it -- aligned all the
    same, covariance why = 4 -- and is solved again at push 4, while its neighbours go on; the manual loop says the same."""
    full, halvings, levels = (74, 140), 0, 2
    tb, refs = _make(hip, full, halvings, levels, hip.EA_F64, cov=True)
    try:
        pushes = _ros_pushes(full[0], full[1], halvings, N, 4, 63, nan_depth={(1, 0)})
        spoiled = pushes[1][1][0]
        assert np.isnan(spoiled).any()
        spoiled[np.isnan(spoiled)] = np.inf
        logs, poses = [], []
        for k, (bgr, depth) in enumerate(pushes):
            logs.append([])
            aligned = _compare_push(hip, tb, refs, bgr, depth, ("failed descent", "push", k + 1), logs[-1])
            assert aligned == [int(k > 0)] * N
            poses.append((refs[0].q.copy(), refs[0].t.copy()))       # (_compare_push: the poses the push returned)
            if k == 2:
                assert tb.last_covariance(0)["why"] == 4
        print("TRACKER_PYRAMID failed descent: (stream, usable levels, (termination, iterations) per level) per push %s" % logs)
        stream, usable, per_level = logs[2][0]
        first = max(usable)                                           # the level the descent reached first
        assert stream == 0 and first == levels - 1 and per_level[first][0] == hip.FAILURE, logs[2]
        assert all(per_level[l] is None for l in range(first)), logs[2]
        assert np.array_equal(poses[2][0], poses[1][0]) and np.array_equal(poses[2][1], poses[1][1])
        assert not np.array_equal(poses[2][0], IDENTITY[0])          # (a prior worth keeping)
        assert all(x is not None and x[0] != hip.FAILURE for x in logs[3][0][2]), logs[3]      # push 4: solved again
        assert tb.last_covariance(0)["why"] in (0, 1, 2, 3)
    finally:
        _close(tb, refs)


def test_levels_one_equals_the_single_level_tracker(hip):
    full, halvings, n = (74, 140), 1, 3
    H, W = full[0] >> halvings, full[1] >> halvings
    cams = _cams(full, halvings, 1, n)
    a = hip.TrackerBatch(cams, dtype=hip.EA_F64, flavour=2, halvings=halvings, levels=1)      # ea_tracker_batch_create_pyramid
    b = hip.TrackerBatch(cams[0], dtype=hip.EA_F64, flavour=2, halvings=halvings)             # ea_tracker_batch_create
    try:
        for tb in (a, b):
            for i in range(n):
                _knobs(tb.problem(i), i)
        for k, (bgr, depth) in enumerate(_ros_pushes(H, W, halvings, n, 3, 17)):
            ra, rb = a.push_frames(bgr, depth), b.push_frames(bgr, depth)
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[3], rb[3]), k
            assert list(ra[3]) == [int(k > 0)] * n and a.info("edge_passes") == 1 and a.info("levels") == 1
            for i in range(n):
                _same_summary(ra[2][i], rb[2][i], (k, i))
                _same_summary(a.last_summaries(i)[0], rb[2][i], (k, i, "last"))
                _same_summary(b.last_summaries(i)[0], rb[2][i], (k, i, "last of the single-level tracker"))
                ros._assert_same(_state(hip, a.problem(i)), _state(hip, b.problem(i)), (k, i))
    finally:
        ros._close(a, b)


def test_reset_restarts_only_that_stream(hip):
    full, halvings, levels = (74, 140), 0, 2
    tb, refs = _make(hip, full, halvings, levels, hip.EA_F64)
    try:
        pushes = _ros_pushes(full[0], full[1], halvings, N, 4, 5)
        for k in range(2):
            _compare_push(hip, tb, refs, *pushes[k], where=("push", k + 1))
        tb.reset(1)
        assert all(tb.level_problem(l, 1).num_points == 0 for l in range(levels)) and tb.level_problem(1, 0).num_points > 0
        refs[1].close()
        refs[1] = _ManualPyramid(hip, 1, _cams(full, halvings, levels), hip.EA_F64, halvings, False, False)   # a fresh chain
        # (the fresh reference starts from images of its own: compare points and poses, not the never-set images, at push 3)
        flags = [_compare_push(hip, tb, refs, *pushes[k], where=("push", k + 1)) for k in (2, 3)]
        assert flags == [[1, 0, 1, 1], [1, 1, 1, 1]]
        tb.reset()
        q, t, sums, aligned = tb.push_frames(*pushes[0])
        assert not aligned.any() and sums == [None] * N and all(tb.last_summaries(i) == [None] * levels for i in range(N))
        assert np.array_equal(q, np.tile(IDENTITY[0], (N, 1))) and not t.any()
    finally:
        _close(tb, refs)


def test_rejected_pushes_leave_the_tracker_as_it_was(hip):
    full, halvings, levels = (72, 144), 1, 2                     # divisible by 8, not by 16; level 1 is 18 x 36
    H, W = full[0] >> halvings, full[1] >> halvings
    tb, refs = _make(hip, full, halvings, levels, hip.EA_F64, n=2)
    try:
        pushes = _ros_pushes(H, W, halvings, 2, 2, 3)
        _compare_push(hip, tb, refs, *pushes[0], where="push 1")
        bgr, depth = pushes[1]
        bad = [(bgr[:1] + [None], depth), (bgr, [None] + depth[1:]),
               ([f[:8, :16] for f in bgr], [f[:8, :16] for f in depth]),       # a coarsest level of 2 x 4
               ([f[:-2] for f in bgr], [f[:-2] for f in depth]),               # 70 rows: not divisible by 4
               ([f[:-4, :-4] for f in bgr], [f[:-4, :-4] for f in depth][:1])]  # a wrong count
        for args in bad:
            with pytest.raises(hip.EAError) as ei:
                tb.push_frames(*args)
            assert ei.value.code == hip.EA_ERR_INVALID_ARG, ei.value
        C, L = hip.C, hip.load()
        ptrs = [(C.c_void_p * 2)(*[f.ctypes.data for f in side]) for side in (bgr, depth)]
        q, t = np.zeros((2, 4)), np.zeros((2, 3))
        assert L.ea_tracker_batch_push_frames_device(tb._h, ptrs[0], ptrs[1], full[0], full[1], 5000.0, None, hip._dp(q), hip._dp(t),
                                                     None, None) == hip.EA_ERR_INVALID_ARG
        assert _compare_push(hip, tb, refs, bgr, depth, where="push 2") == [1, 1]
        # creation: levels and halvings out of range, a flavour without levels
        for kw in (dict(levels=0), dict(levels=9, halvings=1)):
            with pytest.raises(hip.EAError) as ei:
                hip.TrackerBatch(_cams(full, 0, max(kw["levels"], 1), 2), flavour=2, **kw)
            assert ei.value.code == hip.EA_ERR_INVALID_ARG, kw
        assert L.ea_tracker_batch_level_problem(tb._h, levels, 0) is None and L.ea_tracker_batch_level_problem(tb._h, 1, 2) is None
        assert L.ea_tracker_batch_level_problem(tb._h, 0, 1) == L.ea_tracker_batch_problem(tb._h, 1)
    finally:
        _close(tb, refs)


def test_device_frames_equal_host_frames(hip):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch has no device")
    full, halvings, levels, n = (74, 140), 0, 2, 3
    cams = _cams(full, halvings, levels, n)
    host = hip.TrackerBatch(cams, flavour=2, halvings=halvings, levels=levels)
    dev = hip.TrackerBatch(cams, flavour=2, halvings=halvings, levels=levels)
    try:
        for k, (bgr, depth) in enumerate(_ros_pushes(full[0], full[1], halvings, n, 3, 8)):
            d_bgr, d_depth = [torch.from_numpy(f).cuda() for f in bgr], [torch.from_numpy(f).cuda() for f in depth]
            a, b = host.push_frames(bgr, depth), dev.push_frames(d_bgr, d_depth)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[3], b[3]), k
            assert list(a[3]) == [int(k > 0)] * n and dev.info("edge_passes") == levels
            for i in range(n):
                _same_summary(a[2][i], b[2][i], (k, i))
                for l in range(levels):
                    ros._assert_same(_state(hip, host.level_problem(l, i)), _state(hip, dev.level_problem(l, i)), (k, i, l))
    finally:
        ros._close(host, dev)


def test_the_c_demo_prints_the_poses_and_level_iterations_of_the_python_class(hip, tmp_path):
    """examples/pyramid_tracker_demo (plain C99 on the C-ABI): two streams x three levels from the bundled frames, cropped to
    192 x 256 and halved once; its printed poses and per-level iteration counts are TrackerBatch's on the same frames"""
    import os
    import subprocess
    from edge_alignment_amd import synth
    subprocess.check_call(["make", "-s", "-C", os.path.join(ros.ROOT, "examples"), "pyramid_tracker_demo"])
    frames = synth.load_bundled_frames(ros.G)
    H, W, y0, x0, nf, halvings, levels = 192, 256, 100, 200, 4, 1, 3
    bgr = [np.ascontiguousarray(frames[k][0][y0:y0 + H, x0:x0 + W]) for k in range(1, nf + 1)]
    depth = [np.ascontiguousarray(frames[k][1][y0:y0 + H, x0:x0 + W].astype(np.float32) / np.float32(5000.0)) for k in range(1, nf + 1)]
    cam = (ros.K[0], ros.K[1], ros.K[2] - x0, ros.K[3] - y0)
    np.stack(bgr).tofile(tmp_path / "bgr.u8")
    np.stack(depth).tofile(tmp_path / "depth.f32")
    out = subprocess.check_output([os.path.join(ros.ROOT, "examples", "pyramid_tracker_demo"), str(H), str(W)] + ["%r" % v for v in cam] +
                                  [str(halvings), str(nf), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.f32")], text=True).splitlines()
    assert len(out) == 2 * nf + 1
    cams = [[tuple(v / (1 << (halvings + l)) for v in cam)] * 2 for l in range(levels)]
    tb = hip.TrackerBatch(cams, dtype=hip.EA_F64, flavour=2, halvings=halvings, levels=levels)
    try:
        for l in range(levels):
            for i in range(2):
                tb.level_problem(l, i).set_loss(hip.LOSS_CAUCHY, 1.0)
        for k in range(nf):
            pick = [k, nf - 1 - k]
            q, t, sums, aligned = tb.push_frames([bgr[i] for i in pick], [depth[i] for i in pick])
            for i in range(2):
                f = out[2 * k + i].split()
                assert [int(f[0]), int(f[1]), int(f[2])] == [k + 1, i, int(aligned[i])]
                assert np.array_equal(np.array(f[3:10], dtype=np.float64), np.concatenate([q[i], t[i]])), (k, i)
                last = tb.last_summaries(i)
                assert [int(v) for v in f[10:13]] == [-1 if s is None else s["num_iterations"] for s in last], (k, i, f[10:13])
        print("pyramid_tracker_demo, last push:", out[-3:])
        assert [int(v) for v in out[-1].split()] == [levels, levels, 2]
    finally:
        tb.close()
