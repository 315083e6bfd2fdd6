"""Keyframe mode of the multi-stream tracker (ea_tracker_batch_set_keyframes) against a manual loop per stream over the
per-problem API: set_now_frame* -> solve from the stored pose -> Problem.pose_stats -> the rule restated in Python
(tests/keyframe_rule.py) -> set_ref_frame* only when the rule replaces.  Compared with np.array_equal after every push:
poses, aligned flags, the summaries' termination / why / iterations / final-cost bits, the whole keyframe state (push index,
age, reason mask, statistics bits), every stream's points and weights -- and for a stream that kept its keyframe, points and
weights against what they were BEFORE the push.

Four streams with settings of their own (`_knobs` of tests/test_gpu_tracker_batch.py: streams 0 and 3 with depth weighting),
seven pushes of the `lenient` scenario:
  stream 0  one scene, still for three pushes, then a pixel further on per push
  stream 1  one scene, still: keeps its keyframe until max_frames replaces it
  stream 2  still; its first frame's depths put every point inside the z guard, so its first solve fails
            (EA_KEY_SOLVE_FAILED); flavour 2: a frame without any edge at push 4, while it holds a keyframe
  stream 3  still for three pushes, then another part of the scene
so that push 2 replaces some streams but not all, push 3 replaces nothing, and stream 1 keeps for three pushes running.
Three pushes of the `strict` scenario (every visible fraction below 1 replaces, every non-zero flow replaces) bring the
EA_KEY_VISIBLE, EA_KEY_INLIERS and EA_KEY_FLOW bits.  The test asserts all of this."""
import numpy as np
import pytest

import test_gpu_batch_frames_ros as ros
from keyframe_rule import KEY_AGE, KEY_FIRST, KEY_FLOW, KEY_INLIERS, KEY_SOLVE_FAILED, KEY_VISIBLE, keyframe_decide
from test_gpu_preprocess import _random_frame
from test_gpu_tracker_batch import IDENTITY, SIGMAS, _bits, _clean_depth, _knobs, _u16_depth

pytestmark = pytest.mark.gpu
N = 4
ZERO_STATS = dict(n=0, n_invalid=0, n_visible=0, n_inlier=0, n_flow=0, sum_flow=0.0)
LENIENT_OFFSETS = {0: (0, 0, 0, 1, 2, 3, 4), 1: (0,) * 7, 2: (0,) * 7, 3: (0, 0, 0, 14, 14, 14, 14)}
STRICT_OFFSETS = {0: (0, 1, 2), 1: (0,) * 3, 2: (0,) * 3, 3: (0, 0, 9)}
# (flavour, working shape, halvings)
CASES = [(0, (37, 70), 0), (0, (130, 257), 0), (1, (37, 70), 0), (1, (130, 257), 0), (2, (37, 70), 0), (2, (130, 257), 0),
         (2, (37, 70), 1)]


def _params(flavour, strict):
    unit = 255.0 if flavour == 2 else 1.0          # the DT of flavour 2 is in [0, 255]
    if strict:
        return dict(min_visible_fraction=1.0, min_inlier_fraction=1.0, inlier_residual=0.0, max_mean_flow=1e-12, max_frames=0, margin=2)
    if flavour == 0:
        # the Laplacian flavour's thresholded, median-filtered edge map does not put a still frame's own points on zeros of
        # its transform: on frames this small its solves wander by many pixels, so the lenient run leaves the flow and inlier
        # rules off (the strict run has them) and asks for a twentieth of the points in view
        return dict(min_visible_fraction=0.05, min_inlier_fraction=0.0, inlier_residual=0.1, max_mean_flow=0.0, max_frames=4, margin=0)
    return dict(min_visible_fraction=0.5, min_inlier_fraction=0.2, inlier_residual=0.1 * unit, max_mean_flow=8.0, max_frames=4, margin=0)


def _pushes(flavour, H, W, halvings, offsets, seed):
    """[(bgr x N, depth x N)] per push at the full extent; stream 2's first depth frame puts every point inside the guard,
    and (flavour 2) its fourth colour frame has no edge"""
    s = 1 << halvings
    rng = np.random.default_rng(seed)
    scenes = [_random_frame(seed + 17 * i, H * s + 24, W * s + 24) for i in range(N)]
    out = []
    for k in range(len(offsets[0])):
        bgr, depth = [], []
        for i in range(N):
            o = offsets[i][k]
            bgr.append(scenes[i][o:o + H * s, o:o + W * s].copy())
            if flavour == 2:
                depth.append(np.full((H * s, W * s), 0.001, np.float32) if (k, i) == (0, 2) else _clean_depth(H * s, W * s, rng))
            else:
                depth.append(np.full((H, W), 10, np.uint16) if (k, i) == (0, 2) else _u16_depth(H, W, rng, 500))
        if flavour == 2 and len(offsets[0]) > 3:
            bgr[2] = ros._frame("flat", H, W, halvings, rng)[0] if k == 3 else bgr[2]
        out.append((bgr, depth))
    return out


class _ManualKeyframes:
    """stream i as a caller of the per-problem API drives it"""

    def __init__(self, hip, i, cam, dtype, flavour, halvings, params, cov, prior):
        self.hip, self.P, self.flavour, self.halvings, self.params = hip, hip.Problem(*cam, dtype=dtype), flavour, halvings, params
        _knobs(self.P, i)
        self.cov, self.prior, self.frames = cov, prior, 0
        self.q, self.t = IDENTITY
        self.state = dict(keyframe_push=0, age=0, replaced=0, stats=dict(ZERO_STATS))

    def _now(self, bgr):
        """-> does the frame have an edge (flavour 2 leaves the image alone when it has none)"""
        if self.flavour == 0:
            self.P.set_now_frame(bgr)
        elif self.flavour == 1:
            self.P.set_now_frame_canny(bgr)
        else:
            try:
                self.P.set_now_frame_ros(bgr, halvings=self.halvings)
            except self.hip.EAError as e:
                assert e.code == self.hip.EA_ERR_STATE, e
                return False
        return True

    def _ref(self, bgr, depth):
        if self.flavour == 0:
            self.P.set_ref_frame(bgr, depth)
        elif self.flavour == 1:
            self.P.set_ref_frame_canny(bgr, depth)
        else:
            self.P.set_ref_frame_ros(bgr, depth, halvings=self.halvings)

    def push(self, bgr, depth, push_index):
        hip, P, prm = self.hip, self.P, self.params
        has_edge = self._now(bgr)
        aligned = self.frames > 0 and P.num_points > 0 and has_edge
        s = cov = None
        failed, stats = False, dict(ZERO_STATS)
        q_out, t_out = IDENTITY
        if aligned:
            if self.prior:
                P.set_normal_prior(0, np.eye(4) / SIGMAS[0], self.q)
                P.set_normal_prior(1, np.eye(3) / SIGMAS[1], self.t)
            q, t, s = P.solve(self.q, self.t)
            failed = s["termination"] == hip.FAILURE
            if failed:
                q_out, t_out = self.q, self.t
                cov = dict(ok=False, why=4, tangent=np.zeros((6, 6)), eigenvalues=np.zeros(6)) if self.cov else None
            else:
                q_out, t_out = q, t
                cov = P.covariance(q, t) if self.cov else None
                stats = P.pose_stats(q, t, margin=prm["margin"], inlier_residual=prm["inlier_residual"])
        # a frame without any edge keeps what the stream holds; everything else goes through the rule
        why = keyframe_decide(stats, prm, self.state["age"] + 1, aligned, failed) if has_edge else 0
        self.state["replaced"], self.state["stats"] = why, stats
        if why:
            self._ref(bgr, depth)
            self.q, self.t = IDENTITY
            self.state["age"], self.state["keyframe_push"] = 0, push_index
        elif aligned:
            self.q, self.t = q_out, t_out
            self.state["age"] += 1
        self.frames += 1
        return dict(q=q_out, t=t_out, s=s, cov=cov, why=why, aligned=aligned)

    def close(self):
        self.P.close()


def _make(hip, H, W, dtype, flavour, halvings, params, cov=False, prior=False):
    cams = [ros._camera(i, H, W) for i in range(N)]
    tb = hip.TrackerBatch(cams, dtype=dtype, flavour=flavour, halvings=halvings)
    for i in range(N):
        _knobs(tb.problem(i), i)
    if cov:
        tb.set_covariance(True)
    if prior:
        tb.set_motion_prior(*SIGMAS)
    assert tb.info("keyframe_mode") == 0
    tb.set_keyframes(**params)
    assert tb.info("keyframe_mode") == 1
    refs = [_ManualKeyframes(hip, i, cams[i], dtype, flavour, halvings, params, cov, prior) for i in range(N)]
    return tb, refs


def _held(P):
    w = P.get_weights()
    return P.num_points, P.get_points().copy(), None if w is None else w.copy()


def _same_state(got, want):
    return (got["keyframe_push"], got["age"], got["replaced"]) == (want["keyframe_push"], want["age"], want["replaced"]) and \
        all(got["stats"][k] == want["stats"][k] for k in ZERO_STATS if k != "sum_flow") and \
        _bits(got["stats"]["sum_flow"], want["stats"]["sum_flow"])


def _compare_push(hip, tb, refs, bgr, depth, push_index, where, device):
    """one push of the tracker against one push of every manual loop -> the reason masks"""
    before = [_held(tb.problem(i)) for i in range(N)]
    if device:
        import torch
        d_bgr = [torch.from_numpy(f).cuda() for f in bgr]
        d_depth = [torch.from_numpy(f if tb.flavour == 2 else f.view(np.int16)).cuda() for f in depth]
        q, t, sums, aligned = tb.push_frames(d_bgr, d_depth)
    else:
        q, t, sums, aligned = tb.push_frames(bgr, depth)
    assert tb.info("edge_passes") == 1 and tb.info("frames") == push_index, where
    whys = []
    for i, R in enumerate(refs):
        w = R.push(bgr[i], depth[i], push_index)
        at = (where, "stream", i)
        whys.append(w["why"])
        assert bool(aligned[i]) == w["aligned"] == (w["s"] is not None), at
        assert np.array_equal(q[i], w["q"]) and np.array_equal(t[i], w["t"]), (at, q[i], w["q"], t[i], w["t"])
        if w["s"] is None:
            assert sums[i] is None, at
        else:
            for key in ("termination", "why", "num_iterations"):
                assert sums[i][key] == w["s"][key], (at, key, sums[i][key], w["s"][key])
            assert _bits(sums[i]["final_cost"], w["s"]["final_cost"]), (at, sums[i]["final_cost"], w["s"]["final_cost"])
        st = tb.keyframe_state(i)
        assert _same_state(st, R.state), (at, st, R.state)
        got_p = tb.problem(i)
        assert got_p.num_points == R.P.num_points, (at, got_p.num_points, R.P.num_points)
        assert _bits(got_p.get_points(), R.P.get_points()), at
        gw, ww = got_p.get_weights(), R.P.get_weights()
        assert (gw is None) == (ww is None) and (gw is None or _bits(gw, ww)), at
        if w["why"] == 0:
            # a held reference: the bits it had before the push
            n0, p0, w0 = before[i]
            assert got_p.num_points == n0 and _bits(got_p.get_points(), p0), at
            assert (gw is None) == (w0 is None) and (gw is None or _bits(gw, w0)), at
        if w["cov"] is not None:
            c = tb.last_covariance(i)
            assert (c["ok"], c["why"]) == (w["cov"]["ok"], w["cov"]["why"]), at
            assert _bits(c["tangent"], w["cov"]["tangent"]) and _bits(c["eigenvalues"], w["cov"]["eigenvalues"]), at
        elif R.cov:
            with pytest.raises(hip.EAError) as ei:
                tb.last_covariance(i)
            assert ei.value.code == hip.EA_ERR_STATE, at
    assert tb.info("aligned") == int(np.sum(aligned)), where
    assert tb.info("keyframes_taken") == sum(1 for w in whys if w), (where, whys)
    return whys


def _run(hip, flavour, shape, halvings, dtype, device, strict, cov=False, prior=False):
    H, W = shape
    params = _params(flavour, strict)
    tb, refs = _make(hip, H, W, dtype, flavour, halvings, params, cov, prior)
    try:
        frames = _pushes(flavour, H, W, halvings, STRICT_OFFSETS if strict else LENIENT_OFFSETS, 4000 + 10 * flavour + H + halvings)
        log = [_compare_push(hip, tb, refs, bgr, depth, k + 1, (flavour, shape, halvings, device, strict, "push", k + 1), device)
               for k, (bgr, depth) in enumerate(frames)]
        bare = tb.info("frames_without_edges")
    finally:
        ros._close(tb, refs)
    return log, bare


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "f%d_%dx%d_h%d" % ((c[0],) + c[1] + (c[2],)))
def test_keyframe_pushes_equal_the_manual_loop(hip, case, device):
    flavour, shape, halvings = case
    log, _ = _run(hip, flavour, shape, halvings, hip.EA_F64, device, strict=False)
    strict_log, _ = _run(hip, flavour, shape, halvings, hip.EA_F64, device, strict=True)
    print("KEYFRAMES", case, "device" if device else "host", "lenient", log, "strict", strict_log)
    assert len(log) == 7 and len(strict_log) == 3
    assert log[0] == [KEY_FIRST] * N
    # stream 2's first keyframe has every point inside the guard: its solve fails; nothing else replaces in that push
    assert log[1][2] == KEY_SOLVE_FAILED and 0 < sum(1 for w in log[1] if w) < N
    assert any(all(w == 0 for w in push) for push in log[1:]), "no push kept every keyframe"
    keeps = ["".join("k" if push[i] == 0 else "r" for push in log) for i in range(N)]
    assert any("kkk" in s for s in keeps), keeps
    seen = 0
    for push in log + strict_log:
        for w in push:
            seen |= w
    assert seen == KEY_FIRST | KEY_SOLVE_FAILED | KEY_VISIBLE | KEY_INLIERS | KEY_FLOW | KEY_AGE, seen
    assert any(w & KEY_AGE for push in log for w in push)
    if flavour == 2:
        # push 4: stream 2's frame has no edge while it holds a keyframe -- kept, and not through the rule
        assert log[3][2] == 0


def test_fp32_streams_and_covariance_with_the_motion_prior(hip):
    """the lenient scenario once more in fp32, and in fp64 with covariance and the motion prior on (flavours 0 and 2)"""
    log, _ = _run(hip, 1, (37, 70), 0, hip.EA_F32, False, strict=False)
    assert log[0] == [KEY_FIRST] * N and log[1][2] == KEY_SOLVE_FAILED
    for flavour in (0, 2):
        log, bare = _run(hip, flavour, (37, 70), 0, hip.EA_F64, False, strict=False, cov=True, prior=True)
        assert log[0] == [KEY_FIRST] * N and log[1][2] == KEY_SOLVE_FAILED and bare == 0


def test_mode_switching_and_reset(hip):
    H, W = 37, 70
    params = _params(0, strict=False)
    tb, refs = _make(hip, H, W, hip.EA_F64, 0, 0, params)
    try:
        frames = _pushes(0, H, W, 0, LENIENT_OFFSETS, 77)
        for k in range(3):
            _compare_push(hip, tb, refs, frames[k][0], frames[k][1], k + 1, ("switch", k + 1), False)
        for call in (lambda: tb.set_keyframes(None), lambda: tb.set_keyframes(**params)):
            with pytest.raises(hip.EAError) as ei:
                call()                                   # a stream holds a reference
            assert ei.value.code == hip.EA_ERR_STATE
        for bad in (dict(margin=-1), dict(max_mean_flow=float("nan")), dict(inlier_residual=-1.0)):
            with pytest.raises(hip.EAError) as ei:
                tb.set_keyframes(**bad)
            assert ei.value.code == hip.EA_ERR_INVALID_ARG
        with pytest.raises(hip.EAError):
            tb.keyframe_state(N)
        # reset(i) clears stream i's state only
        states = [tb.keyframe_state(i) for i in range(N)]
        assert all(s["keyframe_push"] > 0 for s in states)
        tb.reset(1)
        refs[1].frames, refs[1].q, refs[1].t = 0, IDENTITY[0], IDENTITY[1]
        refs[1].state = dict(keyframe_push=0, age=0, replaced=0, stats=dict(ZERO_STATS))
        for i in range(N):
            assert _same_state(tb.keyframe_state(i), refs[i].state if i == 1 else states[i]), i
        assert tb.problem(1).num_points == 0 and tb.problem(0).num_points > 0
        with pytest.raises(hip.EAError) as ei:
            tb.set_keyframes(None)                       # the other streams still hold theirs
        assert ei.value.code == hip.EA_ERR_STATE
        why = _compare_push(hip, tb, refs, frames[3][0], frames[3][1], 4, ("switch", 4), False)
        assert why[1] == KEY_FIRST and tb.keyframe_state(1)["keyframe_push"] == 4
        tb.reset(-1)
        tb.set_keyframes(None)                           # accepted again
        assert tb.info("keyframe_mode") == 0
        with pytest.raises(hip.EAError) as ei:
            tb.keyframe_state(0)
        assert ei.value.code == hip.EA_ERR_STATE
        tb.set_keyframes(max_frames=2)
        assert tb.info("keyframe_mode") == 1 and tb.keyframe_state(0)["keyframe_push"] == 0
    finally:
        ros._close(tb, refs)
    cams = [[ros._camera(i, 36 >> l, 72 >> l) for i in range(2)] for l in range(2)]
    pyr = hip.TrackerBatch(cams, dtype=hip.EA_F64, flavour=2, levels=2)
    try:
        with pytest.raises(hip.EAError) as ei:
            pyr.set_keyframes()
        assert ei.value.code == hip.EA_ERR_STATE and "levels" in str(ei.value)
        pyr.set_keyframes(None)
    finally:
        pyr.close()


@pytest.mark.parametrize("flavour", [0, 2])
def test_switched_off_before_the_first_push_is_frame_to_frame(hip, flavour):
    H, W = 37, 70
    cams = [ros._camera(i, H, W) for i in range(N)]
    a = hip.TrackerBatch(cams, dtype=hip.EA_F64, flavour=flavour)
    b = hip.TrackerBatch(cams, dtype=hip.EA_F64, flavour=flavour)
    try:
        for tb in (a, b):
            for i in range(N):
                _knobs(tb.problem(i), i)
        b.set_keyframes(max_frames=3)
        b.set_keyframes(None)
        for k, (bgr, depth) in enumerate(_pushes(flavour, H, W, 0, LENIENT_OFFSETS, 31)[:5]):
            ra, rb = a.push_frames(bgr, depth), b.push_frames(bgr, depth)
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[3], rb[3]), k
            for i in range(N):
                assert (ra[2][i] is None) == (rb[2][i] is None)
                if ra[2][i] is not None:
                    assert ra[2][i]["num_iterations"] == rb[2][i]["num_iterations"] and _bits(ra[2][i]["final_cost"], rb[2][i]["final_cost"])
                assert a.problem(i).num_points == b.problem(i).num_points and _bits(a.problem(i).get_points(), b.problem(i).get_points())
            assert b.info("keyframes_taken") == 0 and b.info("keyframe_mode") == 0
            assert int(np.sum(ra[3])) == a.info("aligned") == b.info("aligned") and (k == 0 or ra[3][1] == 1)
    finally:
        a.close(); b.close()


def test_the_c_demo_prints_what_the_python_class_returns(hip, tmp_path):
    """examples/keyframe_tracker_demo (plain C99 on the C-ABI): the five bundled grabs cropped to 120 x 160 through one stream,
    frame to frame and in keyframe mode; the printed poses, statistics and reasons are TrackerBatch's on the same frames"""
    import os
    import subprocess
    from edge_alignment_amd import synth
    subprocess.check_call(["make", "-s", "-C", os.path.join(ros.ROOT, "examples"), "keyframe_tracker_demo"])
    frames = synth.load_bundled_frames(ros.G)
    H, W, y0, x0, nf = 120, 160, 100, 200, 5
    bgr = [np.ascontiguousarray(frames[k][0][y0:y0 + H, x0:x0 + W]) for k in range(1, nf + 1)]
    depth = [np.ascontiguousarray(frames[k][1][y0:y0 + H, x0:x0 + W]) for k in range(1, nf + 1)]
    cam = (ros.K[0], ros.K[1], ros.K[2] - x0, ros.K[3] - y0)
    np.stack(bgr).tofile(tmp_path / "bgr.u8")
    np.stack(depth).tofile(tmp_path / "depth.u16")
    out = subprocess.check_output([os.path.join(ros.ROOT, "examples", "keyframe_tracker_demo"), str(H), str(W)] + ["%r" % v for v in cam] +
                                  [str(nf), str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16")], text=True).splitlines()
    assert len(out) == 2 * nf
    for mode in (0, 1):
        tb = hip.TrackerBatch([cam], dtype=hip.EA_F64, flavour=1, loss=(hip.LOSS_CAUCHY, 1.0))
        try:
            if mode:
                tb.set_keyframes(min_inlier_fraction=0.5, inlier_residual=0.05, max_frames=3, margin=2)
            for k in range(nf):
                q, t, sums, aligned = tb.push_frames([bgr[k]], [depth[k]])
                f = out[mode * nf + k].split()
                assert [int(f[0]), int(f[1]), int(f[2])] == [mode, k + 1, int(aligned[0])]
                assert np.array_equal(np.array(f[12:19], dtype=np.float64), np.concatenate([q[0], t[0]])), (mode, k)
                st = tb.keyframe_state(0) if mode else dict(keyframe_push=0, age=0, replaced=0, stats=ZERO_STATS)
                assert [int(v) for v in f[3:8]] == [st["stats"][key] for key in ("n", "n_invalid", "n_visible", "n_inlier", "n_flow")]
                assert [int(f[9]), int(f[10]), int(f[11])] == [st["replaced"], st["keyframe_push"], st["age"]]
                if mode and k == 0:
                    assert st["replaced"] == KEY_FIRST and st["keyframe_push"] == 1
        finally:
            tb.close()
