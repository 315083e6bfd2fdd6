"""The depth gate on a depth image of 2^s times the DT extent (step 3b of include/ea_hip.h) through the public calls, and the
gate inside the multi-stream tracker (ea_tracker_batch_set_depth_gate).  Exactness is the requirement, as in
tests/test_gpu_depth_gate.py and tests/test_gpu_tracker_batch.py: class bytes, counts and weight bits equal the numpy
restatement (tests/depth_gate_scaled_ref.py), and a gated tracker equals the manual loop -- per push a Batch over fresh problems
that takes set_frames[_canny|_ros] (reference = frame k - 1, current = frame k), set_now_depth with frame k's full-resolution
depth, depth_gate at the tracker's start poses and solve from them -- in poses, summaries and counts, np.array_equal.

Shapes: frames of 64 x 48 for flavours 0 and 1, 128 x 96 halved once for flavour 2, two pyramid levels on top of that (the
coarsest 32 x 24); three streams, four pushes.  The scenes are the generators of tests/test_gpu_tracker_batch.py; from push 2
on streams 0 and 1 get a rectangle of another colour and a nearer depth painted over part of the frame, moved and brought
nearer with every push; stream 2 is untouched and starts a push late (its first reference has no point).  Settings per stream
are `_knobs` (stream 0 with depth weighting)."""
import os
import subprocess

import numpy as np
import pytest

import depth_gate_cases as dc
import depth_gate_ref as dg
import depth_gate_scaled_ref as ds
import test_gpu_batch_frames_ros as ros
from test_gpu_depth_gate import FACTORS, _dtype, _problem
from test_gpu_tracker_batch import _knobs, _ros_pushes, _u16_pushes

pytestmark = pytest.mark.gpu
N = 3
Z = 5000.0
RULE = dict(radius=1, abs_tol=0.05, rel_tol=0.02)
GATE = dict(w_occluded=0.0, w_free=0.25, w_unknown=0.5, **RULE)
# name: flavour, halvings, levels, full extent (H, W)
CONFIGS = {"laplacian": (0, 0, 1, (48, 64)), "canny": (1, 0, 1, (48, 64)), "ros_h0": (2, 0, 1, (48, 64)),
           "ros_h1": (2, 1, 1, (96, 128)), "pyramid": (2, 1, 2, (96, 128))}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- 1: the scaled gate through the public calls ------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_scaled_gate_through_the_public_calls(hip, kind, dtype_name):
    import torch
    f32 = dtype_name == "f32"
    im = dc.SMALL
    for s, T in ((1, dc.MATRICES["rigid"]), (1, dc.MATRICES["identity"]), (2, dc.MATRICES["rigid"])):
        depth = ds.depth_image(im, s, kind)
        for n in (65, 257):
            for variant in ("plain", "distortion"):
                P = _problem(hip, im, variant, ds.points(n, 40 + n, im), _dtype(hip, dtype_name), depth)
                B = hip.Batch([P])
                pts = P.get_points()
                dist = dc.DIST if variant == "distortion" else None
                for radius in (0, 3):
                    where = (s, kind, dtype_name, n, variant, radius)
                    want = ds.classify(pts, dc.matrix_for(variant, T), im["K"], depth, s, dc.Z_SCALING, radius, dist=dist, **dc.TOL)
                    cls, stats = P.depth_gate(T, radius=radius, **dc.TOL, **FACTORS)
                    assert np.array_equal(cls, want), where + (np.flatnonzero(cls != want)[:8],)
                    assert stats == dg.stats(want), where
                    ww = dg.weights(want, pts[:, 2], f32=f32, **FACTORS)
                    assert np.array_equal(_bits(P.get_weights()), _bits(ww)), where
                    P.set_weights(None)
                    bcls, bstats = B.depth_gate(T[None], radius=radius, **dc.TOL, **FACTORS)
                    assert np.array_equal(bcls, want) and bstats == [dg.stats(want)], where
                    assert np.array_equal(_bits(P.get_weights()), _bits(ww)), where
                    P.set_weights(None)
                    dev = torch.full((n,), 99, dtype=torch.uint8, device="cuda")
                    assert B.depth_gate_device(T[None], dev, radius=radius, **dc.TOL, **FACTORS) == [dg.stats(want)], where
                    assert np.array_equal(dev.cpu().numpy(), want), where
                    assert np.array_equal(_bits(P.get_weights()), _bits(ww)), where
                    P.set_weights(None)
                    if T is dc.MATRICES["identity"] and variant == "plain":
                        assert (np.bincount(want, minlength=6) > 0).all(), where     # no class is vacuous on the device either
                B.close()
                P.close()


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_a_batch_mixes_shifts_and_refuses_other_extents(hip, kind):
    im = dc.SMALL
    H, W = im["H"], im["W"]
    depths = [ds.depth_image(im, s, kind) for s in (0, 1, 0, 2)]
    Ps = [_problem(hip, im, "plain", ds.points(n, 70 + n, im), hip.EA_F64, d) for n, d in zip((65, 257, 257, 64), depths)]
    B = hip.Batch(Ps)
    Ts = np.stack([dc.MATRICES[k] for k in ("identity", "rigid", "rigid", "identity")])
    cls, stats = B.depth_gate(Ts, radius=1, apply=0, **dc.TOL)
    off = B.row_offsets()
    for i, (P, s) in enumerate(zip(Ps, (0, 1, 0, 2))):
        want = ds.classify(P.get_points(), Ts[i][:3], im["K"], depths[i], s, dc.Z_SCALING, 1, **dc.TOL)
        assert np.array_equal(cls[off[i]:off[i] + P.num_points], want) and stats[i] == dg.stats(want), i
    zeros = np.zeros if kind == "f32" else (lambda shape, dt: np.full(shape, 1024, dt))
    dt = np.float32 if kind == "f32" else np.uint16
    for shape in ((H + 1, W), (2 * H, W), (3 * H, 3 * W), (H, 2 * W)):
        Ps[1].set_now_depth(zeros(shape, dt), dc.Z_SCALING)                    # accepted by the setter,
        for call in (lambda: Ps[1].depth_gate(Ts[1]), lambda: B.depth_gate(Ts), lambda: B.depth_gate_device(Ts, None)):
            with pytest.raises(hip.EAError) as ei:                             # refused at gate time
                call()
            assert ei.value.code == hip.EA_ERR_STATE, shape
        assert all(P.get_weights() is None for P in Ps), shape
    B.close()
    for P in Ps:
        P.close()


# ---- the tracker's scenes and the manual loop -----------------------------------------------------------------------------------

def _pushes(cfg, seed, pushes=4, late=True):
    flavour, halvings, levels, (FH, FW) = cfg
    if flavour == 2:
        out = _ros_pushes(FH >> halvings, FW >> halvings, halvings, N, pushes, seed, flat={(0, 2)} if late else ())
    else:
        out = _u16_pushes(FH, FW, N, pushes, seed, zero_depth={(0, 2)} if late else ())
    step = 1 << halvings
    for k in range(pushes):
        # denser edges for stream 0, so that its references cross one gate workgroup of 256 points in every flavour: stripes
        # three working pixels wide over the lower third, a working pixel further on per push like its scene
        stripes = ((np.arange(FW) // step - k) % 6 < 3)
        out[k][0][0][2 * FH // 3:, stripes] = 215
        out[k][0][0][2 * FH // 3:, ~stripes] = 25
    for k in range(1, pushes):
        # the occluder: 0.44, 0.28, 0.12 m (0.45, 0.30, 0.15 m) -- each step nearer by more than the gate's tolerance
        y0, x0, h, w = FH // 4 + 2 * k, FW // 4 + 3 * k, FH // 3, FW // 3
        for i in (0, 1):
            bgr, depth = out[k][0][i], out[k][1][i]
            bgr[y0:y0 + h, x0:x0 + w] = (30 + 40 * k, 200 - 30 * k, 90)
            depth[y0:y0 + h, x0:x0 + w] = (0.6 - 0.15 * k) if flavour == 2 else (3000 - 800 * k)
    return out


def _cams(cfg):
    _, halvings, levels, (FH, FW) = cfg
    return [[ros._camera(i, FH >> (halvings + l), FW >> (halvings + l)) for i in range(N)] for l in range(levels)]


def _tracker(hip, cfg, dtype, gate="never"):
    """gate: "never" (set_depth_gate is not called), None (called with NULL) or the fields of ea_depth_gate_params"""
    flavour, halvings, levels, _ = cfg
    cams = _cams(cfg)
    tb = hip.TrackerBatch(cams if levels > 1 else cams[0], dtype=dtype, flavour=flavour, halvings=halvings, levels=levels)
    for l in range(levels):
        for i in range(N):
            _knobs(tb.level_problem(l, i), i)
    if gate is None:
        tb.set_depth_gate(None)
    elif gate != "never":
        tb.set_depth_gate(**gate)
    return tb


def _image(hip, P):
    try:
        return P.get_dt()
    except hip.EAError as e:
        assert e.code == hip.EA_ERR_STATE, e
        return None


def _numpy_gate(P, M, cam, depth, s, f32, prm, i):
    """(class bytes, stats, weights) of problem P's points under M by the restatement; stream i's depth weighting is _knobs'"""
    pts = P.get_points()
    cls = ds.classify(pts, M[:3], cam, depth, s, Z, prm["radius"], prm["abs_tol"], prm["rel_tol"])
    w = dg.weights(cls, pts[:, 2], prm["w_occluded"], prm["w_free"], prm["w_unknown"], (2.0, 1) if i % 3 == 0 else None, f32)
    return cls, dg.stats(cls), w


class _Manual:
    """the manual loop: per push a Batch over fresh problems per level and group, as the module docstring says; every count it
    takes from the device is held to the numpy restatement on the way, with `apply` the written weights too"""

    def __init__(self, hip, cfg, dtype, prm):
        self.hip, self.cfg, self.dtype, self.prm = hip, cfg, dtype, prm
        self.cams = _cams(cfg)
        self.prev = None
        self.q, self.t = np.tile(np.array([1.0, 0, 0, 0]), (N, 1)), np.zeros((N, 3))

    def _set_frames(self, B, l, ref, now):
        flavour, halvings = self.cfg[0], self.cfg[1]
        if flavour == 0:
            B.set_frames(ref[0], ref[1], now[0], z_scaling=Z)
        elif flavour == 1:
            B.set_frames_canny(ref[0], ref[1], now[0], z_scaling=Z)
        else:
            try:
                B.set_frames_ros(ref[0], ref[1], now[0], halvings=halvings + l)
            except self.hip.EAError as e:                      # a current frame without any edge: everything else is set
                assert e.code == self.hip.EA_ERR_STATE, e

    def push(self, bgr, depth):
        hip, prm = self.hip, self.prm
        flavour, halvings, levels, _ = self.cfg
        f32 = self.dtype == hip.EA_F32
        out = dict(aligned=[0] * N, sums=[[None] * N for _ in range(levels)], counts={}, n_ref=[0] * N)
        if self.prev is not None:
            P = [[hip.Problem(*self.cams[l][i], dtype=self.dtype) for i in range(N)] for l in range(levels)]
            for l in range(levels):
                for i in range(N):
                    _knobs(P[l][i], i)
                B = hip.Batch(P[l])
                self._set_frames(B, l, self.prev, (bgr, depth))
                B.close()
            usable = [[P[l][i].num_points > 0 and _image(hip, P[l][i]) is not None for i in range(N)] for l in range(levels)]
            out["n_ref"] = [P[0][i].num_points for i in range(N)]
            al = [i for i in range(N) if usable[0][i]]
            qc, tc, stopped = self.q.copy(), self.t.copy(), set()
            for l in range(levels - 1, -1, -1):
                members = [i for i in al if i not in stopped and usable[l][i]]
                apply = prm is not None and prm.get("apply", 1)
                groups = {}
                for i in members:                              # one kernel family when every stream is weighted
                    groups.setdefault(0 if apply else int(i % 3 == 0), []).append(i)
                for grp in groups.values():
                    B = hip.Batch([P[l][i] for i in grp])
                    if prm is not None:
                        s = halvings + l if flavour == 2 else 0
                        B.set_now_depth([depth[i] for i in grp], Z)
                        M = np.stack([hip.pose_to_matrix(qc[i], tc[i]) for i in grp])
                        _, stats = B.depth_gate(M, classes=False, **prm)
                        for k, i in enumerate(grp):
                            _, want, ww = _numpy_gate(P[l][i], M[k], self.cams[l][i], depth[i], s, f32, prm, i)
                            assert stats[k] == want, (l, i, stats[k], want)
                            if apply:
                                assert np.array_equal(_bits(P[l][i].get_weights()), _bits(ww)), (l, i)
                            out["counts"][(l, i)] = stats[k]
                    q, t, ss = B.solve(qc[grp], tc[grp])
                    for k, i in enumerate(grp):
                        out["sums"][l][i] = ss[k]
                        if ss[k]["termination"] == hip.FAILURE:
                            stopped.add(i)
                        else:
                            qc[i], tc[i] = q[k], t[k]
                    B.close()
            for i in al:
                out["aligned"][i] = 1
                if i not in stopped:
                    self.q[i], self.t[i] = qc[i], tc[i]
            for lv in P:
                for p in lv:
                    p.close()
        self.prev = (bgr, depth)
        out["q"], out["t"] = self.q.copy(), self.t.copy()
        return out


ZERO = {k: 0 for k in ("n",) + dg.NAMES}


def _same_summary(a, b, at):
    assert (a is None) == (b is None), at
    if a is not None:
        for key in ("termination", "why", "num_iterations"):
            assert a[key] == b[key], (at, key, a[key], b[key])
        assert np.array_equal(_bits(a["final_cost"]), _bits(b["final_cost"])), (at, a["final_cost"], b["final_cost"])


def _compare_with_manual(hip, tb, manual, bgr, depth, levels, at, frames=None):
    """one push of the tracker (frames: what it is handed, default the host frames) against one of the manual loop"""
    q, t, sums, aligned = tb.push_frames(*(frames or (bgr, depth)), z_scaling=Z)
    want = manual.push(bgr, depth)
    assert list(aligned) == want["aligned"], (at, list(aligned), want["aligned"])
    assert np.array_equal(q, want["q"]) and np.array_equal(t, want["t"]), (at, q, want["q"], t, want["t"])
    gated = 0
    for i in range(N):
        last = tb.last_summaries(i)
        for l in range(levels):
            _same_summary(last[l], want["sums"][l][i], (at, "stream", i, "level", l))
            got = tb.last_depth_gate(i, level=l)
            assert got == want["counts"].get((l, i), ZERO), (at, i, l, got, want["counts"].get((l, i)))
            gated += int((l, i) in want["counts"])
        finest = [want["sums"][l][i] for l in range(levels) if want["sums"][l][i] is not None]
        _same_summary(sums[i], finest[0] if finest else None, (at, "stream", i))
    assert tb.info("gated") == gated and tb.info("depth_gate") == 1, at
    return want


# ---- 2: apply = 0 changes nothing -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("name", ["laplacian", "canny", "ros_h1", "pyramid"])
def test_counting_alone_changes_nothing(hip, name, dtype_name):
    cfg = CONFIGS[name]
    levels, dtype = cfg[2], _dtype(hip, dtype_name)
    prm = dict(apply=0, **GATE)
    gated, plain, manual = _tracker(hip, cfg, dtype, prm), _tracker(hip, cfg, dtype), _Manual(hip, cfg, dtype, prm)
    try:
        assert gated.info("depth_gate") == 1 and plain.info("depth_gate") == 0
        saw = 0
        for k, (bgr, depth) in enumerate(_pushes(cfg, 11)):
            at = (name, dtype_name, "push", k + 1)
            b = plain.push_frames(bgr, depth, z_scaling=Z)
            want = _compare_with_manual(hip, gated, manual, bgr, depth, levels, at)
            assert np.array_equal(want["q"], b[0]) and np.array_equal(want["t"], b[1]) and want["aligned"] == list(b[3]), at
            for i in range(N):
                _same_summary(gated.last_summaries(i)[0], plain.last_summaries(i)[0], at)
                for l in range(levels):
                    G, Q = gated.level_problem(l, i), plain.level_problem(l, i)
                    assert np.array_equal(_bits(G.get_points()), _bits(Q.get_points())), (at, i, l)
                    gw, qw = G.get_weights(), Q.get_weights()
                    assert (gw is None) == (qw is None) and (gw is None or np.array_equal(_bits(gw), _bits(qw))), (at, i, l)
                    gi, qi = _image(hip, G), _image(hip, Q)
                    assert (gi is None) == (qi is None) and (gi is None or np.array_equal(gi, qi)), (at, i, l)
            assert plain.info("gated") == 0
            saw += len(want["counts"])
            assert want["aligned"] == ([0, 0, 0], [1, 1, 0], [1, 1, 1], [1, 1, 1])[k], at      # stream 2 starts a push late
            if k == 1:
                assert want["n_ref"][0] > 256, want["n_ref"]                                   # more than one gate workgroup
        assert saw >= 8, saw                                       # 2 + 3 + 3 gated (stream, level 0) pairs at least
    finally:
        ros._close(gated, plain)


# ---- 3, 5: apply = 1 equals the manual loop; the occluder -----------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("name", ["laplacian", "canny", "ros_h0", "ros_h1", "pyramid"])
def test_gated_pushes_equal_the_manual_loop(hip, name, dtype_name):
    cfg = CONFIGS[name]
    levels, dtype = cfg[2], _dtype(hip, dtype_name)
    tb, manual = _tracker(hip, cfg, dtype, GATE), _Manual(hip, cfg, dtype, GATE)
    try:
        for k, (bgr, depth) in enumerate(_pushes(cfg, 23)):
            at = (name, dtype_name, "push", k + 1)
            want = _compare_with_manual(hip, tb, manual, bgr, depth, levels, at)
            for i in range(N):
                for l in range(levels):
                    P = tb.level_problem(l, i)                     # the new reference: defined weights, dd or exactly 1
                    if P.num_points:
                        dd = dg.depth_factor(P.get_points()[:, 2], 2.0, 1 if i % 3 == 0 else 0)
                        if dtype_name == "f32":
                            dd = dd.astype(np.float32).astype(np.float64)
                        assert np.array_equal(_bits(P.get_weights()), _bits(dd)), (at, i, l)
            if k >= 1:
                for i in (0, 1):                                   # behind the painted rectangle
                    assert want["counts"][(0, i)]["n_occluded"] > 0, (at, i, want["counts"][(0, i)])
            if k >= 2:
                assert want["counts"][(0, 2)]["n"] > 0, at
    finally:
        tb.close()


# ---- 4, 5: the weights of a kept keyframe ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("name", ["canny", "ros_h1"])
def test_a_kept_keyframe_is_gated_from_its_own_z_every_push(hip, name, dtype_name):
    cfg = CONFIGS[name]
    flavour, halvings = cfg[0], cfg[1]
    dtype, f32 = _dtype(hip, dtype_name), dtype_name == "f32"
    cams = _cams(cfg)[0]
    tb = _tracker(hip, cfg, dtype)
    tb.set_keyframes(min_visible_fraction=0.0)                     # every rule off: a stream replaces only what it must
    tb.set_depth_gate(**GATE)
    start = [(np.array([1.0, 0, 0, 0]), np.zeros(3)) for _ in range(N)]
    kept = occluded = 0
    try:
        for k, (bgr, depth) in enumerate(_pushes(cfg, 31, late=False)):
            before = [tb.problem(i).get_points() for i in range(N)]
            q, t, sums, aligned = tb.push_frames(bgr, depth, z_scaling=Z)
            for i in range(N):
                at = (name, dtype_name, "push", k + 1, "stream", i)
                P, state = tb.problem(i), tb.keyframe_state(i)
                stats = tb.last_depth_gate(i)
                if aligned[i]:
                    assert np.array_equal(_bits(before[i]), _bits(P.get_points())) or state["replaced"], at
                if state["replaced"]:
                    if P.num_points:
                        dd = dg.depth_factor(P.get_points()[:, 2], 2.0, 1 if i % 3 == 0 else 0)
                        dd = dd.astype(np.float32).astype(np.float64) if f32 else dd
                        assert np.array_equal(_bits(P.get_weights()), _bits(dd)), at
                    start[i] = (np.array([1.0, 0, 0, 0]), np.zeros(3))
                    continue
                assert aligned[i] and stats["n"] == P.num_points > 0, at
                M = hip.pose_to_matrix(*start[i])
                cls, want, ww = _numpy_gate(P, M, cams[i], depth[i], halvings if flavour == 2 else 0, f32, GATE, i)
                assert stats == want, (at, stats, want)
                w = P.get_weights()
                assert np.array_equal(_bits(w), _bits(ww)), at
                assert (w[cls == dg.OCCLUDED] == 0.0).all(), at
                kept += 1
                if i in (0, 1):
                    assert want["n_occluded"] > 0, (at, want)
                    occluded += 1
                if sums[i]["termination"] != hip.FAILURE:
                    start[i] = (q[i].copy(), t[i].copy())
        assert kept >= 4 and occluded >= 2, (kept, occluded)
    finally:
        tb.close()


# ---- 6: device frames -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["canny", "ros_h0", "ros_h1", "pyramid"])
def test_device_frames_equal_host_frames(hip, name):
    import torch
    cfg = CONFIGS[name]
    flavour, levels = cfg[0], cfg[2]
    tb, manual = _tracker(hip, cfg, hip.EA_F64, GATE), _Manual(hip, cfg, hip.EA_F64, GATE)
    try:
        for k, (bgr, depth) in enumerate(_pushes(cfg, 23)):
            d_bgr = [torch.from_numpy(f).cuda() for f in bgr]
            d_depth = [torch.from_numpy(f if flavour == 2 else f.view(np.int16)).cuda() for f in depth]
            _compare_with_manual(hip, tb, manual, bgr, depth, levels, (name, "device", "push", k + 1), frames=(d_bgr, d_depth))
    finally:
        tb.close()


# ---- 7: state ---------------------------------------------------------------------------------------------------------------------

def _push_state(tb, levels):
    return [[tb.last_depth_gate(i, level=l) for i in range(N)] for l in range(levels)], tb.info("gated")


@pytest.mark.parametrize("name", ["canny", "pyramid"])
def test_state_rules_and_rejected_pushes(hip, name):
    cfg = CONFIGS[name]
    flavour, levels = cfg[0], cfg[2]
    tb, twin, never = _tracker(hip, cfg, hip.EA_F64, GATE), _tracker(hip, cfg, hip.EA_F64, GATE), _tracker(hip, cfg, hip.EA_F64)
    pushes = _pushes(cfg, 47)
    try:
        for call, code in ((lambda: tb.last_depth_gate(N), hip.EA_ERR_INVALID_ARG), (lambda: tb.last_depth_gate(0, level=levels), hip.EA_ERR_INVALID_ARG)):
            with pytest.raises(hip.EAError) as ei:
                call()
            assert ei.value.code == code
        for k in range(2):
            a, b = tb.push_frames(*pushes[k], z_scaling=Z), twin.push_frames(*pushes[k], z_scaling=Z)
        with pytest.raises(hip.EAError) as ei:                     # a stream holds a reference
            tb.set_depth_gate(None)
        assert ei.value.code == hip.EA_ERR_STATE
        with pytest.raises(hip.EAError) as ei:
            tb.set_depth_gate(**GATE)
        assert ei.value.code == hip.EA_ERR_STATE and tb.info("depth_gate") == 1
        was = _push_state(tb, levels)
        assert was[1] > 0 and was == _push_state(twin, levels)
        bgr, depth = pushes[2]
        bad = [((bgr[:1] + [None] + bgr[2:], depth), {})]
        if flavour == 2:
            bad.append((([f[:-1] for f in bgr], [f[:-1] for f in depth]), {}))             # not divisible by 2^(halvings + levels - 1)
        else:
            bad.append(((bgr, depth), dict(z_scaling=0.0)))
        for args, kw in bad:
            with pytest.raises(hip.EAError) as ei:
                tb.push_frames(*args, **kw)
            assert ei.value.code == hip.EA_ERR_INVALID_ARG, ei.value
            assert _push_state(tb, levels) == was
        a, b = tb.push_frames(bgr, depth, z_scaling=Z), twin.push_frames(bgr, depth, z_scaling=Z)
        assert all(np.array_equal(x, y) for x, y in zip((a[0], a[1], a[3]), (b[0], b[1], b[3])))
        assert _push_state(tb, levels) == _push_state(twin, levels) and tb.info("gated") > 0
        tb.reset(-1)
        never.reset(-1)
        tb.set_depth_gate(None)                                    # accepted now; from here on a tracker that never had one
        assert tb.info("depth_gate") == 0 and _push_state(tb, levels) == ([[ZERO] * N] * levels, 0)
        for k in range(4):
            a, b = tb.push_frames(*pushes[k], z_scaling=Z), never.push_frames(*pushes[k], z_scaling=Z)
            assert all(np.array_equal(x, y) for x, y in zip((a[0], a[1], a[3]), (b[0], b[1], b[3]))), k
            for i in range(N):
                for l in range(levels):
                    _same_summary(tb.last_summaries(i)[l], never.last_summaries(i)[l], (k, i, l))
                    G, Q = tb.level_problem(l, i), never.level_problem(l, i)
                    assert np.array_equal(_bits(G.get_points()), _bits(Q.get_points())), (k, i, l)
                    gw, qw = G.get_weights(), Q.get_weights()
                    assert (gw is None) == (qw is None) and (gw is None or np.array_equal(_bits(gw), _bits(qw))), (k, i, l)
            assert tb.info("gated") == 0
        tb.reset(-1)
        tb.set_depth_gate(**GATE)                                  # and back on
        assert tb.info("depth_gate") == 1
    finally:
        ros._close(tb, twin, never)


def test_a_factor_that_is_no_float_is_refused_by_an_fp32_tracker(hip):
    cfg = CONFIGS["canny"]
    t32, t64 = _tracker(hip, cfg, hip.EA_F32), _tracker(hip, cfg, hip.EA_F64)
    try:
        with pytest.raises(hip.EAError) as ei:
            t32.set_depth_gate(w_unknown=1e39)
        assert ei.value.code == hip.EA_ERR_INVALID_ARG and t32.info("depth_gate") == 0
        t64.set_depth_gate(w_unknown=1e39)
        assert t64.info("depth_gate") == 1
    finally:
        ros._close(t32, t64)


# ---- 8: the example ---------------------------------------------------------------------------------------------------------------

def test_the_c_demo_prints_the_poses_and_counts_of_the_python_class(hip):
    """examples/gated_tracker_demo (plain C99 on the C-ABI) pushes a short synthetic sequence of its own making; it also writes
    the frames it pushed, and TrackerBatch on those frames returns the poses and the six counts it printed"""
    import tempfile
    subprocess.check_call(["make", "-s", "-C", os.path.join(ros.ROOT, "examples"), "gated_tracker_demo"])
    with tempfile.TemporaryDirectory() as tmp:
        out = subprocess.check_output([os.path.join(ros.ROOT, "examples", "gated_tracker_demo"), tmp], text=True).splitlines()
        head = out[0].split()
        assert head[0] == "frames"
        n, pushes, H, W = (int(v) for v in head[1:5])
        cam = tuple(float(v) for v in head[5:9])
        bgr = np.fromfile(os.path.join(tmp, "bgr.u8"), np.uint8).reshape(pushes, n, H, W, 3)
        depth = np.fromfile(os.path.join(tmp, "depth.u16"), np.uint16).reshape(pushes, n, H, W)
    assert len(out) == 1 + pushes * n
    tb = hip.TrackerBatch([cam] * n, dtype=hip.EA_F64, flavour=1)
    tb.set_depth_gate()
    try:
        occluded = 0
        for k in range(pushes):
            q, t, sums, aligned = tb.push_frames(list(bgr[k]), list(depth[k]))
            for i in range(n):
                f = out[1 + k * n + i].split()
                assert [int(f[0]), int(f[1]), int(f[2])] == [k + 1, i, int(aligned[i])], (k, i)
                assert np.array_equal(np.array(f[3:10], dtype=np.float64), np.concatenate([q[i], t[i]])), (k, i)
                st = tb.last_depth_gate(i)
                assert [int(v) for v in f[10:17]] == [st[key] for key in ("n",) + dg.NAMES], (k, i)
                occluded += st["n_occluded"]
        assert occluded > 0
    finally:
        tb.close()
