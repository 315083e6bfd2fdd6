"""ea_batch_set_frames_ros_pyramid / set_frames_ros_pyramid: the batched ROS producers over L pyramid levels from frames handed
in once -- one halving chain per side and kind writes every level's frame into that level's workspace, then each level runs the
single-level sequence.  The reference is Batch.set_frames_ros(halvings + l) on a twin batch per level, compared with
np.array_equal through integer views (tests/test_gpu_batch_frames_ros.py: _assert_same) on num_points, get_points(),
get_weights() and get_dt(), and -- for what the float32 mirror and the cameras feed -- on one evaluation per level.

4 problems per level, each level with cameras of its own extent, one problem with depth weighting.  Cases of (full extent,
halvings, levels): ((74, 140), 0, 2) level 0 is the uploaded frame itself; ((296, 560), 1, 3) the node's halving in front of
three levels, tile edges of the chain in both directions; ((272, 1040), 1, 3) level 0 is wider than a 256-lane row block;
((24, 48), 0, 4) a chain of three steps down to 3 x 6, where the frames have no edge left: the EA_ERR_STATE case.  Frames of
one call differ in kind (noise, lines, dot) so that a frame or a level reading its neighbour's region cannot go unnoticed."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_batch_frames_ros as ros

pytestmark = pytest.mark.gpu
N = 4
CASES = (((74, 140), 0, 2), ((296, 560), 1, 3), ((272, 1040), 1, 3), ((24, 48), 0, 4))
WEIGHTING = [None, (2.0, 1), None, None]


def _id(c):
    return "%dx%d_h%d_l%d" % (c[0] + c[1:])


def _frames(full, halvings, seed):
    """full-size frames made for the level-0 extent (ros._frame: noise, lines, dot, noise)"""
    return ros._pairs(full[0] >> halvings, full[1] >> halvings, halvings, N, seed)


def _levels(hip, full, halvings, levels, dtype):
    """-> ([problems per level], [Batch per level])"""
    probs = [ros._problems(hip, N, full[0] >> (halvings + l), full[1] >> (halvings + l), dtype, WEIGHTING) for l in range(levels)]
    return probs, [hip.Batch(p) for p in probs]


def _single_level_calls(hip, batches, ref, dep, now, halvings):
    """Batch.set_frames_ros per level -> [frames without edges per level]"""
    bare = []
    for l, b in enumerate(batches):
        try:
            b.set_frames_ros(ref, dep, now, halvings=halvings + l)
        except hip.EAError as e:
            assert e.code == hip.EA_ERR_STATE, e
        bare.append(b.info("frames_without_edges"))
    return bare


def _pyramid_call(hip, batches, ref, dep, now, halvings, bare):
    if any(bare):
        with pytest.raises(hip.EAError) as ei:
            hip.set_frames_ros_pyramid(batches, ref, dep, now, halvings=halvings)
        assert ei.value.code == hip.EA_ERR_STATE, ei.value
        first = next(l for l, k in enumerate(bare) if k)
        assert "level %d" % first in str(ei.value) and "%d of" % sum(bare) in str(ei.value), ei.value
    else:
        hip.set_frames_ros_pyramid(batches, ref, dep, now, halvings=halvings)
    assert [b.info("frames_without_edges") for b in batches] == bare


def _assert_levels_same(got_p, want_p, where, points=True, image=True):
    for l, (gl, wl) in enumerate(zip(got_p, want_p)):
        for i in range(N):
            ros._assert_same(ros._state(gl[i], points, image), ros._state(wl[i], points, image), (where, "level", l, "problem", i))


def _assert_levels_eval_same(got_b, want_b, got_p, where):
    q, t = np.tile([1.0, 0, 0, 0], (N, 1)), np.tile([0.01, -0.02, 0.03], (N, 1))
    for l, (g, w) in enumerate(zip(got_b, want_b)):
        if all(p.num_points > 0 for p in got_p[l]):
            ros._assert_same_eval(g.eval(q, t), w.eval(q, t), (where, "level", l))


def _to_device(torch, frames):
    return [torch.from_numpy(np.ascontiguousarray(f)).to(torch.device("cuda", 0)) for f in frames]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dtype_name", ["EA_F64", "EA_F32"])
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_every_level_is_the_single_level_call(hip, case, dtype_name, where):
    full, halvings, levels = case
    dtype = getattr(hip, dtype_name)
    ref, dep, now = _frames(full, halvings, seed=full[0] + levels)
    want_p, want_b = _levels(hip, full, halvings, levels, dtype)
    got_p, got_b = _levels(hip, full, halvings, levels, dtype)
    try:
        bare = _single_level_calls(hip, want_b, ref, dep, now, halvings)
        if where == "device":
            torch = pytest.importorskip("torch")
            if not torch.cuda.is_available():
                pytest.skip("torch has no device")
            d_ref, d_dep, d_now = _to_device(torch, ref), _to_device(torch, dep), _to_device(torch, now)
            _pyramid_call(hip, got_b, d_ref, d_dep, d_now, halvings, bare)
            assert all(torch.equal(a.cpu(), torch.from_numpy(b)) for a, b in zip(d_ref + d_now, ref + now))   # read in place
            assert got_b[0].info("frames_uploaded") == 0
        else:
            _pyramid_call(hip, got_b, ref, dep, now, halvings, bare)
            assert got_b[0].info("frames_uploaded") == 3 * N      # whatever `levels` is
        print(_id(case), dtype_name, where, "frames without edges per level:", bare,
              "points of problem 0 per level:", [p[0].num_points for p in got_p])
        assert bare[0] == 0                                       # every kind has edges on level 0; averaged noise may lose them above
        if full == (24, 48):
            assert bare[-1] > 0                                   # the 3 x 6 level: frames without an edge, the others complete
        assert got_p[0][1].get_weights() is not None
        _assert_levels_same(got_p, want_p, (where, dtype_name))
        _assert_levels_eval_same(got_b, want_b, got_p, (where, dtype_name))
        for l in range(levels):
            assert got_b[l].info("frames_hysteresis_rounds") == want_b[l].info("frames_hysteresis_rounds"), l
    finally:
        ros._close(want_b, got_b, *want_p, *got_p)


@pytest.mark.parametrize("case", CASES[:2], ids=_id)
def test_one_side_at_a_time(hip, case):
    full, halvings, levels = case
    ref, dep, now = _frames(full, halvings, seed=5)
    want_p, want_b = _levels(hip, full, halvings, levels, hip.EA_F64)
    got_p, got_b = _levels(hip, full, halvings, levels, hip.EA_F64)
    try:
        assert not any(_single_level_calls(hip, want_b, ref, dep, None, halvings))
        hip.set_frames_ros_pyramid(got_b, ref, dep, None, halvings=halvings)
        assert got_b[0].info("frames_uploaded") == 2 * N
        _assert_levels_same(got_p, want_p, "reference side only")     # (the images: the ones the problems started with)
        assert not any(_single_level_calls(hip, want_b, None, None, now, halvings))
        hip.set_frames_ros_pyramid(got_b, now_bgr=now, halvings=halvings)
        assert got_b[0].info("frames_uploaded") == N
        _assert_levels_same(got_p, want_p, "current side only")
        # a single-level call on a level's batch afterwards finds the batch in working order
        got_b[levels - 1].set_frames_ros(ref, dep, now[::-1], halvings=halvings + levels - 1)
        want_b[levels - 1].set_frames_ros(ref, dep, now[::-1], halvings=halvings + levels - 1)
        _assert_levels_same(got_p, want_p, "a single-level call afterwards")
    finally:
        ros._close(want_b, got_b, *want_p, *got_p)


def test_levels_one_is_the_single_level_call(hip):
    full, halvings = (74, 140), 1
    ref, dep, now = _frames(full, halvings, seed=9)
    want_p, want_b = _levels(hip, full, halvings, 1, hip.EA_F64)
    got_p, got_b = _levels(hip, full, halvings, 1, hip.EA_F64)
    try:
        assert not any(_single_level_calls(hip, want_b, ref, dep, now, halvings))
        hip.set_frames_ros_pyramid(got_b, ref, dep, now, halvings=halvings)
        assert got_b[0].info("frames_uploaded") == 3 * N
        _assert_levels_same(got_p, want_p, "levels = 1")
    finally:
        ros._close(want_b, got_b, *want_p, *got_p)


def test_misuse_is_refused_and_leaves_every_problem_as_it_was(hip):
    full, halvings, levels = (72, 144), 1, 2                      # divisible by 8, not by 16
    ref, dep, now = _frames(full, halvings, seed=61)
    want_p, want_b = _levels(hip, full, halvings, levels, hip.EA_F64)
    got_p, got_b = _levels(hip, full, halvings, levels, hip.EA_F64)
    extra_p, extra_b = _levels(hip, full, halvings, 3, hip.EA_F64)   # further levels: 18 x 36, 9 x 18 (and a spare)
    f32_p = ros._problems(hip, N, 18, 36, hip.EA_F32)
    f32_b = hip.Batch(f32_p)
    short_b = hip.Batch(extra_p[2][:3])
    twice_b = hip.Batch(got_p[0][:1] + extra_p[2][1:])                 # holds a problem of level 0
    L = hip.load()
    nan = float("nan")
    _single_level_calls(hip, want_b, ref, dep, now, halvings)
    hip.set_frames_ros_pyramid(got_b, ref, dep, now, halvings=halvings)
    other = [f[::-1].copy() for f in now]   # frames that would change every image if a refused call ran

    def refused(call):
        with pytest.raises(hip.EAError) as ei:
            call()
        assert ei.value.code == hip.EA_ERR_INVALID_ARG, ei.value
        _assert_levels_same(got_p, want_p, "unchanged")

    try:
        kw = dict(halvings=halvings)
        P = hip.set_frames_ros_pyramid
        refused(lambda: P(got_b, ref, dep, other[:2] + [None] + other[3:], **kw))                  # a NULL entry
        refused(lambda: P(got_b, ref, dep[:2] + [None] + dep[3:], other, **kw))
        refused(lambda: P(got_b, ref[:-1], dep[:-1], other[:-1], **kw))                            # a wrong count
        refused(lambda: P([], ref, dep, other, **kw))                                              # nlevels < 1
        refused(lambda: P(got_b, ref, dep, other, halvings=-1))
        refused(lambda: P(got_b, ref, dep, other, halvings=8))                                     # halvings + levels - 1 > 8
        refused(lambda: P(got_b + extra_b[:2], ref, dep, other, **kw))                             # 72 x 144 is not divisible by 16
        refused(lambda: P(got_b, ref, dep, other, halvings=3))
        refused(lambda: P(got_b, now_bgr=[f[:8, :16].copy() for f in other], **kw))                # the coarsest level 2 x 4
        refused(lambda: P(got_b + [short_b], ref, dep, other, **kw))                               # batches of different counts
        refused(lambda: P(got_b + [f32_b], ref, dep, other, **kw))                                 # ... of different dtypes
        refused(lambda: P(got_b + [twice_b], ref, dep, other, **kw))                               # a problem on two levels
        refused(lambda: P([got_b[0], got_b[0]], ref, dep, other, **kw))
        refused(lambda: P(got_b, ref, dep, other, t1=nan, **kw))                                   # a NaN threshold
        prm = hip.RosFrameParams()
        L.ea_default_ros_frame_params(C.byref(prm), *other[0].shape[:2])
        prm.halvings = halvings
        hs = (C.c_void_p * levels)(*[b._h for b in got_b])
        ptrs = (C.c_void_p * N)(*[f.ctypes.data for f in other])
        dptrs = (C.c_void_p * N)(*[d.ctypes.data for d in dep])
        refused(lambda: hip._check(L.ea_batch_set_frames_ros_pyramid(None, levels, None, None, ptrs, C.byref(prm))))
        refused(lambda: hip._check(L.ea_batch_set_frames_ros_pyramid(hs, levels, None, None, ptrs, None)))
        refused(lambda: hip._check(L.ea_batch_set_frames_ros_pyramid(hs, levels, None, None, None, C.byref(prm))))
        refused(lambda: hip._check(L.ea_batch_set_frames_ros_pyramid(hs, levels, ptrs, None, None, C.byref(prm))))
        refused(lambda: hip._check(L.ea_batch_set_frames_ros_pyramid((C.c_void_p * levels)(got_b[0]._h, None), levels, None, None, ptrs, C.byref(prm))))
        # host pointers handed to the device entry
        refused(lambda: hip._check(L.ea_batch_set_frames_ros_pyramid_device(hs, levels, None, None, ptrs, C.byref(prm))))
        refused(lambda: hip._check(L.ea_batch_set_frames_ros_pyramid_device(hs, levels, ptrs, dptrs, None, C.byref(prm))))
        # an accepted call afterwards does what it should
        P(got_b, now_bgr=other, **kw)
        assert not np.array_equal(got_p[1][0].get_dt(), want_p[1][0].get_dt())
        P(got_b, now_bgr=now, **kw)
        _assert_levels_same(got_p, want_p, "again")
    finally:
        ros._close(short_b, twice_b, f32_b, want_b, got_b, extra_b, f32_p, *want_p, *got_p, *extra_p)
