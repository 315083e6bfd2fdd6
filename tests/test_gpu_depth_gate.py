"""ea_*_set_now_depth and ea_*_depth_gate on the device against tests/depth_gate_ref.py, the numpy restatement of the header's
arithmetic.  Exactness is the requirement -- there are no tolerances: both sides run the same IEEE operations in the same
order on the same matrix, the same stored points (an fp32 problem: the floats it holds, read back with get_points) and the
same depth samples, so the class bytes, the counts and the bits of the written weights are equal.

Shapes: n in {1, 63, 64, 65, 255, 256, 257, 513} on the 5 x 7 image of tests/test_gpu_reproject.py (every window of radius 2
or 3 clips at a border) and one 48 x 64 case; radius 0..3; both depth kinds; both dtypes; plain, distortion, rig, both; the
three matrices of that test (the degenerate one gives bz == 0, NaN and points behind).  The inputs (tests/depth_gate_cases.py)
are dyadic: with rel_tol = 0 and abs_tol = 0.25 points sit exactly on the class boundary, one ulp beyond it on either side,
and between two equidistant samples of opposite sign."""
import os
import subprocess

import numpy as np
import pytest

import depth_gate_cases as dc
import depth_gate_ref as dg

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FACTORS = dict(w_occluded=0.125, w_free=0.3, w_unknown=0.7)
STAT_KEYS = ("n",) + dg.NAMES


def _dtype(hip, name):
    return hip.EA_F64 if name == "f64" else hip.EA_F32


def _problem(hip, im, variant, xyz, dtype, depth=None, order=None):
    dist, second = dc.VARIANTS[variant]
    P = hip.Problem(*im["K"], dtype=dtype)
    if order is not None:
        P.set_point_order(order)
    if xyz is not None and len(xyz):
        P.set_points(xyz)
    dt = np.random.default_rng(0).uniform(0.0, 1.0, (im["H"], im["W"])).astype(np.float32)
    P.set_dt_grid(np.ascontiguousarray(dt.astype(np.float64).T))
    if dist:
        P.set_distortion(*dc.DIST)
    if second:
        P.set_second_camera(dc.T12, dc.T12INV)
    if depth is not None:
        P.set_now_depth(depth, dc.Z_SCALING)
    return P


def _want(P, im, variant, T, depth, radius, tol=dc.TOL, details=False):
    return dg.classify(P.get_points(), dc.matrix_for(variant, T), im["K"], depth, dc.Z_SCALING, radius,
                       dist=dc.DIST if dc.VARIANTS[variant][0] else None, details=details, **tol)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_the_cases_are_those_of_the_reprojection_test():
    import test_gpu_reproject as tgr
    assert dc.SIZES == tgr.SIZES and dc.SMALL == tgr.SMALL and dc.BIG == tgr.BIG and dc.DIST == tgr.DIST
    assert dc.VARIANTS == tgr.VARIANTS and list(dc.MATRICES) == list(tgr.MATRICES)
    assert all(np.array_equal(dc.MATRICES[k], tgr.MATRICES[k]) for k in dc.MATRICES)
    assert np.array_equal(dc.T12, tgr.T12) and np.array_equal(dc.T12INV, tgr.T12INV)


# ---- class bytes, counts and weight bits ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_classes_counts_and_weights(hip, kind, dtype_name):
    f32 = dtype_name == "f32"
    cases = [(dc.SMALL, n) for n in dc.SIZES] + [(dc.BIG, 513)]
    # the restatement first: no class, boundary or tie of this ladder is vacuous
    problems, wants = [], {}
    seen = np.zeros(6, np.int64)
    tie = boundary = ulp_occluded = ulp_free = 0
    for im, n in cases:
        depth = dc.depth_image(im, kind)
        xyz = dc.points(n, 100 + n, im, f32)
        for variant in dc.VARIANTS:
            P = _problem(hip, im, variant, xyz, _dtype(hip, dtype_name), depth)
            problems.append((P, im, n, variant, depth))
            for name, T in dc.MATRICES.items():
                for radius in range(4):
                    want, det = _want(P, im, variant, T, depth, radius, details=True)
                    wants[(id(P), name, radius)] = want
                    seen += np.bincount(want, minlength=6)
                    if name == "identity" and variant == "plain":
                        tie += int(det["tie"].sum())
                        on = det["have"]
                        boundary += int((on & (np.abs(det["diff"]) == det["tol"]) & (want == dg.CONSISTENT)).sum())
                        beyond = on & (np.abs(det["diff"]) > det["tol"]) & (np.abs(det["diff"]) - det["tol"] < 2.0 ** -20)
                        ulp_occluded += int((beyond & (want == dg.OCCLUDED)).sum())
                        ulp_free += int((beyond & (want == dg.FREE)).sum())
    assert (seen > 0).all(), seen
    assert tie > 0 and boundary > 0 and ulp_occluded > 0 and ulp_free > 0
    # the device
    for P, im, n, variant, depth in problems:
        z = P.get_points()[:, 2]
        assert P.get_weights() is None
        for name, T in dc.MATRICES.items():
            for radius in range(4):
                want = wants[(id(P), name, radius)]
                where = (kind, dtype_name, n, variant, name, radius)
                P.set_depth_weighting(1.0, 0)
                cls, stats = P.depth_gate(T, radius=radius, **dc.TOL, **FACTORS)
                assert np.array_equal(cls, want), where + (np.flatnonzero(cls != want)[:8],)
                assert stats == dg.stats(want) and sum(stats[k] for k in dg.NAMES) == stats["n"] == n, where
                assert np.array_equal(_bits(P.get_weights()), _bits(dg.weights(want, z, f32=f32, **FACTORS))), where
                if radius == 1:      # with the depth-weighting factor, power 1 and 3; no class buffer asked for
                    for dw in ((1.0, 1), (1.25, 3)):
                        P.set_depth_weighting(*dw)
                        none, stats = P.depth_gate(T, classes=False, radius=radius, **dc.TOL, **FACTORS)
                        assert none is None and stats == dg.stats(want), where
                        ww = dg.weights(want, z, depth_weighting=dw, f32=f32, **FACTORS)
                        assert np.array_equal(_bits(P.get_weights()), _bits(ww)), where + (dw,)
        assert np.array_equal(P.depth_gate((np.array([1.0, 0, 0, 0]), np.zeros(3)), classes=True, apply=0)[0],
                              P.depth_gate(np.eye(4), apply=0)[0])                      # the (q, t) form
        P.set_weights(None)
        assert P.get_weights() is None                                                  # undone
        P.close()


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_the_tie_keeps_the_first_and_the_boundary_is_consistent(hip, kind):
    """the planted points by name, fp64: z = 1.5 between 1.25 and 1.75 (abs_tol = 0.125: the class names the kept sample);
    |d - bz| == tol is CONSISTENT, one ulp more is not"""
    xyz, what = dc.planted(False)
    depth = dc.depth_image(dc.SMALL, kind)
    P = _problem(hip, dc.SMALL, "plain", xyz, hip.EA_F64, depth)
    tight = dict(abs_tol=0.125, rel_tol=0.0)
    want, det = _want(P, dc.SMALL, "plain", np.eye(4), depth, 1, tol=tight, details=True)
    below, above = what.index("tie_first_below"), what.index("tie_first_above")
    assert det["tie"][below] and det["tie"][above] and want[below] == dg.OCCLUDED and want[above] == dg.FREE
    cls, _ = P.depth_gate(np.eye(4), radius=1, apply=0, **tight)
    assert np.array_equal(cls, want)
    for radius in range(4):
        want, det = _want(P, dc.SMALL, "plain", np.eye(4), depth, radius, details=True)
        cls, _ = P.depth_gate(np.eye(4), radius=radius, apply=0, **dc.TOL)
        assert np.array_equal(cls, want)
        for name, c in (("boundary_below", dg.CONSISTENT), ("boundary_above", dg.CONSISTENT), ("ulp_occluded", dg.OCCLUDED),
                        ("ulp_free", dg.FREE)):
            i = what.index(name)
            assert cls[i] == c, (name, radius)
            assert (abs(det["diff"][i]) == 0.25) == (c == dg.CONSISTENT) and abs(abs(det["diff"][i]) - 0.25) < 2.0 ** -50
    P.close()


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_apply_zero_changes_nothing(hip, dtype_name):
    """weights, the weighted state and a resident-pose evaluation are what they were, weighted or not"""
    im = dc.SMALL
    depth = dc.depth_image(im, "u16")
    P = _problem(hip, im, "plain", dc.points(257, 3, im), _dtype(hip, dtype_name), depth)
    B = hip.Batch([P])
    q = np.tile(np.array([1.0, 0, 0, 0]), (2, 1, 1))
    t = np.zeros((2, 1, 3))
    t[1, 0, 0] = 0.05
    for given in (None, np.random.default_rng(5).uniform(0.1, 1.0, 257)):
        P.set_weights(given)
        kept = P.get_weights()
        B.set_poses(q, t)
        before = B.eval_resident_poses()
        cls, stats = P.depth_gate(np.eye(4), apply=0, **dc.TOL)
        _, bstats = B.depth_gate(np.eye(4)[None], apply=0, **dc.TOL)
        assert stats == bstats[0] == dg.stats(_want(P, im, "plain", np.eye(4), depth, 1))
        after = B.eval_resident_poses()            # (raises if the resident poses were dropped)
        for key in ("cost", "JtJ", "Jtr"):
            assert np.array_equal(_bits(before[key]), _bits(after[key])), key
        now = P.get_weights()
        assert (now is None) == (given is None) and (given is None or np.array_equal(_bits(now), _bits(kept)))
        assert B.info("weighted") == (0 if given is None else 1)
    B.close()
    P.close()


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_callers_order_under_a_tiled_point_order(hip, kind, dtype_name):
    """48 x 64, set_point_order(16): the single-problem class bytes and the weights read back are in the caller's order, the
    batch form's rows in storage order"""
    im = dc.BIG
    f32 = dtype_name == "f32"
    depth = dc.depth_image(im, kind)
    P = _problem(hip, im, "plain", dc.points(513, 7, im), _dtype(hip, dtype_name), depth, order=16)
    assert P.point_order == 16
    T = dc.MATRICES["rigid"]
    for radius in range(4):
        want = _want(P, im, "plain", T, depth, radius)               # get_points: the caller's order
        cls, stats = P.depth_gate(T, radius=radius, **dc.TOL, **FACTORS)
        assert np.array_equal(cls, want) and stats == dg.stats(want), radius
        assert np.array_equal(_bits(P.get_weights()), _bits(dg.weights(want, P.get_points()[:, 2], f32=f32, **FACTORS)))
    B = hip.Batch([P])
    stored, bstats = B.depth_gate(T[None], radius=3, apply=0, **dc.TOL)
    assert bstats[0] == stats and not np.array_equal(stored, cls) and np.array_equal(np.bincount(stored, minlength=6), np.bincount(cls, minlength=6))
    uv_caller, uv_stored = P.reproject(T), B.reproject(T[None])      # the same permutation as the reprojection's rows
    keys = {row.tobytes(): i for i, row in enumerate(uv_caller)}
    perm = np.array([keys[row.tobytes()] for row in uv_stored])
    assert np.array_equal(stored, cls[perm])
    B.close()
    P.close()


# ---- batch forms --------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def five(hip, request):
    """five problems of sizes {0, 1, 64, 257, 513}: the 257 one is plain and carries a rig TERM of 63 points, then a distorted
    one, a second-camera one, a plain one"""
    dtype_name, kind = getattr(request, "param", ("f64", "u16"))
    dtype = _dtype(hip, dtype_name)
    im = dc.SMALL
    depth = dc.depth_image(im, kind)
    term = _problem(hip, im, "rig", dc.points(63, 21, im), dtype, depth)
    kinds = ["plain", "distortion", "rig", "plain", "plain"]
    Ps = [_problem(hip, im, "plain", None, dtype, depth),
          _problem(hip, im, "distortion", dc.points(1, 22, im), dtype, depth),
          _problem(hip, im, "rig", dc.points(64, 23, im), dtype, depth),
          _problem(hip, im, "plain", dc.points(257, 24, im), dtype, depth),
          _problem(hip, im, "plain", dc.points(513, 25, im), dtype, depth)]
    Ps[3].add_term(term)
    Ts = np.stack([dc.MATRICES[k] for k in ("identity", "rigid", "degenerate", "rigid", "degenerate")])
    B = hip.Batch(Ps)
    yield dict(Ps=Ps, term=term, kinds=kinds, Ts=Ts, B=B, im=im, depth=depth, f32=dtype_name == "f32")
    B.close()
    Ps[3].clear_terms()
    for P in Ps + [term]:
        P.close()


@pytest.mark.parametrize("five", [("f64", "u16"), ("f32", "f32"), ("f64", "f32"), ("f32", "u16")], indirect=True)
def test_batch_forms_agree_with_the_single_problem_calls(hip, five):
    import torch
    Ps, B, Ts, kinds, im, depth, f32 = (five[k] for k in ("Ps", "B", "Ts", "kinds", "im", "depth", "f32"))
    off = B.row_offsets()
    assert list(off) == [0, 0, 1, 65, 65 + 257 + 63, 385 + 513]
    rows = int(off[-1])
    prm = dict(radius=2, **dc.TOL, **FACTORS)
    single = [P.depth_gate(T, apply=0, **prm) if P.num_points else (np.zeros(0, np.uint8), dg.stats(np.zeros(0, np.uint8)))
              for P, T in zip(Ps, Ts)]
    for i, P in enumerate(Ps):
        if P.num_points:
            assert np.array_equal(single[i][0], _want(P, im, kinds[i], Ts[i], depth, 2)), i
    sentinel = 99
    q = np.tile(np.array([1.0, 0, 0, 0]), (2, 5, 1))
    t = np.zeros((2, 5, 3))
    t[1, :, 1] = 0.03
    assert B.info("weighted") == 0
    host, stats = B.depth_gate(Ts, out=np.full(rows, sentinel, np.uint8), **prm)          # apply: the weights appear
    B.row_offsets()
    assert B.info("weighted") == 4                                                         # every head family with points
    dev = torch.full((rows,), sentinel, dtype=torch.uint8, device="cuda")
    B.set_poses(q, t)
    before = B.eval_resident_poses()
    dev_stats = B.depth_gate_device(Ts, dev, **prm)                                        # only the values change (same ones)
    after = B.eval_resident_poses()                                                        # (raises if the poses were dropped)
    for key in ("cost", "JtJ", "Jtr"):
        assert np.array_equal(_bits(before[key]), _bits(after[key])), key
    assert np.array_equal(dev.cpu().numpy(), host) and dev_stats == stats
    assert B.depth_gate_device(Ts, None, **prm) == stats                                   # no class buffer at all
    for i, P in enumerate(Ps):
        n = P.num_points
        assert np.array_equal(host[off[i]:off[i] + n], single[i][0]) and stats[i] == single[i][1], i
        if n:
            assert np.array_equal(_bits(P.get_weights()), _bits(dg.weights(single[i][0], P.get_points()[:, 2], f32=f32, **FACTORS))), i
    assert stats[0] == {k: 0 for k in STAT_KEYS} and Ps[0].get_weights() is None
    assert (host[off[3] + 257:off[4]] == sentinel).all() and stats[3]["n"] == 257          # the term's rows are left alone
    assert five["term"].get_weights() is None
    # other values: still no rebuild, the poses stay resident and see the new weights
    B.depth_gate_device(Ts, None, radius=2, w_occluded=0.5, w_free=0.5, w_unknown=0.25, **dc.TOL)
    moved = B.eval_resident_poses()
    assert not np.array_equal(_bits(moved["cost"]), _bits(before["cost"]))
    # capacity and argument errors with a real batch
    for call in (lambda: B.depth_gate(Ts, out=np.zeros(rows - 1, np.uint8), **prm),
                 lambda: B.depth_gate_device(Ts, dev, capacity_rows=rows - 1, **prm)):
        with pytest.raises(hip.EAError) as ei:
            call()
        assert ei.value.code == hip.EA_ERR_INVALID_ARG
    bad = Ts.copy()
    bad[4, 3, 3] = 2.0
    with pytest.raises(hip.EAError) as ei:
        B.depth_gate(bad, **prm)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    if f32:     # a factor that is a double but no float
        with pytest.raises(hip.EAError) as ei:
            B.depth_gate(Ts, w_unknown=1e39)
        assert ei.value.code == hip.EA_ERR_INVALID_ARG
    else:
        B.depth_gate(Ts, w_unknown=1e39, apply=0)


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_head_rows_come_down_around_a_term_in_the_middle(hip, dtype_name):
    """three problems of 1, 257 and 64 head points, the middle one with a TERM of 5 points: the head rows are not adjacent,
    and one segment ends a single point past a 256-lane workgroup.  Batch.reproject and the host form of Batch.depth_gate with
    classes give every problem the bits of its single-problem call and leave the term's rows as the caller wrote them"""
    import test_gpu_reproject as tgr
    dtype, im = _dtype(hip, dtype_name), dc.SMALL
    depth = dc.depth_image(im, "u16")
    term = _problem(hip, im, "rig", dc.points(5, 31, im), dtype, depth)
    Ps = [_problem(hip, im, "distortion", dc.points(1, 32, im), dtype, depth),
          _problem(hip, im, "plain", dc.points(257, 33, im), dtype, depth),
          _problem(hip, im, "rig", dc.points(64, 34, im), dtype, depth)]
    Ps[1].add_term(term)
    Ts = np.stack([dc.MATRICES[k] for k in ("rigid", "degenerate", "rigid")])
    B = hip.Batch(Ps)
    off = B.row_offsets()
    assert list(off) == [0, 1, 1 + 257 + 5, 263 + 64]
    prm = dict(radius=1, apply=0, **dc.TOL, **FACTORS)
    uv = B.reproject(Ts, out=np.full((327, 2), 7.25))
    cls, stats = B.depth_gate(Ts, out=np.full(327, 99, np.uint8), **prm)
    for i, P in enumerate(Ps):
        n = P.num_points
        tgr._assert_same_bits(uv[off[i]:off[i] + n], P.reproject(Ts[i]), ("reproject", dtype_name, i))
        single = P.depth_gate(Ts[i], **prm)
        assert np.array_equal(cls[off[i]:off[i] + n], single[0]) and stats[i] == single[1], i
    assert (uv[258:263] == 7.25).all() and (cls[258:263] == 99).all()                      # the term's rows are left alone
    B.close()
    Ps[1].clear_terms()
    for P in Ps + [term]:
        P.close()


def test_batch_set_now_depth_host_and_device(hip):
    """N images in one call, from host arrays and from tensors on the device, of either kind; the image survives new points, a
    new DT image and dropped weights; NULL drops it"""
    import torch
    im = dc.SMALL
    Ps = [_problem(hip, im, "plain", dc.points(n, 40 + n, im), hip.EA_F64) for n in (65, 257)]
    B = hip.Batch(Ps)
    with pytest.raises(hip.EAError) as ei:
        B.depth_gate([np.eye(4)] * 2, apply=0)
    assert ei.value.code == hip.EA_ERR_STATE                                   # no depth yet
    for kind in ("u16", "f32"):
        d0 = dc.depth_image(im, kind)
        d1 = np.ascontiguousarray(d0[::-1])
        want = [dg.stats(_want(P, im, "plain", np.eye(4), d, 1)) for P, d in zip(Ps, (d0, d1))]
        B.set_now_depth([d0, d1], dc.Z_SCALING)
        assert B.depth_gate([np.eye(4)] * 2, apply=0, **dc.TOL)[1] == want
        B.set_now_depth(None)
        tensors = [torch.from_numpy(d.view(np.int16) if kind == "u16" else d).cuda() for d in (d1, d0)]
        B.set_now_depth(tensors, dc.Z_SCALING)
        assert B.depth_gate([np.eye(4)] * 2, apply=0, **dc.TOL)[1] == [dg.stats(_want(P, im, "plain", np.eye(4), d, 1)) for P, d in zip(Ps, (d1, d0))]
        tensors[0].zero_()                                                     # copied, not borrowed
        Ps[0].set_now_depth(torch.from_numpy(d0.view(np.int16) if kind == "u16" else d0).cuda(), dc.Z_SCALING)
        Ps[1].set_now_depth(d1, dc.Z_SCALING)
        Ps[0].set_points(Ps[0].get_points())
        Ps[1].set_dt_grid(np.zeros((im["W"], im["H"])))
        assert B.depth_gate([np.eye(4)] * 2, apply=0, **dc.TOL)[1] == want
    host = dc.depth_image(im, "u16")
    with pytest.raises(hip.EAError) as ei:                                     # host memory handed to the device form
        hip._check(hip.load().ea_batch_set_now_depth_device(B._h, (hip.C.c_void_p * 2)(host.ctypes.data, host.ctypes.data), 0, 5, 7, 1024.0))
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    with pytest.raises(hip.EAError) as ei:
        hip._check(hip.load().ea_problem_set_now_depth_device(Ps[0]._h, hip.C.c_void_p(host.ctypes.data), 0, 5, 7, 1024.0))
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    assert B.depth_gate([np.eye(4)] * 2, apply=0, **dc.TOL)[1] == want         # a refused call leaves the held images alone
    twice = hip.Batch([Ps[0], Ps[0]])
    with pytest.raises(hip.EAError) as ei:
        twice.set_now_depth([host, host], dc.Z_SCALING)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    twice.close()
    Ps[1].set_now_depth(None)
    with pytest.raises(hip.EAError) as ei:
        B.depth_gate([np.eye(4)] * 2, **dc.TOL)
    assert ei.value.code == hip.EA_ERR_STATE and Ps[0].get_weights() is None   # the whole call fails before any launch
    B.close()
    for P in Ps:
        P.close()


# ---- downstream: the gate's weights are weights like any other --------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_downstream_equivalence_with_set_weights(hip, dtype_name):
    """batch A after ea_batch_depth_gate(apply) against batch B of identical problems whose weights come from the restatement
    through ea_problem_set_weights: the same bits from ea_batch_eval, the same poses and iteration counts from ea_batch_solve"""
    im = dc.BIG
    f32 = dtype_name == "f32"
    depth = dc.depth_image(im, "u16")
    sizes, variants = (513, 257, 64), ("plain", "distortion", "rig")
    A = [_problem(hip, im, v, dc.points(n, 60 + n, im), _dtype(hip, dtype_name), depth) for n, v in zip(sizes, variants)]
    Bp = [_problem(hip, im, v, dc.points(n, 60 + n, im), _dtype(hip, dtype_name)) for n, v in zip(sizes, variants)]
    for P in A + Bp:
        P.set_depth_weighting(1.25, 2)
    Ts = np.stack([dc.MATRICES["rigid"]] * 3)
    BA, BB = hip.Batch(A), hip.Batch(Bp)
    BA.depth_gate_device(Ts, None, radius=1, **dc.TOL, **FACTORS)
    for P, Q, v in zip(A, Bp, variants):
        want = _want(Q, im, v, Ts[0], depth, 1)
        assert len(set(want)) >= 4
        Q.set_weights(dg.weights(want, Q.get_points()[:, 2], depth_weighting=(1.25, 2), f32=f32, **FACTORS))
        assert np.array_equal(_bits(P.get_weights()), _bits(Q.get_weights()))
    q0 = np.array([0.9995, 0.01, -0.02, 0.015])
    q = np.tile(q0 / np.linalg.norm(q0), (3, 1))
    t = np.tile(np.array([0.02, -0.01, 0.03]), (3, 1))
    ea, eb = BA.eval(q, t), BB.eval(q, t)
    for key in ("cost", "JtJ", "Jtr"):
        assert np.array_equal(_bits(ea[key]), _bits(eb[key])), key
    assert np.array_equal(ea["n_invalid"], eb["n_invalid"]) and np.isfinite(ea["cost"]).all() and (ea["cost"] > 0).all()
    qa, ta, sa = BA.solve(q, t, max_num_iterations=8)
    qb, tb, sb = BB.solve(q, t, max_num_iterations=8)
    assert np.array_equal(_bits(qa), _bits(qb)) and np.array_equal(_bits(ta), _bits(tb))
    assert [s["num_iterations"] for s in sa] == [s["num_iterations"] for s in sb]
    assert [s["termination"] for s in sa] == [s["termination"] for s in sb]
    BA.close(); BB.close()
    for P in A + Bp:
        P.close()


# ---- state errors -------------------------------------------------------------------------------------------------------------

def test_state_errors(hip):
    import torch
    im = dc.SMALL
    depth = dc.depth_image(im, "u16")
    P = hip.Problem(*im["K"], dtype=hip.EA_F64)
    P.set_points(dc.points(65, 1, im))
    P.set_now_depth(depth, dc.Z_SCALING)
    with pytest.raises(hip.EAError) as ei:                  # no DT image
        P.depth_gate(np.eye(4))
    assert ei.value.code == hip.EA_ERR_STATE
    P.set_dt_grid(np.zeros((im["W"], im["H"])))
    P.set_now_depth(None)
    with pytest.raises(hip.EAError) as ei:                  # no depth
        P.depth_gate(np.eye(4))
    assert ei.value.code == hip.EA_ERR_STATE
    P.set_now_depth(np.zeros((im["H"] + 1, im["W"]), np.uint16), dc.Z_SCALING)      # accepted by the setter,
    with pytest.raises(hip.EAError) as ei:                  # an extent mismatch is found at gate time
        P.depth_gate(np.eye(4))
    assert ei.value.code == hip.EA_ERR_STATE and P.get_weights() is None
    P.set_now_depth(depth, dc.Z_SCALING)
    Q = _problem(hip, im, "plain", None, hip.EA_F64, depth)
    with pytest.raises(hip.EAError) as ei:                  # no points
        Q.depth_gate(np.eye(4))
    assert ei.value.code == hip.EA_ERR_STATE
    R = _problem(hip, im, "plain", dc.points(64, 2, im), hip.EA_F64, dc.depth_image(im, "f32"))
    B = hip.Batch([P, R])
    with pytest.raises(hip.EAError) as ei:                  # one kernel, one kind
        B.depth_gate([np.eye(4)] * 2)
    assert ei.value.code == hip.EA_ERR_STATE and P.get_weights() is None and R.get_weights() is None
    R.set_now_depth(depth, dc.Z_SCALING)
    host_cls = np.zeros(129, np.uint8)
    with pytest.raises(hip.EAError) as ei:                  # cls_dev that is host memory
        B.depth_gate_device([np.eye(4)] * 2, host_cls.ctypes.data, capacity_rows=129)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG and not host_cls.any() and P.get_weights() is None
    import ctypes as C
    cls = np.zeros(64, np.uint8)
    st = hip.DepthGateStats()
    prm = hip.default_depth_gate_params()
    rc = hip.load().ea_problem_depth_gate(P.handle, np.eye(4).ctypes.data_as(C.POINTER(C.c_double)), C.byref(prm),
                                          cls.ctypes.data_as(C.c_void_p), 64, C.byref(st))      # capacity 64 < 65
    assert rc == hip.EA_ERR_INVALID_ARG and not cls.any() and P.get_weights() is None
    twice = hip.Batch([P, P])
    with pytest.raises(hip.EAError) as ei:                  # with apply a problem's weights can be written once per call
        twice.depth_gate([np.eye(4)] * 2, **dc.TOL)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG and P.get_weights() is None
    both = twice.depth_gate([np.eye(4), dc.MATRICES["rigid"]], apply=0, **dc.TOL)[1]
    assert both[0] == P.depth_gate(np.eye(4), apply=0, **dc.TOL)[1] and both[1] == P.depth_gate(dc.MATRICES["rigid"], apply=0, **dc.TOL)[1]
    twice.close()
    dev = torch.zeros(129, dtype=torch.uint8, device="cuda")
    stats = B.depth_gate_device([np.eye(4)] * 2, dev, **dc.TOL)
    assert [s["n"] for s in stats] == [65, 64] and P.get_weights() is not None
    B.close()
    for X in (P, Q, R):
        X.close()


# ---- the example ----------------------------------------------------------------------------------------------------------------

def test_depth_gate_demo(hip, tmp_path):
    """examples/depth_gate_demo (plain C99 on the C-ABI) on the bundled pair: reference = frame 1, current = frame 2 with its
    depth; gate at the identity, solve, gate at the solved pose"""
    from oracle import preprocess_np as pp
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "depth_gate_demo"])
    G = os.path.join(ROOT, "tests", "golden", "rgbd")
    paths = []
    for k in (1, 2):
        bgr, depth = pp.load_rgb_as_bgr(os.path.join(G, "rgb_%d.png" % k)), pp.load_depth_u16(os.path.join(G, "depth_%d.png" % k))
        assert bgr.dtype == np.uint8 and depth.dtype == np.uint16 and bgr.shape[:2] == depth.shape
        for name, a in (("bgr_%d.u8" % k, bgr), ("depth_%d.u16" % k, depth)):
            paths.append(str(tmp_path / name))
            np.ascontiguousarray(a).tofile(paths[-1])
    H, W = depth.shape
    out = subprocess.run([os.path.join(ROOT, "examples", "depth_gate_demo"), str(H), str(W), "525.0", "525.0", "319.5", "239.5"] + paths,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [ln[0] for ln in lines] == ["identity", "solved", "pose"]
    for ln in lines[:2]:
        n, classes = int(ln[1]), [int(v) for v in ln[2:8]]
        assert n > 0 and sum(classes) == n
    assert int(lines[1][2 + dg.CONSISTENT]) > 0              # a sanity condition on real data, not a tuned number
