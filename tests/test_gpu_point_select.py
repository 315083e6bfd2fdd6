"""ea_*_select_points on the device against tests/point_select_ref.py, the numpy restatement of the header's rule.  Exactness is
the requirement -- there are no tolerances: the survivors are copies of stored values, the pixel of a point is the same IEEE
operations in the same order on both sides, and the winners of a cell are minima of integers, so points, weights and stats are
equal bit for bit, and an evaluation of the thinned problem equals the evaluation of a fresh problem that was handed the
restatement's survivors.

Shapes (tests/point_select_cases.py): a camera on a 37 x 29 grid, n in {0, 1, 63, 64, 65, 1023, 1024, 1025, 2049} (wavefront
and workgroup edges of the 256-lane passes), every combination of dtype, cell_px in {0, 1, 4, 64}, rule, `outside`, stride in
{1, 2, 30} and target in {0, 5, n, n + 1}, with and without weights; one case of 1024 * 1024 + 5 points (4097 block counts: the
scan carries across its chunks of 1024); the bundled frame (44 457 points, stride 30 -> the reference's 1 482 blocks); and the
multi-stream tracker on 64 x 48 Canny frames and 128 x 96 ROS frames halved once with two levels, against the manual loop."""
import os

import numpy as np
import pytest

import point_select_cases as pc
import point_select_ref as ps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q0, T0 = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)
POSE = (np.array([0.9995, 0.01, -0.02, 0.015]), np.array([0.01, -0.02, 0.03]))


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dtype(hip, name):
    return hip.EA_F64 if name == "f64" else hip.EA_F32


def _dt_grid(seed=0, H=pc.H, W=pc.W):
    dt = np.random.default_rng(seed).uniform(0.0, 1.0, (H, W)).astype(np.float32)
    return np.ascontiguousarray(dt.astype(np.float64).T)


def _problem(hip, dtype, xyz=None, w=None, dt=True, K=pc.K):
    P = hip.Problem(*K, dtype=dtype)
    if dt:
        P.set_dt_grid(_dt_grid())
    _load(P, xyz, w)
    return P


def _load(P, xyz, w):
    P.set_points(xyz if xyz is not None else np.zeros((0, 3)))
    if w is not None and len(w):
        P.set_weights(w)


def _same_eval(a, b, at):
    for key in ("cost", "JtJ", "Jtr"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (at, key)
    assert a["n_invalid"] == b["n_invalid"], at


def _holds(P, xyz, w, kept, at):
    """problem P holds exactly xyz[kept] (and w[kept]), bit for bit"""
    assert P.num_points == len(kept), (at, P.num_points, len(kept))
    assert np.array_equal(_bits(P.get_points()), _bits(xyz[kept])), at
    got = P.get_weights()
    if w is None or len(kept) == 0:
        assert got is None, at
    else:
        assert got is not None and np.array_equal(_bits(got), _bits(w[kept])), at


# ---- every combination on the synthetic points ------------------------------------------------------------------------------

@pytest.mark.parametrize("cell_px", pc.CELLS)
@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_points_weights_and_stats_are_the_restatement(hip, dtype_name, cell_px):
    f32 = dtype_name == "f32"
    P, F = _problem(hip, _dtype(hip, dtype_name)), _problem(hip, _dtype(hip, dtype_name))
    thinned = cells_won = strided = bypassed = 0
    try:
        for n in pc.SIZES:
            xyz = pc.stored(pc.points(n, 100 + n), f32)
            for w in (None, pc.weights(n, n)):
                for prm in pc.param_sets(n):
                    if prm["cell_px"] != cell_px:
                        continue
                    at = (dtype_name, n, w is not None, prm)
                    kept, want = ps.select(xyz, pc.K, pc.H, pc.W, **prm)
                    _load(P, xyz, w)
                    assert P.num_points == n and (n == 0 or np.array_equal(_bits(P.get_points()), _bits(xyz))), at
                    # the extent: the DT image's, or named -- the same grid
                    extent = dict(height=pc.H, width=pc.W) if prm["outside"] else {}
                    got = P.select_points(**prm, **extent)
                    assert got == want, (at, got, want)
                    _holds(P, xyz, w, kept, at)
                    if len(kept):
                        _load(F, xyz[kept], None if w is None else w[kept])
                        _same_eval(P.eval(*POSE), F.eval(*POSE), at)
                    thinned += int(0 < want["n_after"] < n)
                    cells_won += int(0 < want["after_cells"] < n - want["no_pixel"])
                    strided += int(want["stride_used"] > 1)
                    bypassed += int(prm["outside"] == 1 and want["no_pixel"] > 0 and prm["cell_px"] > 0)
        assert thinned > 0 and strided > 0                      # nothing here is vacuous
        assert cell_px == 0 or (cells_won > 0 and bypassed > 0)
    finally:
        P.close()
        F.close()


def test_nearest_and_first_disagree_where_a_later_point_is_nearer(hip):
    """the two rules on one crowded cell: FIRST keeps index 0, NEAREST the smallest z, and of equal z the lowest index"""
    uvz = [(9, 6, 2.0), (9, 6, 1.0), (10, 7, 1.0), (9, 6, 3.0), (30, 20, 1.5)]
    xyz = pc.back_project(np.array([p[0] for p in uvz], float), np.array([p[1] for p in uvz], float), np.array([p[2] for p in uvz]))
    P = _problem(hip, hip.EA_F64, xyz)
    try:
        assert P.select_points(cell_px=4, cell_rule=hip.CELL_FIRST)["n_after"] == 2
        assert np.array_equal(_bits(P.get_points()), _bits(xyz[[0, 4]]))
        _load(P, xyz, None)
        assert P.select_points(cell_px=4, cell_rule=hip.CELL_NEAREST)["n_after"] == 2
        assert np.array_equal(_bits(P.get_points()), _bits(xyz[[1, 4]]))
    finally:
        P.close()


def test_the_scan_carries_across_its_chunks(hip):
    """1024 * 1024 + 5 points are 4097 block counts: four full chunks of the scan and one count more"""
    n = 1024 * 1024 + 5
    xyz, w = pc.points(n, 7), pc.weights(n, 7)
    P, F = _problem(hip, hip.EA_F64), _problem(hip, hip.EA_F64)
    P.set_point_order(0)                                       # (a set this large would be stored in tiles: out of scope)
    F.set_point_order(0)
    try:
        for prm in (dict(stride=7), dict(cell_px=1, cell_rule=1, outside=1, stride=7)):
            kept, want = ps.select(xyz, pc.K, pc.H, pc.W, **prm)
            _load(P, xyz, w)
            assert P.select_points(**prm) == want, prm
            assert want["n_after"] > 1024 * 16 and want["stride_used"] == 7
            _holds(P, xyz, w, kept, prm)
        _load(F, xyz[kept], w[kept])
        _same_eval(P.eval(*POSE), F.eval(*POSE), "big")
    finally:
        P.close()
        F.close()


# ---- batches ------------------------------------------------------------------------------------------------------------------

def test_a_batch_thins_the_selected_problems_only(hip):
    sizes = (1025, 300, 0)
    xyz = [pc.points(n, 40 + n) for n in sizes]
    w = [pc.weights(sizes[0], 1), None, None]
    Ps = [_problem(hip, hip.EA_F64, xyz[i], w[i]) for i in range(3)]
    B, B0, B1 = hip.Batch(Ps), hip.Batch([Ps[0]]), hip.Batch([Ps[1]])
    F = [_problem(hip, hip.EA_F64) for _ in range(2)]
    try:
        for b in (B0, B1):
            b.set_poses(POSE[0][None, None], POSE[1][None, None])
        before = {k: np.array(v) for k, v in B1.eval_resident_poses().items() if k != "_ptrs"}
        # the identity: nothing changes, no version moves (the resident poses of both batches survive)
        ident = B.select_points()
        assert ident == [dict(n_before=n, no_pixel=0, after_cells=n, n_after=n, stride_used=1) for n in sizes]
        assert Ps[0].select_points(outside=1, cell_rule=1)["n_after"] == sizes[0]
        B0.eval_resident_poses()
        B1.eval_resident_poses()
        for i in range(3):
            _holds(Ps[i], xyz[i], w[i], np.arange(sizes[i]), i)
        # sel = [2, 0]: the stats come in that order, problem 1 is not touched
        prm = dict(cell_px=4, cell_rule=1, outside=1, stride=2)
        stats = B.select_points(sel=[2, 0], **prm)
        kept0, want0 = ps.select(xyz[0], pc.K, pc.H, pc.W, **prm)
        assert stats == [dict(n_before=0, no_pixel=0, after_cells=0, n_after=0, stride_used=1), want0]
        _holds(Ps[0], xyz[0], w[0], kept0, "selected")
        _holds(Ps[1], xyz[1], None, np.arange(sizes[1]), "unselected")
        _holds(Ps[2], xyz[2], None, np.arange(0), "empty")
        after = B1.eval_resident_poses()                       # (raises if problem 1's version had moved)
        for key in ("cost", "JtJ", "Jtr"):
            assert np.array_equal(_bits(before[key]), _bits(after[key])), key
        with pytest.raises(hip.EAError) as ei:                 # problem 0's version moved: its batch dropped the poses
            B0.eval_resident_poses()
        assert ei.value.code == hip.EA_ERR_STATE
        # a solve of the thinned batch equals the solve of fresh problems with the restatement's survivors
        two = hip.Batch(Ps[:2])
        _load(F[0], xyz[0][kept0], w[0][kept0])
        _load(F[1], xyz[1], None)
        fresh = hip.Batch(F)
        q0, t0 = np.tile(Q0, (2, 1)), np.zeros((2, 3))
        q, t, sums = two.solve(q0, t0)
        qf, tf, sums_f = fresh.solve(q0, t0)
        assert np.array_equal(_bits(q), _bits(qf)) and np.array_equal(_bits(t), _bits(tf))
        for a, b in zip(sums, sums_f):
            assert a["termination"] == b["termination"] and a["num_iterations"] == b["num_iterations"]
            assert np.array_equal(_bits(a["final_cost"]), _bits(b["final_cost"]))
        two.close()
        fresh.close()
        # errors: before anything changes
        for bad in (dict(sel=[0, 0]), dict(sel=[0, 3]), dict(sel=[-1]), dict(cell_px=4097), dict(stride=0), dict(stride=2, target=3),
                    dict(cell_rule=2), dict(outside=2), dict(target=-1), dict(height=5), dict(height=-1, width=-1),
                    dict(cell_px=1, height=8193, width=8192)):
            with pytest.raises(hip.EAError) as ei:
                B.select_points(**bad)
            assert ei.value.code == hip.EA_ERR_INVALID_ARG, bad
        _holds(Ps[0], xyz[0], w[0], kept0, "after the refused calls")
    finally:
        for b in (B, B0, B1):
            b.close()
        for p in Ps + F:
            p.close()


def test_borrowed_points_become_owned(hip):
    import torch
    n = 1025
    xyz = pc.points(n, 5)
    dev = [torch.tensor(np.ascontiguousarray(xyz[:, c]), dtype=torch.float64, device="cuda") for c in range(3)]
    torch.cuda.synchronize()
    P = _problem(hip, hip.EA_F64)
    try:
        P.set_points_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n)
        prm = dict(cell_px=4, stride=3)
        kept, want = ps.select(xyz, pc.K, pc.H, pc.W, **prm)
        assert P.select_points(**prm) == want
        for c in range(3):                                     # the caller's arrays were read, not written
            assert np.array_equal(_bits(dev[c].cpu().numpy()), _bits(xyz[:, c]))
            dev[c].zero_()
        torch.cuda.synchronize()
        _holds(P, xyz, None, kept, "owned")                    # and the problem no longer reads them
        P.set_weights(np.ones(len(kept)))                      # (weights need owned points: nothing is copied again)
        _holds(P, xyz, np.ones(n), kept, "owned, weighted")
    finally:
        P.close()


def test_state_errors_leave_the_problem_as_it_was(hip):
    xyz = pc.points(300, 9)
    T = hip.Problem(*pc.K, dtype=hip.EA_F64)
    N = _problem(hip, hip.EA_F64, xyz, dt=False)
    try:
        T.set_dt_grid(_dt_grid())
        T.set_point_order(4)
        T.set_points(xyz)
        assert T.point_order == 4
        with pytest.raises(hip.EAError) as ei:
            T.select_points(stride=2)
        assert ei.value.code == hip.EA_ERR_STATE and "ea_problem_set_point_order(p, 0)" in str(ei.value)
        assert T.num_points == 300 and np.array_equal(_bits(T.get_points()), _bits(xyz))
        # no DT image and no extent: the cell step has no grid; the stride step needs none
        with pytest.raises(hip.EAError) as ei:
            N.select_points(cell_px=4)
        assert ei.value.code == hip.EA_ERR_STATE and N.num_points == 300
        kept, want = ps.select(xyz, pc.K, pc.H, pc.W, cell_px=4)
        assert N.select_points(cell_px=4, height=pc.H, width=pc.W) == want
        _holds(N, xyz, None, kept, "named extent")
        assert N.select_points(stride=2)["n_after"] == (len(kept) + 1) // 2
        # everything dropped: a problem without points, and without weights
        behind = xyz.copy()
        behind[:, 2] = -1.0
        _load(N, behind, pc.weights(300, 1))
        want = ps.select(behind, pc.K, pc.H, pc.W, cell_px=4)[1]
        assert want["no_pixel"] == 300 and want["n_after"] == 0
        assert N.select_points(cell_px=4, height=pc.H, width=pc.W) == want
        assert N.num_points == 0 and N.get_weights() is None
        assert N.select_points(stride=3) == dict(n_before=0, no_pixel=0, after_cells=0, n_after=0, stride_used=1)
    finally:
        T.close()
        N.close()


# ---- a producer's points: the bundled frame -----------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def frame():
    from oracle import preprocess_np as pp
    G = os.path.join(ROOT, "tests", "golden", "rgbd")
    K = (525.0, 525.0, 319.5, 239.5)
    bgr, depth = pp.load_rgb_as_bgr(os.path.join(G, "rgb_1.png")), pp.load_depth_u16(os.path.join(G, "depth_1.png"))
    aX, _ = pp.get_aX(bgr, depth, *K)
    return dict(K=K, bgr=bgr, depth=depth, aX=aX)


def test_the_references_stride_on_the_bundled_frame(hip, frame):
    """edge_align_test1's `i += 30`: 44 457 points become 1 482 blocks; and every back-projected point lands on its own pixel"""
    P = hip.Problem(*frame["K"], dtype=hip.EA_F64)
    try:
        P.set_depth_weighting(2.0, 2)
        P.set_ref_frame(frame["bgr"], frame["depth"])
        pts, w = P.get_points(), P.get_weights()
        assert P.num_points == 44457 == frame["aX"].shape[1] and w is not None
        H, W = frame["depth"].shape
        # cell_px = 1, FIRST: one point per pixel -- every point is kept, so none shares a pixel or lost its own to rounding
        st = P.select_points(cell_px=1, cell_rule=hip.CELL_FIRST, height=H, width=W)
        assert st == dict(n_before=44457, no_pixel=0, after_cells=44457, n_after=44457, stride_used=1)
        assert st == ps.select(pts, frame["K"], H, W, cell_px=1)[1]
        _holds(P, pts, w, np.arange(44457), "cell_px = 1")
        st = P.select_points(stride=30)
        assert st == dict(n_before=44457, no_pixel=0, after_cells=44457, n_after=1482, stride_used=30)
        assert np.array_equal(P.get_points(), frame["aX"][:3, 0::30].T)
        assert np.array_equal(_bits(P.get_weights()), _bits(w[0::30]))            # the producer's weights of the survivors
        # the stereo tests' iterStep: N / minNumOfPointsPerimage when N exceeds it
        P.set_ref_frame(frame["bgr"], frame["depth"])
        st = P.select_points(target=3000)
        assert st["stride_used"] == 44457 // 3000 == 14 and st["n_after"] == len(range(0, 44457, 14))
        assert np.array_equal(P.get_points(), frame["aX"][:3, 0::14].T)
    finally:
        P.close()


def test_the_c_demo_prints_the_references_block_count(hip, frame, tmp_path):
    import subprocess
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "point_selection_demo"])
    H, W = frame["depth"].shape
    frame["bgr"].tofile(str(tmp_path / "bgr.u8"))
    frame["depth"].tofile(str(tmp_path / "depth.u16"))
    out = subprocess.check_output([os.path.join(ROOT, "examples", "point_selection_demo"), str(H), str(W)] + ["%r" % k for k in frame["K"]]
                                  + [str(tmp_path / "bgr.u8"), str(tmp_path / "depth.u16"), "8", "2000"], timeout=60).decode().split("\n")
    assert out[0] == "stride 44457 1482"
    pts = frame["aX"][:3].T
    want = ps.select(pts, frame["K"], H, W, cell_px=8, cell_rule=1, target=2000)[1]
    assert out[1] == "cells %d %d %d %d %d" % tuple(want[k] for k in ps.STAT_KEYS)


# ---- the multi-stream tracker -------------------------------------------------------------------------------------------------

import test_gpu_batch_frames_ros as ros                                            # noqa: E402
from test_gpu_tracker_batch import _knobs                                          # noqa: E402
from test_gpu_tracker_depth_gate import CONFIGS, N, Z, _cams, _Manual, _pushes, _same_summary, _tracker   # noqa: E402

SEL = dict(cell_px=4, target=200)
ZERO = dict(n_before=0, no_pixel=0, after_cells=0, n_after=0, stride_used=1)


def _level_extent(cfg, l):
    _, halvings, _, (FH, FW) = cfg
    return FH >> (halvings + l), FW >> (halvings + l)


def _select_level(hip, cfg, B, l, f32):
    """ea_batch_select_points over a level's batch of fresh problems, held to the restatement on the way; the stats per stream"""
    before = [(P.get_points(), P.get_weights()) for P in B.problems]
    stats = B.select_points(**SEL)
    H, W = _level_extent(cfg, l)
    for i, P in enumerate(B.problems):
        pts, w = before[i]
        kept, want = ps.select(pts, _cams(cfg)[l][i], H, W, **SEL)
        assert stats[i] == want, (l, i, stats[i], want)
        _holds(P, pts, w, kept, (l, i))
    return stats


class _SelectingManual(_Manual):
    """the manual loop of tests/test_gpu_tracker_depth_gate.py without a gate, with ea_batch_select_points between the batched
    producer and the solves: per push fresh problems take reference = frame k - 1, current = frame k"""

    def __init__(self, hip, cfg, dtype):
        super().__init__(hip, cfg, dtype, None)
        self.selected = {}

    def _set_frames(self, B, l, ref, now):
        super()._set_frames(B, l, ref, now)
        self.selected[l] = _select_level(self.hip, self.cfg, B, l, self.dtype == self.hip.EA_F32)


def _reference_of(hip, cfg, dtype, bgr, depth):
    """what a push leaves as every stream's reference: the batched producer on the pushed frame, then the selection"""
    manual = _SelectingManual(hip, cfg, dtype)
    out = {}
    for l in range(cfg[2]):
        Ps = [hip.Problem(*manual.cams[l][i], dtype=dtype) for i in range(N)]
        for i, P in enumerate(Ps):
            _knobs(P, i)
        B = hip.Batch(Ps)
        manual._set_frames(B, l, (bgr, depth), (bgr, depth))
        for i, P in enumerate(Ps):
            out[(l, i)] = (P.get_points(), P.get_weights(), manual.selected[l][i])
        B.close()
        for P in Ps:
            P.close()
    return out


def _holds_reference(tb, want, levels, at):
    rows = tb.last_point_selection()
    for (l, i), (pts, w, stats) in want.items():
        P = tb.level_problem(l, i)
        assert P.num_points == len(pts) and np.array_equal(_bits(P.get_points()), _bits(pts)), (at, l, i)
        got = P.get_weights()
        assert (got is None) == (w is None) and (w is None or np.array_equal(_bits(got), _bits(w))), (at, l, i)
        assert rows[l][i] == stats, (at, l, i, rows[l][i], stats)


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("name", ["canny", "pyramid"])
def test_selecting_pushes_equal_the_manual_loop(hip, name, dtype_name):
    cfg = CONFIGS[name]
    levels, dtype = cfg[2], _dtype(hip, dtype_name)
    tb, manual = _tracker(hip, cfg, dtype), _SelectingManual(hip, cfg, dtype)
    tb.set_point_selection(**SEL)
    thinned = 0
    try:
        assert tb.info("point_selection") == 1 and tb.last_point_selection() == [[dict(ZERO, stride_used=0)] * N] * levels
        for k, (bgr, depth) in enumerate(_pushes(cfg, 31, pushes=3, late=False)):
            at = (name, dtype_name, "push", k + 1)
            q, t, sums, aligned = tb.push_frames(bgr, depth, z_scaling=Z)
            want = manual.push(bgr, depth)
            assert list(aligned) == want["aligned"], (at, list(aligned), want["aligned"])
            assert np.array_equal(_bits(q), _bits(want["q"])) and np.array_equal(_bits(t), _bits(want["t"])), at
            for i in range(N):
                last = tb.last_summaries(i)
                for l in range(levels):
                    _same_summary(last[l], want["sums"][l][i], (at, "stream", i, "level", l))
                finest = [want["sums"][l][i] for l in range(levels) if want["sums"][l][i] is not None]
                _same_summary(sums[i], finest[0] if finest else None, (at, "stream", i))
            assert tb.info("selected") == N, at
            ref = _reference_of(hip, cfg, dtype, bgr, depth)
            _holds_reference(tb, ref, levels, at)
            thinned += sum(int(st["n_after"] < st["n_before"]) for _, _, st in ref.values())
            if k > 0:
                assert sum(want["aligned"]) > 0, at
        assert thinned > 0
    finally:
        ros._close(tb)


@pytest.mark.parametrize("name", ["canny", "pyramid"])
def test_selection_never_set_is_the_manual_loop_without_it(hip, name):
    """a tracker on which the selection is never set, and one on which it is set and switched off again, equal the manual loop
    of the batched producers and solves alone; nothing is selected"""
    cfg = CONFIGS[name]
    levels, dtype = cfg[2], hip.EA_F64
    never, off, manual = _tracker(hip, cfg, dtype), _tracker(hip, cfg, dtype), _Manual(hip, cfg, dtype, None)
    off.set_point_selection(**SEL)
    off.set_point_selection(None)
    try:
        for k, (bgr, depth) in enumerate(_pushes(cfg, 31, pushes=3, late=False)):
            at = (name, "push", k + 1)
            want = manual.push(bgr, depth)
            for tb in (never, off):
                q, t, sums, aligned = tb.push_frames(bgr, depth, z_scaling=Z)
                assert list(aligned) == want["aligned"], at
                assert np.array_equal(_bits(q), _bits(want["q"])) and np.array_equal(_bits(t), _bits(want["t"])), at
                for i in range(N):
                    for l in range(levels):
                        _same_summary(tb.last_summaries(i)[l], want["sums"][l][i], (at, i, l))
                assert tb.info("selected") == 0 and tb.info("point_selection") == 0, at
                assert all(row["n_before"] == 0 for lv in tb.last_point_selection() for row in lv), at
    finally:
        ros._close(never, off)


def test_a_kept_keyframe_is_not_selected_again(hip):
    """keyframe mode with every rule off: a stream keeps its first reference until it is reset.  A kept stream's points and
    stats row are what the push that took the reference left; a stream that takes the frame gets the frame's selection"""
    cfg = CONFIGS["canny"]
    dtype = hip.EA_F64
    tb = _tracker(hip, cfg, dtype)
    tb.set_keyframes(min_visible_fraction=0.0, min_inlier_fraction=0.0, max_mean_flow=0.0, max_frames=0)
    tb.set_point_selection(**SEL)
    kept = took = 0
    try:
        held = {}
        for k, (bgr, depth) in enumerate(_pushes(cfg, 31, pushes=3, late=False)):
            if k == 2:
                tb.reset(1)                                    # stream 1 is not aligned in push 3: it takes the frame
                assert tb.last_point_selection()[0][1]["n_before"] == 0
            tb.push_frames(bgr, depth, z_scaling=Z)
            ref = _reference_of(hip, cfg, dtype, bgr, depth)
            n_took = 0
            for i in range(N):
                if tb.keyframe_state(i)["replaced"]:
                    held[i] = ref[(0, i)]
                    n_took += 1
                    took += 1
                else:
                    kept += 1
            assert tb.info("selected") == n_took == tb.info("keyframes_taken"), k
            _holds_reference(tb, {(0, i): held[i] for i in range(N)}, 1, ("push", k + 1))
        assert kept > 0 and took > N                           # some kept, and one taken after the first push
    finally:
        ros._close(tb)
