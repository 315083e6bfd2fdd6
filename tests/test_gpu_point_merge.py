"""ea_*_transform_points and ea_*_merge_points on the device, and points carried across a keyframe replacement in the
multi-stream tracker, against tests/point_merge_ref.py, the numpy restatement of the header's rules.  Exactness is the
requirement -- there are no tolerances: every output is a stored value, an IEEE operation in a stated order rounded once, or an
integer minimum, so points, weights and stats are equal bit for bit, an evaluation of the merged problem equals the evaluation
of a fresh problem that was handed the restatement's arrays, and ea_problem_select_points applied afterwards equals the
restatement's selection of the merged set.

Shapes (tests/point_merge_cases.py): point selection's camera on its 37 x 29 grid; n in {0, 1, 63, 64, 65, 255, 256, 257, 2049}
(wavefront and workgroup edges of the 256-lane passes) on both sides; every filter alone and all together, cell_px in
{0, 1, 4, 64}, both rules, margin in {0, 3}, max_carried in {0, 1, 5, n}, the four weighted / unweighted combinations with
weight_scale in {1, 0.5}, both dtypes; one case of 1024 * 256 + 5 src points (1025 block counts: the scan carries across its
chunks of 1024); and the tracker on 64 x 48 Canny frames and 128 x 96 ROS frames halved once, four streams, in keyframe mode
with max_frames = 2, against the manual loop.  The EA_ERR_INVALID_ARG and EA_ERR_STATE rows that need a problem to exist are
here too (tests/test_point_merge_capi.py has the ones a NULL handle shows)."""
import os
import subprocess

import numpy as np
import pytest

import point_merge_cases as mc
import point_merge_ref as pm
import point_select_ref as ps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POSE = (np.array([0.9995, 0.01, -0.02, 0.015]), np.array([0.01, -0.02, 0.03]))
AFTER = dict(cell_px=4, cell_rule=1, target=50)                 # the selection applied to a merged set
ZERO = dict.fromkeys(pm.STAT_KEYS, 0)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _dtype(hip, name):
    return hip.EA_F64 if name == "f64" else hip.EA_F32


def _problem(hip, dtype, xyz=None, w=None, dt=True):
    P = hip.Problem(*mc.K, dtype=dtype)
    P.set_point_order(0)
    if dt:
        P.set_dt_grid(np.ascontiguousarray(mc.dt_image().T))
    _load(P, xyz, w)
    return P


def _load(P, xyz, w):
    P.set_points(xyz if xyz is not None else np.zeros((0, 3)))
    if w is not None and len(w):
        P.set_weights(w)


def _holds(P, xyz, w, at):
    """problem P holds exactly the points xyz and the weights w (None: unweighted), bit for bit"""
    assert P.num_points == len(xyz), (at, P.num_points, len(xyz))
    assert np.array_equal(_bits(P.get_points()), _bits(xyz)), at
    got = P.get_weights()
    if w is None or len(xyz) == 0:
        assert got is None, at
    else:
        assert got is not None and np.array_equal(_bits(got), _bits(w)), at


def _same_eval(a, b, at):
    for key in ("cost", "JtJ", "Jtr"):
        assert np.array_equal(_bits(a[key]), _bits(b[key])), (at, key)
    assert a["n_invalid"] == b["n_invalid"], at


# ---- transform ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_transformed_points_are_the_restatement(hip, dtype_name):
    f32 = dtype_name == "f32"
    P = _problem(hip, _dtype(hip, dtype_name), dt=False)
    try:
        for n in mc.SIZES:
            for k, (name, M) in enumerate(mc.MATRICES.items()):
                at = (dtype_name, n, name)
                xyz = mc.src_points(n, n, M)
                sp = mc.special_points()
                xyz[:min(n, len(sp))] = sp[:n]                 # NaN, +-Inf, +-0 and z <= 0 lead every set that has room
                xyz = mc.pc.stored(xyz, f32)
                w = mc.pc.weights(n, n) if k % 2 and n else None
                _load(P, xyz, w)
                P.transform_points(M)
                once = pm.transform(xyz, M, f32)
                _holds(P, once, w, at)
                # two chained transforms equal the restatement's chain: each call rounds to the dtype
                P.transform_points(mc.MATRICES["nonrigid"])
                _holds(P, pm.transform(once, mc.MATRICES["nonrigid"], f32), w, (at, "chain"))
        xyz = mc.pc.stored(mc.src_points(2049, 1, mc.MATRICES["rigid"]), f32)
        _load(P, xyz, None)
        P.transform_points(mc.MATRICES["rigid"])
        P.transform_points(mc.MATRICES["nonrigid"])
        product = pm.transform(xyz, mc.MATRICES["nonrigid"] @ mc.MATRICES["rigid"], f32)
        assert not np.array_equal(_bits(P.get_points()), _bits(product))           # (the chain is not the product matrix)
        # a (q, t) tuple is ea_pose_to_matrix's matrix
        _load(P, xyz, None)
        P.transform_points(POSE)
        _holds(P, pm.transform(xyz, hip.pose_to_matrix(*POSE), f32), None, "pose tuple")
    finally:
        P.close()


def test_a_batch_transforms_the_selected_problems_in_one_call(hip):
    import torch
    sizes = (2049, 257, 0, 65)
    xyz = [mc.src_points(n, 20 + n, mc.SMALL) for n in sizes]
    w = [mc.pc.weights(sizes[0], 3), None, None, None]
    Ps = [_problem(hip, hip.EA_F64, xyz[i], w[i]) for i in range(3)] + [_problem(hip, hip.EA_F64)]
    dev = [torch.tensor(np.ascontiguousarray(xyz[3][:, c]), dtype=torch.float64, device="cuda") for c in range(3)]
    torch.cuda.synchronize()
    Ps[3].set_points_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), sizes[3])    # borrowed points
    B, B1 = hip.Batch(Ps), hip.Batch([Ps[1]])
    Ms = [mc.MATRICES["rigid"], mc.MATRICES["nonrigid"], mc.MATRICES["translation"], mc.SMALL]
    try:
        B1.set_poses(POSE[0][None, None], POSE[1][None, None])
        B1.eval_resident_poses()
        B.transform_points([Ms[3], Ms[0]], sel=[3, 0])
        _holds(Ps[0], pm.transform(xyz[0], Ms[0]), w[0], "selected")
        _holds(Ps[1], xyz[1], None, "unselected")
        _holds(Ps[3], pm.transform(xyz[3], Ms[3]), None, "borrowed")
        for c in range(3):                                     # the caller's arrays were read, not written
            assert np.array_equal(_bits(dev[c].cpu().numpy()), _bits(xyz[3][:, c]))
        B1.eval_resident_poses()                               # (raises if problem 1's version had moved)
        B.transform_points(np.stack(Ms))
        _holds(Ps[1], pm.transform(xyz[1], Ms[1]), None, "all")
        _holds(Ps[0], pm.transform(pm.transform(xyz[0], Ms[0]), Ms[0]), w[0], "all, twice")
        with pytest.raises(hip.EAError) as ei:                 # problem 1's version moved: its batch dropped the poses
            B1.eval_resident_poses()
        assert ei.value.code == hip.EA_ERR_STATE
        # errors: before anything changes
        held = Ps[1].get_points()
        bad_row = np.eye(4)
        bad_row[3, 0] = 1e-300
        nan = np.eye(4)
        nan[1, 2] = np.nan
        for kw in (dict(M=[np.eye(4)] * 2, sel=[1, 1]), dict(M=[np.eye(4)], sel=[4]), dict(M=[np.eye(4)], sel=[-1]),
                   dict(M=[np.eye(4), bad_row], sel=[1, 0]), dict(M=[nan, np.eye(4)], sel=[1, 0])):
            with pytest.raises(hip.EAError) as ei:
                B.transform_points(**kw)
            assert ei.value.code == hip.EA_ERR_INVALID_ARG, kw
        assert np.array_equal(_bits(Ps[1].get_points()), _bits(held))
        # a storage order: the same message as point selection
        T = hip.Problem(*mc.K, dtype=hip.EA_F64)
        T.set_point_order(4)
        T.set_points(xyz[1])
        with pytest.raises(hip.EAError) as ei:
            T.transform_points(np.eye(4))
        assert ei.value.code == hip.EA_ERR_STATE and "ea_problem_set_point_order(p, 0)" in str(ei.value)
        T.close()
    finally:
        B.close()
        B1.close()
        for P in Ps:
            P.close()


# ---- merge: the case table ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_merged_points_weights_and_stats_are_the_restatement(hip, dtype_name):
    f32 = dtype_name == "f32"
    dtype = _dtype(hip, dtype_name)
    D, S, F = _problem(hip, dtype), _problem(hip, dtype, dt=False), _problem(hip, dtype)
    dt = mc.dt_image()
    carried = unchanged = thinned = 0
    try:
        assert np.array_equal(_bits(D.get_dt()), _bits(dt))
        for case in mc.cases():
            at = (dtype_name, case["name"], case["params"])
            dst, dw, src, sw, M = mc.build(case, f32)
            _load(D, dst, dw)
            _load(S, src, sw)
            pts, w, want, kept = pm.merge(dst, dw, src, sw, M, mc.K, dt, f32, **case["params"])
            got = D.merge_points(S, M, **case["params"])
            assert got == want, (at, got, want)
            _holds(D, pts, w, at)
            _holds(S, src, sw, (at, "src"))                    # src is not touched
            carried += int(want["carried"] > 0)
            unchanged += int(want["carried"] == 0 and want["n_src"] > 0)
            if len(pts) == 0:
                continue
            _load(F, pts, w)
            _same_eval(D.eval(*POSE), F.eval(*POSE), at)
            # the selection of the merged set: what step 1's rounding is for
            sel_kept, sel_want = ps.select(pts, mc.K, mc.H, mc.W, **AFTER)
            assert D.select_points(**AFTER) == sel_want, (at, "select")
            _holds(D, pts[sel_kept], None if w is None else w[sel_kept], (at, "select"))
            thinned += int(sel_want["n_after"] < len(pts))
        assert carried > 0 and unchanged > 0 and thinned > 0    # nothing here is vacuous
    finally:
        for P in (D, S, F):
            P.close()


def test_the_scan_carries_across_its_chunks(hip):
    """1024 * 256 + 5 src points are 1025 block counts: one full chunk of the scan and one count more"""
    n = 1024 * 256 + 5
    src, sw = mc.src_points(n, 7, mc.SMALL), mc.pc.weights(n, 7)
    dst = mc.dst_points(257, 7)
    D, S = _problem(hip, hip.EA_F64), _problem(hip, hip.EA_F64, src, sw, dt=False)
    dt = mc.dt_image()
    try:
        for prm in (dict(require_pixel=1, max_carried=150000), dict(cell_px=1, cell_rule=1, max_dt=2.0, weight_scale=0.5)):
            _load(D, dst, None)
            pts, w, want, kept = pm.merge(dst, None, src, sw, mc.SMALL, mc.K, dt, **prm)
            assert D.merge_points(S, mc.SMALL, **prm) == want, prm
            _holds(D, pts, w, prm)
            assert want["capped"] > 0 or want["lost_cell"] > 1024 * 64, want
        _load(D, dst, None)
        pts, w, want, kept = pm.merge(dst, None, src, sw, mc.SMALL, mc.K, dt, require_pixel=1)
        assert D.merge_points(S, mc.SMALL, require_pixel=1) == want and want["carried"] > 1024 * 64 and kept.max() > 1024 * 256
        _holds(D, pts, w, "require_pixel")
    finally:
        D.close()
        S.close()


def test_a_batch_of_three_equals_three_single_calls(hip):
    cases = [c for c in mc.cases() if c["n_src"] in (257, 2049, 65) and c["n_dst"] > 0][:3]
    prm = dict(require_pixel=1, margin=3, max_dt=1.5, cell_px=4, cell_rule=1, max_carried=40, weight_scale=0.5)
    data = [mc.build(c, False) for c in cases]
    one = [_problem(hip, hip.EA_F64, d[0], d[1]) for d in data]
    many = [_problem(hip, hip.EA_F64, d[0], d[1]) for d in data]
    srcs = [_problem(hip, hip.EA_F64, d[2], d[3], dt=False) for d in data]
    spare = _problem(hip, hip.EA_F64, data[0][0], None)
    B = hip.Batch(many + [spare])
    try:
        singles = [one[i].merge_points(srcs[i], data[i][4], **prm) for i in range(3)]
        order = [2, 0, 1]
        stats = B.merge_points([srcs[i] for i in order], [data[i][4] for i in order], sel=order, **prm)
        assert stats == [singles[i] for i in order] and sum(s["carried"] for s in stats) > 0
        for i in range(3):
            _holds(many[i], one[i].get_points(), one[i].get_weights(), i)
            pts, w, want, _ = pm.merge(data[i][0], data[i][1], data[i][2], data[i][3], data[i][4], mc.K, mc.dt_image(), **prm)
            assert singles[i] == want
            _holds(one[i], pts, w, (i, "restatement"))
        _holds(spare, data[0][0], None, "unselected")
    finally:
        B.close()
        for P in one + many + srcs + [spare]:
            P.close()


def test_special_cases_and_errors(hip):
    src = mc.src_points(300, 2, mc.SMALL)
    dst = mc.dst_points(65, 2)
    D, S = _problem(hip, hip.EA_F64, dst), _problem(hip, hip.EA_F64, src, dt=False)
    E, N32 = _problem(hip, hip.EA_F64, dt=False), _problem(hip, hip.EA_F32, src, dt=False)
    B0 = hip.Batch([D])
    try:
        B0.set_poses(POSE[0][None, None], POSE[1][None, None])
        B0.eval_resident_poses()
        # carried == 0 changes nothing and moves no version: an empty src, and a filter nothing passes
        assert D.merge_points(E, mc.SMALL) == dict(ZERO, n_dst=65, n_after=65)
        st = D.merge_points(S, mc.SMALL, require_pixel=1, margin=15)
        assert st == dict(ZERO, n_dst=65, n_src=300, no_pixel=300, n_after=65)
        _holds(D, dst, None, "nothing carried")
        B0.eval_resident_poses()                               # (raises if the version had moved)
        # a dst without points and every filter off is a_X2 = T * a_X; no extent or DT image is needed for it
        assert E.merge_points(S, mc.SMALL) == dict(ZERO, n_src=300, carried=300, n_after=300)
        _holds(E, pm.transform(src, mc.SMALL), None, "copy")
        # the merge moved D's version
        assert D.merge_points(S, mc.SMALL, weight_scale=0.5)["carried"] == 300
        with pytest.raises(hip.EAError) as ei:
            B0.eval_resident_poses()
        assert ei.value.code == hip.EA_ERR_STATE
        _load(D, dst, None)
        # EA_ERR_INVALID_ARG, before anything changes
        B = hip.Batch([D, E])
        for kw in (dict(src=[S, S], M=[np.eye(4)] * 2, sel=[0, 0]), dict(src=[S], M=[np.eye(4)], sel=[2]),
                   dict(src=[S], M=[np.eye(4)], sel=[-1]), dict(src=[D], M=[np.eye(4)], sel=[0]),
                   dict(src=[E, S], M=[np.eye(4)] * 2, sel=[0, 1]), dict(src=[N32], M=[np.eye(4)], sel=[0]),
                   dict(src=[S], M=[np.eye(4)], sel=[0], max_dt=1.0, height=mc.H + 1, width=mc.W)):
            with pytest.raises(hip.EAError) as ei:
                B.merge_points(**kw)
            assert ei.value.code == hip.EA_ERR_INVALID_ARG, kw
        B.close()
        with pytest.raises(hip.EAError) as ei:
            D.merge_points(D, np.eye(4))
        assert ei.value.code == hip.EA_ERR_INVALID_ARG and "dst == src" in str(ei.value)
        # EA_ERR_STATE: no extent for a pixel test, no DT image for the edge test, a storage order on either side
        _load(E, None, None)
        for prm in (dict(require_pixel=1), dict(cell_px=4), dict(max_dt=1.0), dict(max_dt=1.0, height=mc.H, width=mc.W)):
            with pytest.raises(hip.EAError) as ei:
                E.merge_points(S, mc.SMALL, **prm)
            assert ei.value.code == hip.EA_ERR_STATE, prm
        want = pm.merge(np.zeros((0, 3)), None, src, None, mc.SMALL, mc.K, None, cell_px=4, height=mc.H, width=mc.W)
        assert E.merge_points(S, mc.SMALL, cell_px=4, height=mc.H, width=mc.W) == want[2]   # a named extent serves
        _holds(E, want[0], None, "named extent")
        T = hip.Problem(*mc.K, dtype=hip.EA_F64)
        T.set_point_order(4)
        T.set_points(src)
        for a, b in ((D, T), (T, S)):
            with pytest.raises(hip.EAError) as ei:
                a.merge_points(b, mc.SMALL)
            assert ei.value.code == hip.EA_ERR_STATE and "ea_problem_set_point_order(p, 0)" in str(ei.value)
        T.close()
        _holds(D, dst, None, "after the refused calls")
        _holds(S, src, None, "src after the refused calls")
    finally:
        B0.close()
        for P in (D, S, E, N32):
            P.close()


def test_borrowed_points_on_both_sides(hip):
    import torch
    src, dst = mc.src_points(257, 5, mc.SMALL), mc.dst_points(65, 5)
    dev = [torch.tensor(np.ascontiguousarray(a[:, c]), dtype=torch.float64, device="cuda") for a in (dst, src) for c in range(3)]
    torch.cuda.synchronize()
    D, S = _problem(hip, hip.EA_F64), _problem(hip, hip.EA_F64, dt=False)
    try:
        D.set_points_device(*[d.data_ptr() for d in dev[:3]], 65)
        S.set_points_device(*[d.data_ptr() for d in dev[3:]], 257)
        prm = dict(cell_px=4, weight_scale=0.5)
        pts, w, want, _ = pm.merge(dst, None, src, None, mc.SMALL, mc.K, mc.dt_image(), **prm)
        assert D.merge_points(S, mc.SMALL, **prm) == want and want["carried"] > 0
        for k, a in enumerate((dst, src)):                     # the callers' arrays were read, not written
            for c in range(3):
                assert np.array_equal(_bits(dev[3 * k + c].cpu().numpy()), _bits(a[:, c]))
        for d in dev[:3]:
            d.zero_()
        torch.cuda.synchronize()
        _holds(D, pts, w, "owned")                             # and dst no longer reads its old arrays
    finally:
        D.close()
        S.close()


def test_the_c_demo_places_copies_and_solves(hip):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "model_prior_demo"])
    out = subprocess.check_output([os.path.join(ROOT, "examples", "model_prior_demo")], timeout=60).decode().split("\n")
    assert out[0] == "points 240 240" and out[1] == "merge 0 240 240 240" and out[2].startswith("cost "), out


# ---- the multi-stream tracker ---------------------------------------------------------------------------------------------------

import test_gpu_batch_frames_ros as ros                                            # noqa: E402
from test_gpu_tracker_batch import _knobs, _ros_pushes, _u16_pushes                # noqa: E402
from test_gpu_tracker_depth_gate import _same_summary                             # noqa: E402

N = 4
Z = 5000.0
PUSHES = 5
# name: flavour, halvings, full extent (H, W)
CONFIGS = {"canny": (1, 0, (48, 64)), "ros_h1": (2, 1, (96, 128))}
CARRIES = {"pixel": dict(require_pixel=1, margin=2, cell_px=2, cell_rule=1, weight_scale=0.5), "edge": dict(max_dt=0.25, max_carried=40)}
SELECT = dict(cell_px=2, target=300)
Q_ID, T_ID = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)


def _frames(cfg, seed):
    flavour, halvings, (FH, FW) = cfg
    if flavour == 2:
        return _ros_pushes(FH >> halvings, FW >> halvings, halvings, N, PUSHES, seed)
    return _u16_pushes(FH, FW, N, PUSHES, seed)


def _cams(cfg):
    _, halvings, (FH, FW) = cfg
    return [ros._camera(i, FH >> halvings, FW >> halvings) for i in range(N)]


def _tracker(hip, cfg, dtype, carry, select):
    tb = hip.TrackerBatch(_cams(cfg), dtype=dtype, flavour=cfg[0], halvings=cfg[1])
    for i in range(N):
        _knobs(tb.problem(i), i)
    tb.set_keyframes(min_visible_fraction=0.0, min_inlier_fraction=0.0, max_mean_flow=0.0, max_frames=2)
    if carry is not None:
        tb.set_point_carry(**carry)
    if select:
        tb.set_point_selection(**SELECT)
    return tb


class _Manual:
    """the manual loop: per push fresh problems take the batched producer on the pushed frame (reference and image); a stream
    that holds a reference is solved, from its start pose, on a fresh problem that was handed the held points and weights
    under the frame's image; a stream that replaces takes the producer's points, and where it carries Batch.merge_points with
    the held reference and the returned pose, then select_points when set.  Which streams replace, and why, is read off the
    tracker (ea_tracker_batch_keyframe_state): the rule is tests/test_gpu_tracker_keyframes.py's business"""

    def __init__(self, hip, cfg, dtype, carry, select):
        self.hip, self.cfg, self.dtype, self.carry, self.select = hip, cfg, dtype, carry, select
        self.cams = _cams(cfg)
        self.held = [None] * N                                 # per stream (points, weights)
        self.start = [(Q_ID.copy(), T_ID.copy()) for _ in range(N)]

    def _produce(self, bgr, depth):
        Ps = [self.hip.Problem(*self.cams[i], dtype=self.dtype) for i in range(N)]
        for i, P in enumerate(Ps):
            P.set_point_order(0)
            _knobs(P, i)
        B = self.hip.Batch(Ps)
        if self.cfg[0] == 1:
            B.set_frames_canny(bgr, depth, bgr, z_scaling=Z)
        else:
            B.set_frames_ros(bgr, depth, bgr, halvings=self.cfg[1])
        return Ps, B

    def solve(self, bgr, depth):
        """poses and summaries of the streams that hold a reference, against the pushed frame"""
        hip = self.hip
        S, BS = self._produce(bgr, depth)
        BS.close()
        al = [i for i in range(N) if self.held[i] is not None and len(self.held[i][0])]
        out = dict(aligned=[int(i in al) for i in range(N)], sums=[None] * N, q=[s[0].copy() for s in self.start],
                   t=[s[1].copy() for s in self.start], failed=set())
        groups = {}
        for i in al:
            _load(S[i], *self.held[i])
            groups.setdefault(self.held[i][1] is not None, []).append(i)
        for grp in groups.values():
            B = hip.Batch([S[i] for i in grp])
            q, t, ss = B.solve(np.stack([self.start[i][0] for i in grp]), np.stack([self.start[i][1] for i in grp]))
            for k, i in enumerate(grp):
                out["sums"][i] = ss[k]
                if ss[k]["termination"] == hip.FAILURE:
                    out["failed"].add(i)
                else:
                    out["q"][i], out["t"][i] = q[k], t[k]
            B.close()
        self.S = S
        return out

    def references(self, bgr, depth, solved, why):
        """the references after the push; returns the merge's stats per stream (zeros: it did not carry)"""
        hip = self.hip
        f32 = self.dtype == hip.EA_F32
        F, B = self._produce(bgr, depth)
        take = [i for i in range(N) if why[i]]
        carrying = [i for i in take if self.carry is not None and not (why[i] & (hip.KEY_FIRST | hip.KEY_SOLVE_FAILED))
                    and self.held[i] is not None and len(self.held[i][0])]
        stats = [dict(ZERO) for _ in range(N)]
        if carrying:
            M = [hip.pose_to_matrix(solved["q"][i], solved["t"][i]) for i in carrying]
            before = [(F[i].get_points(), F[i].get_weights(), F[i].get_dt()) for i in carrying]
            got = B.merge_points([self.S[i] for i in carrying], M, sel=carrying, **self.carry)
            for k, i in enumerate(carrying):                   # the device merge is the restatement's on the way
                pts, w, want, _ = pm.merge(before[k][0], before[k][1], self.held[i][0], self.held[i][1], M[k], self.cams[i],
                                           before[k][2], f32, **self.carry)
                assert got[k] == want, (i, got[k], want)
                _holds(F[i], pts, w, ("manual merge", i))
                stats[i] = got[k]
        if self.select and take:
            B.select_points(sel=take, **SELECT)
        for i in range(N):
            if why[i]:
                self.held[i] = (F[i].get_points(), F[i].get_weights())
                self.start[i] = (Q_ID.copy(), T_ID.copy())
            elif solved["aligned"][i] and i not in solved["failed"]:
                self.start[i] = (solved["q"][i].copy(), solved["t"][i].copy())
        B.close()
        for P in F + self.S:
            P.close()
        return stats, len(carrying)


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("carry", ["pixel", "edge"])
@pytest.mark.parametrize("name", ["canny", "ros_h1"])
def test_carrying_pushes_equal_the_manual_loop(hip, name, carry, dtype_name):
    cfg, dtype = CONFIGS[name], _dtype(hip, dtype_name)
    select = carry == "edge"
    tb, manual = _tracker(hip, cfg, dtype, CARRIES[carry], select), _Manual(hip, cfg, dtype, CARRIES[carry], select)
    plain = _tracker(hip, cfg, dtype, None, select)               # the same tracker without a carry
    carried = kept = replaced = together = 0
    try:
        assert tb.info("point_carry") == 1 and plain.info("point_carry") == 0 and tb.last_point_carry() == [ZERO] * N
        for k, (bgr, depth) in enumerate(_frames(cfg, 31)):
            at = (name, carry, dtype_name, "push", k + 1)
            want = manual.solve(bgr, depth)
            q, t, sums, aligned = tb.push_frames(bgr, depth, z_scaling=Z)
            # the poses and summaries: ea_batch_solve on the manual problems, which hold what the pushes so far have merged
            assert list(aligned) == want["aligned"], (at, list(aligned), want["aligned"])
            for i in range(N):
                _same_summary(sums[i], want["sums"][i], (at, "stream", i))
                if aligned[i]:
                    assert np.array_equal(_bits(q[i]), _bits(want["q"][i])) and np.array_equal(_bits(t[i]), _bits(want["t"][i])), (at, i)
            why = [tb.keyframe_state(i)["replaced"] for i in range(N)]
            stats, n_carrying = manual.references(bgr, depth, want, why)
            print(at, "why", why, "carry", [(s["n_src"], s["carried"]) for s in stats])
            assert tb.last_point_carry() == stats, (at, tb.last_point_carry(), stats)
            assert tb.info("carried") == n_carrying, at
            for i in range(N):
                _holds(tb.problem(i), manual.held[i][0], manual.held[i][1], (at, "stream", i))
            carried += sum(s["carried"] for s in stats)
            replaced += sum(int(bool(w)) for w in why)
            kept += sum(int(not w) for w in why)
            # a push in which no stream carries leaves what a tracker without a carry leaves, until the first point is carried
            if together == k and n_carrying == 0:
                pq, pt, psums, pal = plain.push_frames(bgr, depth, z_scaling=Z)
                assert np.array_equal(_bits(pq), _bits(q)) and np.array_equal(_bits(pt), _bits(t)) and list(pal) == list(aligned), at
                for i in range(N):
                    _same_summary(psums[i], sums[i], (at, "plain", i))
                    _holds(plain.problem(i), manual.held[i][0], manual.held[i][1], (at, "plain", i))
                for key in ("aligned", "keyframes_taken", "selected", "carried"):
                    assert plain.info(key) == tb.info(key), (at, key)
                together += 1
        assert kept > 0 and replaced > N and together >= 2      # some pushes keep, some replace, and two ran without a carry
        if carry == "pixel":
            assert carried > 0
    finally:
        ros._close(tb, plain)


def test_carry_needs_keyframe_mode_and_streams_without_a_reference(hip):
    cfg = CONFIGS["canny"]
    tb = hip.TrackerBatch(_cams(cfg), dtype=hip.EA_F64, flavour=1)
    try:
        with pytest.raises(hip.EAError) as ei:
            tb.set_point_carry(cell_px=4)
        assert ei.value.code == hip.EA_ERR_STATE and "keyframe mode" in str(ei.value)
        tb.set_point_carry(None)                               # switching it off is always allowed before a reference
        tb.set_keyframes(max_frames=2)
        tb.set_point_carry(cell_px=4)
        assert tb.info("point_carry") == 1
        bgr, depth = _frames(cfg, 31)[0]
        tb.push_frames(bgr, depth, z_scaling=Z)
        assert tb.info("carried") == 0 and tb.last_point_carry() == [ZERO] * N     # first keyframes carry nothing
        for call in (lambda: tb.set_point_carry(cell_px=2), lambda: tb.set_point_carry(None)):
            with pytest.raises(hip.EAError) as ei:
                call()
            assert ei.value.code == hip.EA_ERR_STATE and "holds a reference" in str(ei.value)
        tb.reset(-1)
        tb.set_point_carry(None)
        assert tb.info("point_carry") == 0
    finally:
        tb.close()
