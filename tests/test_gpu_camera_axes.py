"""Every path that reads the intrinsics, on an anisotropic, off-centre camera (border_band.camera_C: fy = 1.37 fx, the
principal point 3.25 pixels right of and 2.5 pixels above the centre), against the extended-precision restatement of
tests/border_band.py.  Every other plain-functor test of the suite has fx == fy and the principal point at the image
centre, where fx read for fy, cx and cy passed in the wrong order, or a principal point rebuilt from the extent change
nothing.  tests/test_camera_axes_reference.py shows that each of these mistakes moves the reference by at least 100
times the bounds used here, so none of them can pass.

Covered: the per-point and rows kernels, the fused kernel in its launch shapes / addressing forms / image forms, the
pose-batched kernels (lanes = points with both reductions, one pose per lane in its four instantiations under the three
losses -- the unweighted Cauchy cost through the running product --, resident poses), the cost-only kernel and its
fall-back, the riding fold, the fused-iteration solve, the starts kernel, the variant functors and the weighted kernels,
the integer-pixel cost and the quantile key pass; then all of these again in the ROS flavour (z_guard = 0, z_eps =
0.001, rotation applied transposed), which otherwise reaches the device only through the fused kernel; and solves end to
end on a solvable problem against the oracle's LM loop.

Workload and bounds are those of tests/test_gpu_border_band.py: 1000 points, >= half with a tap outside the image,
n_invalid == 0, all rows compared; the larger of the project's bar and 4x the CPU-measured deviation of plain arithmetic
of the kernel's precision from the reference (border_band.bounds) -- never a device figure.

Per case (test_per_point_and_rows_kernels, and test_ros_flavour_rows_sums_costs_and_quantiles for the rows marked ROS:
per-point kernel, rows kernel and one fused evaluation at the three poses): the largest deviation of plain arithmetic of
the kernel's precision from the reference (CPU), the bounds (smallest .. largest over the poses), and the largest
deviation of the device on an MI355X; r absolute, J and the sums relative to the largest entry.  profiles/LOG.md
("Camera axes") has the other kernels; every test prints its figures as BAND-GPU lines.

  fp64 case              | r: plain   bound              device  | J: plain   bound              device  | sums: plain bound              device
       27x41 noise       |    5.4e-15 1.0e-12            7.5e-15 |    1.5e-14 1.0e-12            1.1e-14 |       1.2e-14 1.0e-11            5.0e-15
       33x257 noise      |    4.5e-14 1.0e-12            4.2e-14 |    8.1e-14 1.0e-12            1.1e-13 |       3.6e-14 1.0e-11            4.2e-14
       160x120 noise     |    2.8e-14 1.0e-12            3.0e-14 |    6.2e-14 1.0e-12            5.3e-14 |       2.9e-14 1.0e-11            2.2e-14
       160x120 dt        |    5.9e-16 1.0e-12            4.6e-16 |    3.6e-14 1.0e-12            3.5e-14 |       5.1e-15 1.0e-11            4.7e-15
       27x41 noise ROS   |    9.3e-15 1.0e-12            1.0e-14 |    1.7e-14 1.0e-12            2.2e-14 |       5.6e-15 1.0e-11            7.6e-15
       160x120 noise ROS |    1.8e-14 1.0e-12            2.3e-14 |    6.8e-14 1.0e-12            6.0e-14 |       8.7e-14 1.0e-11            4.1e-14
  fp32 case              | r: plain   bound              device  | J: plain   bound              device  | sums: plain bound              device
       27x41 noise       |    3.4e-06 2.0e-05            3.6e-06 |    7.1e-06 2.0e-04            6.9e-06 |       5.3e-06 1.0e-04            4.2e-06
       33x257 noise      |    1.7e-05 4.1e-05 .. 6.8e-05 2.0e-05 |    3.4e-05 2.0e-04            5.2e-05 |       3.5e-05 1.0e-04 .. 1.4e-04 7.8e-05
       160x120 noise     |    1.1e-05 2.3e-05 .. 4.3e-05 1.7e-05 |    5.2e-05 2.0e-04 .. 2.1e-04 4.5e-05 |       9.2e-06 1.0e-04            8.6e-06
       160x120 dt        |    3.3e-07 2.0e-05            2.4e-07 |    2.3e-05 2.0e-04            2.2e-05 |       3.1e-06 1.0e-04            1.2e-06
       27x41 noise ROS   |    4.8e-06 2.0e-05            3.4e-06 |    9.5e-06 2.0e-04            5.3e-06 |       3.6e-06 1.0e-04            3.1e-06
       160x120 noise ROS |    1.2e-05 3.9e-05 .. 4.7e-05 1.3e-05 |    3.0e-05 2.0e-04            3.6e-05 |       2.8e-05 1.0e-04 .. 1.1e-04 1.9e-05

A case's largest device deviation stays within 2.3 times its largest plain-arithmetic deviation; the 4x rule decides only
in fp32, on r and the sums of the shapes from 120 pixels up.
"""
import itertools

import numpy as np
import pytest

import border_band as bb
from edge_alignment_amd import synth
from oracle import ea_numpy as en
from test_gpu_border_band import DIST, T12, TRACE

pytestmark = pytest.mark.gpu
N = bb.N_GPU
DTYPES = ("EA_F64", "EA_F32")
SHAPES = ((27, 41), (33, 257), (160, 120))
CASES = [(s, "noise") for s in SHAPES] + [((160, 120), "dt")]
TWO = [((27, 41), "noise"), ((160, 120), "noise")]
ROS = (0.0, 0.001, True)
FIELDS = ("cost", "JtJ", "Jtr", "n_invalid")
K_POSES = 65   # two wavefronts of the one-pose-per-lane kernel


def _ids(cases):
    return ["%dx%d-%s" % (s[0], s[1], k) for s, k in cases]


def _case(hip, shape, kind, dtype_name, **kw):
    return bb.Case(hip, shape[0], shape[1], kind, getattr(hip, dtype_name), camera="C", **kw)


def _poses():
    """the three POSES and seeded small perturbations of (Q_SMALL, T_SMALL): up to 0.05 degrees and half a millimetre, a
    fraction of a pixel at these focal lengths, so every pose keeps the border workload (asserted per case)"""
    rng = np.random.default_rng(65)
    out = list(bb.POSES)
    while len(out) < K_POSES:
        dq = bb.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0.0, 0.05)))
        out.append((synth.quat_mul(dq, bb.Q_SMALL), bb.T_SMALL + rng.uniform(-0.0005, 0.0005, 3)))
    return out


POSES65 = _poses()
Q65 = np.stack([p[0] for p in POSES65]).reshape(-1, 1, 4)
T65 = np.stack([p[1] for p in POSES65]).reshape(-1, 1, 3)


def _check_poses(c, got, loss, where, seen):
    for k, p in enumerate(POSES65):
        c.check_sums({f: got[f][k] for f in FIELDS}, p, loss, where + (k,), seen)


def _check_costs(c, got, loss, where):
    """cost-only results of the 65 poses: cost within the bound on the sums, n_invalid that of the reference (0)"""
    worst = 0.0
    for k, p in enumerate(POSES65):
        es, tol = c.sums(p, loss), c.tol(p, loss)
        d = bb.dev_rel(got["cost"][k, 0], es["cost"])
        worst = max(worst, d / tol["sums"])
        assert got["n_invalid"][k, 0] == es["n_invalid"] == 0, where + (k,)
        assert d <= tol["sums"], (c.name(), where, k, d, tol["sums"])
    return worst


# ---- a. per-point and rows kernels --------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,kind", CASES, ids=_ids(CASES))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_per_point_and_rows_kernels(hip, dtype_name, shape, kind):
    """eval_points (raw, corrected), Batch.eval_rows (both layouts, staged and direct stores) row by row, one Batch.eval;
    the loss rotates with the pose"""
    c = _case(hip, shape, kind, dtype_name)
    B = hip.Batch([c.P])
    try:
        for pi, pose in enumerate(bb.POSES):
            loss = bb.LOSSES[(pi + bb.SHAPES.index(shape)) % 3]
            c.P.set_loss(*loss)
            c.raw(pose)
            seen = {}
            for corrected in (False, True):
                r, J = c.P.eval_points(*pose, corrected=corrected)
                c.check_rows(r, J, pose, loss, corrected, ("eval_points", pi, corrected), seen)
                first = None
                for staged, layout in itertools.product((1, 0), (0, 1)):
                    B.set_tuning("rows_staged", staged)
                    rr, JJ, bad = B.eval_rows(*pose, corrected=corrected, layout=layout)
                    JJ = JJ if layout == 0 else JJ.T
                    where = ("eval_rows", pi, corrected, staged, layout)
                    assert bad == 0 and rr.dtype == c.np and JJ.shape == (N, 6), where
                    if first is None:
                        c.check_rows(rr, JJ, pose, loss, corrected, where, seen)
                        first = (rr.copy(), JJ.copy())
                    assert np.array_equal(rr, first[0]) and np.array_equal(JJ, first[1]), where
            c.check_sums(B.eval(*pose), pose, loss, ("eval", pi), seen)
            c.report(seen, pose, loss, "rows p%d l%d" % (pi, loss[0]))
    finally:
        B.close(); c.close()


# ---- b. fused kernel forms ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,kind", TWO, ids=_ids(TWO))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_fused_kernel_forms(hip, dtype_name, shape, kind):
    """Batch.eval: points per lane x workgroup size x LDS staging (61440 bytes hold the padded 27x41 image, 4096 do not)
    x raw-buffer / flat addressing x float32 mirror (fp64) or wide accumulation (fp32); B.info says which form ran"""
    dtype = getattr(hip, dtype_name)
    key, on, off = ("dt_f32", -1, 0) if dtype == hip.EA_F64 else ("wide_accumulate", 1, 0)
    c = _case(hip, shape, kind, dtype_name)
    B = hip.Batch([c.P])
    try:
        for li, loss in enumerate(bb.LOSSES):
            pose = bb.POSES[li]
            c.P.set_loss(*loss)
            c.raw(pose)
            seen = {}
            for ppt, nt in itertools.product((1, 2, 4), (256, 1024)):
                B.set_tuning("points_per_thread", ppt); B.set_tuning("threads", nt)
                # (an fp64 lane takes at most two points, and one in a 1024-lane workgroup: its register budget)
                run = ppt if dtype == hip.EA_F32 else 1 if nt == 1024 else min(ppt, 2)
                for lds_bytes in (61440, 4096):
                    B.set_tuning("use_lds", 1); B.set_tuning("lds_bytes", lds_bytes)
                    g = B.eval(*pose)
                    where = (li, ppt, nt, "lds", lds_bytes)
                    assert B.info("lds_bytes") == lds_bytes and B.info("points_per_thread") == run and B.info("threads") == nt, where
                    c.check_sums(g, pose, loss, where, seen)
                B.set_tuning("use_lds", 0); B.set_tuning("lds_bytes", -1)
                for buf, extra in itertools.product((1, 0), (1, 0)):
                    B.set_tuning("buffer_loads", buf); B.set_tuning(key, on if extra else off)
                    g = B.eval(*pose)
                    where = (li, ppt, nt, "buf", buf, key, extra)
                    assert B.info("buffer_loads") == buf and B.info("lds_bytes") == 0 and B.info(key) == extra, where
                    assert B.info("points_per_thread") == run and B.info("threads") == nt, where
                    c.check_sums(g, pose, loss, where, seen)
                B.set_tuning("buffer_loads", -1); B.set_tuning(key, -1 if dtype == hip.EA_F64 else 0)
            c.report(seen, pose, loss, "fused l%d" % loss[0])
    finally:
        B.close(); c.close()


# ---- c. pose-batched kernels, d. cost-only kernel ---------------------------------------------------------------------------

def _band_of_every_pose(c):
    for p in POSES65:
        c.raw(p)   # (asserts the band share of this pose)


@pytest.mark.parametrize("shape,kind", CASES, ids=_ids(CASES))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_lanes_are_points_pose_kernel_and_cost_kernel(hip, dtype_name, shape, kind):
    """eval_poses with "poses_lane_per_pose" 0 at 65 poses, each against its own reference sums; both reductions
    ("poses_wave_exchange", fp64); the resident poses give the same bits; cost_poses through the cost kernel and through
    its fall-back to the full evaluation"""
    dtype = getattr(hip, dtype_name)
    loss = bb.LOSSES[1]
    c = _case(hip, shape, kind, dtype_name)
    c.P.set_loss(*loss)
    B = hip.Batch([c.P])
    try:
        _band_of_every_pose(c)
        seen = {}
        B.set_tuning("poses_lane_per_pose", 0)
        for exchange in ((1, 0) if dtype == hip.EA_F64 else (0,)):
            if dtype == hip.EA_F64:
                B.set_tuning("poses_wave_exchange", exchange)
            got = B.eval_poses(Q65, T65)
            assert B.info("poses_lane_per_pose") == 0 and B.info("poses_wave_exchange") == exchange, exchange
            _check_poses(c, got, loss, ("eval_poses", exchange), seen)
            again = B.eval_resident_poses()
            assert all(np.array_equal(again[f], got[f]) for f in FIELDS), exchange
        if dtype == hip.EA_F64:
            B.set_tuning("poses_wave_exchange", -1)
        for form in (1, 0):
            B.set_tuning("cost_form", form)
            cost = B.cost_poses(Q65, T65)
            assert B.info("cost_form") == form
            worst = _check_costs(c, cost, loss, ("cost_poses", form))
            print("BAND-GPU %-24s cost_form %d: worst cost deviation %.2f of its bound" % (c.name(), form, worst))
        c.report(seen, POSES65[1], loss, "poses key 0")
    finally:
        B.close(); c.close()


@pytest.mark.parametrize("loss", bb.LOSSES, ids=("trivial", "cauchy", "huber"))
@pytest.mark.parametrize("shape,kind", CASES, ids=_ids(CASES))
def test_pose_per_lane_kernel(hip, shape, kind, loss):
    """fp64, "poses_lane_per_pose" 1 at 65 poses (one full group of lanes and one lane of a second): float32 mirror x
    addressing, each pose against its own reference; Cauchy's cost is the logarithm of the running product of a sub-run"""
    c = _case(hip, shape, kind, "EA_F64")
    c.P.set_loss(*loss)
    B = hip.Batch([c.P])
    try:
        _band_of_every_pose(c)
        seen = {}
        B.set_tuning("poses_lane_per_pose", 1)
        for mirror, buf in itertools.product((1, 0), (1, 0)):
            B.set_tuning("dt_f32", mirror); B.set_tuning("buffer_loads", buf)
            got = B.eval_poses(Q65, T65)
            where = ("lanes", mirror, buf)
            assert B.info("poses_lane_per_pose") == 1 and B.info("dt_f32") == mirror and B.info("buffer_loads") == buf, where
            _check_poses(c, got, loss, where, seen)
            again = B.eval_resident_poses()
            assert all(np.array_equal(again[f], got[f]) for f in FIELDS), where
        c.report(seen, POSES65[1], loss, "poses key 1 l%d" % loss[0])
    finally:
        B.close(); c.close()


# ---- e. riding fold and fused iteration, f. starts kernel -------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", DTYPES)
def test_riding_fold_and_fused_iteration(hip, dtype_name):
    loss, pose = bb.LOSSES[1], bb.POSES[1]
    c = _case(hip, (160, 120), "noise", dtype_name)
    c.P.set_loss(*loss)
    c.raw(pose); c.raw(bb.POSES[0])
    B = hip.Batch([c.P])
    try:
        seen = {}
        c.check_sums(B.eval(*pose), pose, loss, "eval", seen)
        B.bench_capture_pipelined(3)
        B.bench_steps(3)
        c.check_sums(B.bench_result(), pose, loss, "pipelined", seen)
        c.report(seen, pose, loss, "riding fold")
        out = []
        for fused in (1, 0):
            B.set_tuning("fused_iterations", -1 if fused else 0)
            q, t, s = B.solve(bb.Q_ID, bb.T_ID, max_num_iterations=4)
            out.append((q, t, s[0], B.info("fused_iterations")))
        (qa, ta, sa, fa), (qb, tb, sb, fb) = out
        assert fa == 1 and fb == 0
        assert np.array_equal(qa, qb) and np.array_equal(ta, tb)
        for k in ("termination", "why", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost"):
            assert sa[k] == sb[k], (k, sa[k], sb[k])
        for k in TRACE:
            assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), k
        es, tol = c.sums(bb.POSES[0], loss), c.tol(bb.POSES[0], loss)
        d_cost = bb.dev_rel(sa["initial_cost"], es["cost"])
        # Ceres' gradient_max_norm is || x - Plus(x, -g) ||_inf in the ambient space, g = Jtr.  Plus is 1-Lipschitz in g
        # (a point on the unit sphere times q, a subtraction for t), so an error of g within the bound on the sums,
        # which is relative to max |Jtr|, moves the norm by no more than that bound times max |Jtr|.
        g = es["Jtr"].astype(np.float64)
        want = max(np.abs(bb.Q_ID - synth.quat_plus(bb.Q_ID, -g[:3])).max(), np.abs(g[3:]).max())
        d_grad = abs(sa["it_gradient_max_norm"][0] - want) / np.abs(g).max()
        print("BAND-GPU %-24s solve start: cost %.1e gradient %.1e | bound %.1e" % (c.name(), d_cost, d_grad, tol["sums"]))
        assert d_cost <= tol["sums"] and d_grad <= tol["sums"], (d_cost, d_grad, tol["sums"])
    finally:
        B.close(); c.close()


def _same_solve(a, b):
    (qa, ta, sa), (qb, tb, sb) = a, b
    return (np.array_equal(qa, qb) and np.array_equal(ta, tb) and sa["num_iterations"] == sb["num_iterations"] and sa["why"] == sb["why"]
            and all(np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])) for k in TRACE))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_starts_kernel(hip, dtype_name):
    """solve_starts from three of the poses: a start's first cost is the bits eval_poses gives at that pose (the same
    kernel below the one-pose-per-lane threshold), the same start alone (K = 1) gives the same pose and trace bit for bit,
    and ea_batch_solve from that start, which cuts its partial rows differently, begins at the reference's cost"""
    loss = bb.LOSSES[1]
    c = _case(hip, (160, 120), "noise", dtype_name)
    c.P.set_loss(*loss)
    B = hip.Batch([c.P])
    try:
        pick = (0, 1, 3)   # unit quaternions
        q0, t0 = Q65[list(pick)], T65[list(pick)]
        at = B.eval_poses(q0, t0)
        assert B.info("poses_lane_per_pose") == 0
        q, t, s, best = B.solve_starts(q0, t0, max_num_iterations=4)
        assert B.info("starts_form") == 1
        for k, p in enumerate(pick):
            assert s[k][0]["it_cost"][0] == at["cost"][k, 0] == s[k][0]["initial_cost"], k
            c.check_sums({f: at[f][k] for f in FIELDS}, POSES65[p], loss, ("starts eval_poses", k))
            q1, t1, s1, _ = B.solve_starts(q0[k:k + 1], t0[k:k + 1], max_num_iterations=4)
            assert _same_solve((q1[0, 0], t1[0, 0], s1[0][0]), (q[k, 0], t[k, 0], s[k][0])), k
            _, _, sb = B.solve(q0[k, 0], t0[k, 0], max_num_iterations=4)
            d = bb.dev_rel(sb[0]["initial_cost"], c.sums(POSES65[p], loss)["cost"])
            assert d <= c.tol(POSES65[p], loss)["sums"], (k, d)
    finally:
        B.close(); c.close()


# ---- g. variant and weighted kernels ------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", DTYPES)
@pytest.mark.parametrize("name,variant", [("Ex", dict(distortion=DIST)), ("SecondCam", dict(T12=T12)),
                                          ("SecondCamEx", dict(distortion=DIST, T12=T12))])
def test_variant_functors(hip, name, variant, dtype_name):
    c = _case(hip, (27, 41), "noise", dtype_name, variant=variant, vname=name)
    B = hip.Batch([c.P])
    try:
        for pi, pose in ((1, bb.POSES[1]), (2, bb.POSES[2])):
            loss = bb.LOSSES[(pi + 1) % 3]
            c.P.set_loss(*loss)
            c.raw(pose)
            seen = {}
            r, J = c.P.eval_points(*pose, corrected=False)
            c.check_rows(r, J, pose, loss, False, (name, "eval_points", pi), seen)
            for layout in (0, 1):
                rr, JJ, bad = B.eval_rows(*pose, corrected=True, layout=layout)
                assert bad == 0
                c.check_rows(rr, JJ if layout == 0 else JJ.T, pose, loss, True, (name, "eval_rows", pi, layout), seen)
            for ppt, nt in ((1, 256), (4, 1024)):
                B.set_tuning("points_per_thread", ppt); B.set_tuning("threads", nt)
                c.check_sums(B.eval(*pose), pose, loss, (name, "eval", pi, ppt, nt), seen)
            c.report(seen, pose, loss, name + " p%d" % pi)
    finally:
        B.close(); c.close()


def _weighted(hip, c, loss, tag):
    """the weighted kernels on case c: Batch.eval at one and two points per lane and both addressings, corrected rows, and
    the pose-batched kernel over the three poses"""
    B = hip.Batch([c.P])
    try:
        seen = {}
        for pi, pose in enumerate(bb.POSES):
            c.raw(pose)
            for ppt, buf in ((1, 1), (2, 1), (2, 0)):
                B.set_tuning("points_per_thread", ppt); B.set_tuning("buffer_loads", buf)
                g = B.eval(*pose)
                where = (tag, "eval", pi, ppt, buf)
                assert B.info("weighted") == 1 and B.info("points_per_thread") == ppt and B.info("buffer_loads") == buf, where
                c.check_sums(g, pose, loss, where, seen)
            B.set_tuning("points_per_thread", -1); B.set_tuning("buffer_loads", -1)
            rr, JJ, bad = B.eval_rows(*pose, corrected=True)
            assert bad == 0
            c.check_rows(rr, JJ, pose, loss, True, (tag, "eval_rows", pi), seen)
        q = np.stack([p[0] for p in bb.POSES]).reshape(-1, 1, 4)
        t = np.stack([p[1] for p in bb.POSES]).reshape(-1, 1, 3)
        got = B.eval_poses(q, t)
        for k, p in enumerate(bb.POSES):
            c.check_sums({f: got[f][k] for f in FIELDS}, p, loss, (tag, "eval_poses", k), seen)
        c.report(seen, bb.POSES[1], loss, tag)
    finally:
        B.close()


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_weighted_kernels(hip, dtype_name):
    import weights_ref as wr
    loss = bb.LOSSES[1]
    c = _case(hip, (27, 41), "noise", dtype_name, weights=(wr.real_weights(N, 67), "real67"))
    try:
        c.P.set_loss(*loss)
        _weighted(hip, c, loss, "weighted")
    finally:
        c.close()


# ---- h. integer-pixel cost, i. quantile key pass ----------------------------------------------------------------------------

@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_integer_pixel_cost(hip, dtype_name, shape):
    c = _case(hip, shape, "noise", dtype_name)
    try:
        for pose in list(bb.POSES) + [bb.POSE_FAR]:
            got = c.P.pixel_cost(*pose)
            want = en.pixel_cost(c.xyz, pose[0], pose[1], *c.pr["K"], c.pr["image"])
            where = (c.name(), tuple(pose[1]))
            assert got["count"] == want["count"] and got["outside"] == want["outside"], where + (got, want)
            assert got["count"] + got["outside"] == N
            assert got["total_cost"] == pytest.approx(want["total_cost"], rel=1e-12), where
            assert got["max_cost"] == want["max_cost"] and got["max_pixel"] == want["max_pixel"], where
        at_id = en.pixel_cost(c.xyz, bb.Q_ID, bb.T_ID, *c.pr["K"], c.pr["image"])
        assert at_id["outside"] > N // 10 and at_id["count"] > 0, (c.name(), at_id)
    finally:
        c.close()


PROBS = (0.0, 0.25, 0.5, 1.0)


def _check_quantiles(c, where):
    """Problem.residual_quantiles against the same order statistics of the reference's |r| (tests/test_gpu_quantiles.py:
    rank floor(prob (m - 1)), one IEEE multiplication; two vectors' k-th order statistics differ by at most their largest
    per-element difference, so the bound is the one on r)"""
    for pi, pose in enumerate(bb.POSES):
        absr = np.sort(np.abs(c.raw(pose)["r"]))
        want = np.array([absr[int(np.floor(np.float64(p) * np.float64(N - 1)))] for p in PROBS])
        v, m = c.P.residual_quantiles(*pose, PROBS)
        d, bound = bb.dev_r(v, want), c.tol(pose, bb.LOSSES[0])["r"]
        print("BAND-GPU %-24s quantiles p%d: device %.1e | bound %.1e" % (c.name(), pi, d, bound))
        assert m == N and d <= bound, (c.name(), where, pi, d, bound)


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_quantile_key_pass(hip, dtype_name, shape):
    c = _case(hip, shape, "noise", dtype_name)
    try:
        c.P.set_loss(*bb.LOSSES[1])   # (the quantiles are those of the raw residuals whatever the loss)
        _check_quantiles(c, "plain")
    finally:
        c.close()


# ---- j. the ROS flavour -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,kind", TWO, ids=_ids(TWO))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_ros_flavour_rows_sums_costs_and_quantiles(hip, dtype_name, shape, kind):
    """z_guard = 0, z_eps = 0.001, R(q)^T: per-point kernel, rows, fused sums, the cost-only kernel at 65 poses and the
    quantile key pass against the reference with rot_transposed=True"""
    c = _case(hip, shape, kind, dtype_name, flavour=ROS)
    B = hip.Batch([c.P])
    try:
        for pi, pose in enumerate(bb.POSES):
            loss = bb.LOSSES[pi]
            c.P.set_loss(*loss)
            c.raw(pose)
            seen = {}
            for corrected in (False, True):
                r, J = c.P.eval_points(*pose, corrected=corrected)
                c.check_rows(r, J, pose, loss, corrected, ("ros eval_points", pi, corrected), seen)
                for layout in (0, 1):
                    rr, JJ, bad = B.eval_rows(*pose, corrected=corrected, layout=layout)
                    assert bad == 0
                    c.check_rows(rr, JJ if layout == 0 else JJ.T, pose, loss, corrected, ("ros eval_rows", pi, corrected, layout), seen)
            c.check_sums(B.eval(*pose), pose, loss, ("ros eval", pi), seen)
            c.report(seen, pose, loss, "ros rows p%d l%d" % (pi, loss[0]))
        loss = bb.LOSSES[1]
        c.P.set_loss(*loss)
        _band_of_every_pose(c)
        cost = B.cost_poses(Q65, T65)
        assert B.info("cost_form") == 1
        _check_costs(c, cost, loss, ("ros cost_poses",))
        _check_quantiles(c, "ros")
    finally:
        B.close(); c.close()


@pytest.mark.parametrize("shape,kind", TWO, ids=_ids(TWO))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_ros_flavour_pose_batched_kernels(hip, dtype_name, shape, kind):
    """eval_poses at 65 poses with key 0 and (fp64) key 1, where every lane takes the general form of the row"""
    dtype = getattr(hip, dtype_name)
    loss = bb.LOSSES[1]
    c = _case(hip, shape, kind, dtype_name, flavour=ROS)
    c.P.set_loss(*loss)
    B = hip.Batch([c.P])
    try:
        _band_of_every_pose(c)
        for lanes in ((0, 1) if dtype == hip.EA_F64 else (0,)):
            seen = {}
            B.set_tuning("poses_lane_per_pose", lanes)
            got = B.eval_poses(Q65, T65)
            assert B.info("poses_lane_per_pose") == lanes
            _check_poses(c, got, loss, ("ros eval_poses", lanes), seen)
            again = B.eval_resident_poses()
            assert all(np.array_equal(again[f], got[f]) for f in FIELDS), lanes
            c.report(seen, POSES65[1], loss, "ros poses key %d" % lanes)
    finally:
        B.close(); c.close()


@pytest.mark.parametrize("shape,kind", TWO, ids=_ids(TWO))
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_ros_flavour_weighted_kernels(hip, dtype_name, shape, kind):
    import weights_ref as wr
    loss = bb.LOSSES[1]
    c = _case(hip, shape, kind, dtype_name, flavour=ROS, weights=(wr.real_weights(N, 67), "real67"))
    try:
        c.P.set_loss(*loss)
        _weighted(hip, c, loss, "ros weighted")
    finally:
        c.close()


# ---- k. solves end to end -----------------------------------------------------------------------------------------------------

PLANTED_Q, PLANTED_T = synth.quat_from_axis_angle([1, 2, 3], 0.01), (0.004, -0.002, 0.006)


def solvable_problem():
    """80 x 60 edge image with camera_C(60, 80), 1025 points planted on its edges (two rows of the pose kernels and a point)"""
    return bb._cached(("solvable", 60, 80), lambda: synth.make_problem(60, 80, 1025, 12, 3, *bb.camera_C(60, 80), planted_q=PLANTED_Q,
                                                                       planted_t=PLANTED_T, normalize=True))


def _follows_the_oracle(got, want, where):
    """the assertions of tests/test_gpu_lm_random.py between a device solve and the oracle's from the same start"""
    from test_gpu_lm_random import COST_RTOL, LIVE_COST, POSE_BAR
    (q, t, s), (qo, to, so) = got, want
    assert s["why"] == so["why"] and s["num_iterations"] == so["num_iterations"], where
    assert list(s["it_successful"]) == list(so["it_successful"]), where
    live = so["it_cost"] > LIVE_COST * so["initial_cost"]
    assert np.allclose(np.asarray(s["it_cost"])[live], so["it_cost"][live], rtol=COST_RTOL, atol=0), where
    if live.all():
        assert synth.rotation_angle_between(q, qo) < POSE_BAR and np.linalg.norm(t - to) < POSE_BAR, where


def test_fp64_solves_follow_the_oracle_at_camera_C(hip, oracle):
    pr = solvable_problem()
    loss = (hip.LOSS_CAUCHY, 0.7)
    O = oracle.OracleProblem(pr["grid"], *pr["K"], loss=loss[0], loss_a=loss[1])
    q0 = np.stack([bb.Q_ID, synth.quat_from_axis_angle([0.3, -1.0, 0.2], 0.006), synth.quat_from_axis_angle([1.0, 0.5, -2.0], 0.012)])
    t0 = np.array([[0.0, 0.0, 0.0], [0.002, 0.001, -0.003], [-0.004, 0.003, 0.002]])
    want = [O.solve(pr["xyz"], q0[k], t0[k]) for k in range(3)]
    assert want[0][2]["termination"] == 0 and want[0][2]["num_iterations"] >= 3   # a solve, not a start at the answer
    assert synth.rotation_angle_between(want[0][0], pr["q_true"]) < 1e-6 and np.linalg.norm(want[0][1] - pr["t_true"]) < 1e-6
    P = hip.Problem(*pr["K"], dtype=hip.EA_F64)
    B = None
    try:
        P.set_points(pr["xyz"]); P.set_dt_grid(pr["grid"]); P.set_loss(*loss)
        _follows_the_oracle(P.solve(q0[0], t0[0]), want[0], "Problem.solve")
        B = hip.Batch([P])
        for k in range(3):
            q, t, s = B.solve(q0[k], t0[k])
            _follows_the_oracle((q[0], t[0], s[0]), want[k], ("Batch.solve", k))
        q, t, s, best = B.solve_starts(q0[:, None, :], t0[:, None, :])
        assert B.info("starts_form") == 1
        for k in range(3):
            _follows_the_oracle((q[k, 0], t[k, 0], s[k][0]), want[k], ("solve_starts", k))
    finally:
        if B is not None:
            B.close()
        P.close()


def test_fp32_solves_recover_the_planted_pose_at_camera_C(hip):
    from test_gpu_fp32_pose import ANGLE_BAR, DIST_BAR
    pr = solvable_problem()
    P = hip.Problem(*pr["K"], dtype=hip.EA_F32)
    B = None
    try:
        P.set_points(pr["xyz"]); P.set_dt_grid(pr["grid"]); P.set_loss(hip.LOSS_CAUCHY, 0.7)
        q, t, s = P.solve(bb.Q_ID, bb.T_ID)
        B = hip.Batch([P])
        qb, tb, sb = B.solve(bb.Q_ID, bb.T_ID)
        qs, ts, ss, best = B.solve_starts(np.stack([bb.Q_ID, bb.Q_SMALL]).reshape(2, 1, 4), np.stack([bb.T_ID, bb.T_SMALL]).reshape(2, 1, 3))
        for name, (qq, tt, sm) in (("Problem.solve", (q, t, s)), ("Batch.solve", (qb[0], tb[0], sb[0])),
                                   ("solve_starts 0", (qs[0, 0], ts[0, 0], ss[0][0])), ("solve_starts 1", (qs[1, 0], ts[1, 0], ss[1][0]))):
            ang, dist = synth.rotation_angle_between(qq, pr["q_true"]), float(np.linalg.norm(tt - pr["t_true"]))
            print("fp32 %s: %d iterations, %.1e rad, %.1e m from the planted pose" % (name, sm["num_iterations"], ang, dist))
            assert sm["termination"] == hip.CONVERGENCE, name
            assert ang < ANGLE_BAR and dist < DIST_BAR, (name, ang, dist)
    finally:
        if B is not None:
            B.close()
        P.close()
