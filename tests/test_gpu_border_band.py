"""Every kernel that samples the distance transform, on clouds whose 4x4 stencils touch the image border, against the
extended-precision restatement of tests/border_band.py (numpy.longdouble, each tap clamped on its own): the fused sums
in every launch shape / addressing form / image form, the per-point kernel, the materialised rows, the pose-batched
kernel, the variant functors (the reference is extended by the same distortion and rig maps, not the oracle's Jet
rows), the weighted kernels (per-point weights: the reference's rows times sqrt(w_i rho')), the riding fold, one
fused-iteration solve against its pair form, and the integer-pixel cost report.  Images are
tall, wide, square, smaller than the stencil, and of widths either side of the upload's 32-texel tiles and of every
residue mod 4 (border_band.SHAPES); texels are noise (every tap matters) or distance-like.

The reference is fed the points the device holds (Problem.get_points), so fp32 storage rounding is not counted as
kernel error.  Every case asserts its own workload: >= half of the points have a tap outside the image, n_invalid == 0,
no NaN row, and ALL rows are compared (no "noise row" exemption: |d(u, v)/d pose| stays of order fx).

Tolerances (border_band.tolerances): the larger of the project's bound -- fp64 rows 1e-12 (absolute on r, of the largest
entry on J), fp64 sums 1e-11; fp32 rows 2e-5 / 2e-4, sums 1e-4; variant functors J 1e-11 and 5e-5 / 5e-4 as in
test_gpu_rows.py -- and 4x the deviation of the SAME formulas in plain numpy arithmetic of the kernel's precision from
the reference, measured on the CPU.  fp32 is compared per point, not only on sums.  A wrong border texel of a noise image
is an error of 0.1 - 1 in r.

Per case (1000 points, test_per_point_kernel_and_rows_on_every_shape: per-point kernel and rows kernel): the largest
deviation of plain arithmetic of the kernel's precision from the reference over the three poses (CPU), the bounds used
(smallest .. largest over the poses; each pose has its own), and the largest deviation of the device on an MI355X.
profiles/LOG.md ("Border band") has the sums and the other kernels; every test prints its figures as BAND-GPU lines.

  case          | fp64 r: plain   bound    device  | fp32 r: plain   bound              device  | fp32 J: plain   bound              device
  5x3 noise     |         4.8e-16 1.0e-12  4.2e-16 |         3.0e-07 2.0e-05            2.9e-07 |         9.6e-07 2.0e-04            1.2e-06
  27x41 noise   |         6.7e-15 1.0e-12  7.8e-15 |         4.7e-06 2.0e-05            3.5e-06 |         8.3e-06 2.0e-04            7.5e-06
  160x120 noise |         3.9e-14 1.0e-12  3.1e-14 |         1.7e-05 2.0e-05 .. 6.9e-05 1.3e-05 |         4.3e-05 2.0e-04            4.2e-05
  33x257 noise  |         3.6e-14 1.0e-12  4.7e-14 |         1.4e-05 3.2e-05 .. 5.6e-05 2.2e-05 |         5.5e-05 2.0e-04 .. 2.2e-04 3.9e-05
  480x640 noise |         1.3e-13 1.0e-12  9.3e-14 |         5.0e-05 1.8e-04 .. 2.0e-04 5.3e-05 |         1.7e-04 3.4e-04 .. 6.7e-04 1.6e-04
  480x640 dt    |         7.5e-16 1.0e-12  6.7e-16 |         2.8e-07 2.0e-05            3.0e-07 |         1.1e-04 2.0e-04 .. 4.4e-04 7.8e-05

(fp64 J, relative: plain <= 3.1e-13, bound 1.0e-12 .. 1.3e-12, device <= 2.8e-13, all at 480x640.)  On these images the
device stays within 2.5 times the plain-arithmetic deviation; the 4x rule decides only in fp32 from 160 pixels up."""
import itertools

import numpy as np
import pytest

import border_band as bb
from oracle import ea_numpy as en

pytestmark = pytest.mark.gpu
N = bb.N_GPU
DIST = (0.01, -0.002, 0.0005, -0.0003, 0.001)   # weak enough that the band stays the band
T12 = np.eye(4)
T12[:3, :3] = en.quat_to_R(bb.quat_from_axis_angle([0.1, 1.0, 0.2], 0.001))
T12[:3, 3] = [0.0006, 0.0002, -0.0005]
DTYPES = ("EA_F64", "EA_F32")
NOISE_CORE = [(s, "noise") for s in bb.CORE_SHAPES]
# all shapes with noise texels, the core shapes also with distance-like texels
ALL_CASES = [(s, "noise") for s in bb.SHAPES] + [(s, "dt") for s in bb.CORE_SHAPES]


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_per_point_kernel_and_rows_on_every_shape(hip, dtype_name):
    """eval_points and Batch.eval_rows (both layouts, corrected and raw, staged and direct stores), row by row, and one
    fused evaluation, on all shapes at the three poses; the loss changes with the pose"""
    for (H, W), kind in ALL_CASES:
        c = bb.make_case(hip, H, W, kind, getattr(hip, dtype_name))
        if c is None:
            continue
        B = hip.Batch([c.P])
        try:
            for pi, pose in enumerate(bb.POSES):
                loss = bb.LOSSES[(pi + bb.SHAPES.index((H, W))) % 3]
                c.P.set_loss(*loss)
                c.raw(pose)   # (asserts the workload)
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
                        if first is None:   # row by row against the reference ...
                            c.check_rows(rr, JJ, pose, loss, corrected, where, seen)
                            first = (rr.copy(), JJ.copy())
                        # ... and layouts and store forms move the same numbers: bit-identical to the rows just compared
                        assert np.array_equal(rr, first[0]) and np.array_equal(JJ, first[1]), where
                c.check_sums(B.eval(*pose), pose, loss, ("eval", pi), seen)
                c.report(seen, pose, loss, "rows p%d l%d" % (pi, loss[0]))
        finally:
            B.close(); c.close()


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_fused_sums_in_every_launch_shape_on_the_band(hip, dtype_name):
    """Batch.eval: points per lane x workgroup size x LDS staging (61440 bytes stage the whole padded image of the small
    shapes -- a tile whose origin is padded texel (0, 0) -- and fall back to L2 on the large ones; 4096 bytes fall back
    on all but 5x3) x raw-buffer / flat addressing x float32 mirror on / off (fp64) x wide accumulation (fp32) x tile point
    order, the three losses each at its own pose"""
    dtype = getattr(hip, dtype_name)
    key, on, off = ("dt_f32", -1, 0) if dtype == hip.EA_F64 else ("wide_accumulate", 1, 0)
    for (H, W), kind in NOISE_CORE + [((160, 120), "dt")]:
        for tile in (0, 16):
            c = bb.make_case(hip, H, W, kind, dtype, tile=tile)
            if c is None:
                continue
            assert c.P.point_order == tile
            B = hip.Batch([c.P])
            try:
                for li, loss in enumerate(bb.LOSSES):
                    pose = bb.POSES[li]
                    c.P.set_loss(*loss)
                    c.raw(pose)
                    seen = {}
                    big = (H, W) == (480, 640)   # the tuning product is trimmed on the large shape, not the border shapes
                    for ppt, nt in itertools.product((1, 2, 4), (256, 1024)):
                        B.set_tuning("points_per_thread", ppt); B.set_tuning("threads", nt)
                        for lds_bytes in ((61440,) if big else (61440, 4096)):
                            B.set_tuning("use_lds", 1); B.set_tuning("lds_bytes", lds_bytes)
                            g = B.eval(*pose)
                            assert B.info("lds_bytes") == lds_bytes
                            c.check_sums(g, pose, loss, (tile, li, ppt, nt, "lds", lds_bytes), seen)
                        B.set_tuning("use_lds", 0); B.set_tuning("lds_bytes", -1)
                        for buf in (1, 0):
                            B.set_tuning("buffer_loads", buf)
                            for extra in ((1,) if big and buf == 0 else (1, 0)):
                                # the float32 mirror of an fp64 image / the fp64 accumulation of an fp32 evaluation
                                B.set_tuning(key, on if extra else off)
                                g = B.eval(*pose)
                                where = (tile, li, ppt, nt, "buf", buf, key, extra)
                                assert B.info("buffer_loads") == buf and B.info("lds_bytes") == 0 and B.info(key) == extra, where
                                c.check_sums(g, pose, loss, where, seen)
                        B.set_tuning("buffer_loads", -1); B.set_tuning(key, -1 if dtype == hip.EA_F64 else 0)
                    if tile == 0:
                        c.report(seen, pose, loss, "fused l%d" % loss[0])
            finally:
                B.close(); c.close()


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_pose_batched_kernel_on_the_band(hip, dtype_name):
    """Batch.eval_poses / the resident poses: the three poses, one a pixel away and one that swings most of the cloud out
    of the frame, in one call, each against the reference; every split over launches lands on the same bits"""
    dtype = getattr(hip, dtype_name)
    poses = list(bb.POSES) + [(bb.Q_SMALL, bb.T_SMALL + [0.0006, 0.0, 0.0]), bb.POSE_FAR]
    loss = bb.LOSSES[1]
    for (H, W), kind in NOISE_CORE + [((33, 257), "dt")]:
        c = bb.make_case(hip, H, W, kind, dtype)
        if c is None:
            continue
        c.P.set_loss(*loss)
        B = hip.Batch([c.P])
        try:
            far = c.raw(bb.POSE_FAR, min_share=0.0)
            out = (far["u"] < 0) | (far["u"] >= W) | (far["v"] < 0) | (far["v"] >= H)
            assert out.mean() > 0.5, (c.name(), float(out.mean()))
            for p in poses[:-1]:
                c.raw(p)   # (asserts the band share)
            q = np.stack([p[0] for p in poses]).reshape(-1, 1, 4)
            t = np.stack([p[1] for p in poses]).reshape(-1, 1, 3)
            seen = {}
            got = B.eval_poses(q, t)
            for k, p in enumerate(poses):
                c.check_sums({f: got[f][k] for f in got}, p, loss, ("eval_poses", k), seen)
            again = B.eval_resident_poses()
            assert all(np.array_equal(again[f], got[f]) for f in ("cost", "JtJ", "Jtr", "n_invalid"))
            for g in (1, 2):
                B.set_tuning("poses_per_launch", g)
                split = B.eval_poses(q, t)
                assert all(np.array_equal(split[f], got[f]) for f in ("cost", "JtJ", "Jtr", "n_invalid")), g
            B.set_tuning("poses_per_launch", 0)
            c.report(seen, poses[1], loss, "poses")
        finally:
            B.close(); c.close()


@pytest.mark.parametrize("name,variant", [("Ex", dict(distortion=DIST)), ("SecondCam", dict(T12=T12)),
                                          ("SecondCamEx", dict(distortion=DIST, T12=T12))])
def test_variant_functors_on_the_band(hip, name, variant):
    """EAResidueEx / EAResidueSecondCam / EAResidueSecondCamEx: per-point kernel, rows and fused sums, both dtypes, against
    the reference extended by the same maps"""
    for dtype_name in DTYPES:
        for (H, W), kind in NOISE_CORE:
            c = bb.make_case(hip, H, W, kind, getattr(hip, dtype_name), variant=variant, vname=name)
            if c is None:
                continue
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


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("cost", "JtJ", "Jtr", "n_invalid"))


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_riding_fold_on_the_band(hip, dtype_name):
    """the pipelined sequence of test_gpu_pipelined.py (fold of step k-1 riding in evaluation k): the result against the
    reference, riding and closing folds bit for bit, launch by launch the same bits, the serial graph = Batch.eval"""
    dtype = getattr(hip, dtype_name)
    loss, pose = bb.LOSSES[1], bb.POSES[1]
    for (H, W), kind in NOISE_CORE:
        c = bb.make_case(hip, H, W, kind, dtype)
        if c is None:
            continue
        c.P.set_loss(*loss)
        c.raw(pose)
        B = hip.Batch([c.P])
        try:
            for ppt, nt in ((1, 256), (2, 1024), (4, 256)):
                B.set_tuning("points_per_thread", ppt); B.set_tuning("threads", nt)
                ref = B.eval(*pose)
                c.check_sums(ref, pose, loss, ("eval", ppt, nt))
                for steps in (1, 3):
                    where = (c.name(), ppt, nt, steps)
                    B.bench_capture_pipelined(steps)
                    B.bench_steps(steps)
                    last = B.bench_result()
                    c.check_sums(last, pose, loss, where)
                    for k in ("cost", "JtJ", "Jtr"):   # the same partial rows summed in another fixed order
                        assert bb.dev_rel(last[k], ref[k]) <= 1e-13, where
                    if steps >= 2:
                        assert _same(B.bench_result(riding=True), last), where
                    B.bench_steps(steps, riding=True)
                    assert _same(B.bench_result(), last), where + ("launch by launch",)
                B.bench_capture(2)
                B.bench_steps(2)
                assert _same(B.bench_result(), ref), (c.name(), ppt, nt, "serial graph")
        finally:
            B.close(); c.close()


TRACE = ("it_cost", "it_cost_change", "it_gradient_max_norm", "it_step_norm", "it_relative_decrease", "it_radius", "it_successful")


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_fused_iteration_solve_started_in_the_band(hip, dtype_name):
    """one launch per LM iteration against the (evaluate, step) pairs, bit for bit, from a start (the identity) at which
    most points have a tap outside the image"""
    dtype = getattr(hip, dtype_name)
    for (H, W), kind in [(s, k) for s in bb.CORE_SHAPES for k in bb.KINDS]:
        c = bb.make_case(hip, H, W, kind, dtype)
        if c is None:
            continue
        c.P.set_loss(*bb.LOSSES[1])
        c.raw(bb.POSES[0])   # (asserts the band share at the start)
        B = hip.Batch([c.P])
        try:
            out = []
            for fused in (1, 0):
                B.set_tuning("fused_iterations", -1 if fused else 0)
                q, t, s = B.solve(bb.Q_ID, bb.T_ID, max_num_iterations=6)
                out.append((q, t, s[0], B.info("fused_iterations")))
            (qa, ta, sa, fa), (qb, tb, sb, fb) = out
            assert fa == 1 and fb == 0, c.name()
            assert np.array_equal(qa, qb) and np.array_equal(ta, tb), c.name()
            for k in ("termination", "why", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost",
                      "final_cost", "num_point_evals"):
                assert sa[k] == sb[k], (c.name(), k, sa[k], sb[k])
            for k in TRACE:
                assert np.array_equal(np.asarray(sa[k]), np.asarray(sb[k])), (c.name(), k)
            # and the start of the trace is the reference's cost at the identity
            es = c.sums(bb.POSES[0], bb.LOSSES[1])
            assert bb.dev_rel(sa["initial_cost"], es["cost"]) <= c.tol(bb.POSES[0], bb.LOSSES[1])["sums"], c.name()
        finally:
            B.close(); c.close()


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_integer_pixel_cost_on_the_band(hip, dtype_name):
    """ea_problem_pixel_cost against oracle/ea_numpy.pixel_cost: the `(int)` truncation of u in (-1, 0) (pixel 0) and at
    W - 1 .. W, on every shape"""
    dtype = getattr(hip, dtype_name)
    for (H, W), kind in [(s, "noise") for s in bb.SHAPES]:
        c = bb.make_case(hip, H, W, kind, dtype)
        if c is None:
            continue
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
            assert at_id["outside"] > N // 10 and at_id["count"] > 0, (c.name(), at_id)   # both sides of the border are populated
        finally:
            c.close()


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_weighted_kernels_on_the_band(hip, dtype_name):
    """per-point weights (the weighted kernels of the variant translation unit, plain functor) on the band: Batch.eval at one
    and two points per lane and both addressing forms, the corrected rows, and the pose-batched kernel over the three poses,
    against the reference's weighted rows (border_band.with_loss(weights=): rows times sqrt(w_i rho'), rho times w_i, with the
    weights the device holds).  Distinct real weights with exact zeros (weights_ref.real_weights)."""
    import weights_ref as wr
    dtype = getattr(hip, dtype_name)
    loss = bb.LOSSES[1]
    for (H, W), kind in NOISE_CORE:
        c = bb.make_case(hip, H, W, kind, dtype, weights=(wr.real_weights(N, 40 + H), "real%d" % (40 + H)))
        if c is None:
            continue
        c.P.set_loss(*loss)
        B = hip.Batch([c.P])
        try:
            seen = {}
            for pi, pose in enumerate(bb.POSES):
                c.raw(pose)   # (asserts the workload)
                for ppt, buf in ((1, 1), (2, 1), (2, 0)):
                    B.set_tuning("points_per_thread", ppt); B.set_tuning("buffer_loads", buf)
                    g = B.eval(*pose)
                    where = ("weighted eval", pi, ppt, buf)
                    assert B.info("weighted") == 1 and B.info("points_per_thread") == ppt and B.info("buffer_loads") == buf, where
                    assert B.info("chunk") == 256 * ppt and B.info("threads") == 256, where
                    c.check_sums(g, pose, loss, where, seen)
                B.set_tuning("points_per_thread", -1); B.set_tuning("buffer_loads", -1)
                rr, JJ, bad = B.eval_rows(*pose, corrected=True)
                assert bad == 0
                c.check_rows(rr, JJ, pose, loss, True, ("weighted eval_rows", pi), seen)
            q = np.stack([p[0] for p in bb.POSES]).reshape(-1, 1, 4)
            t = np.stack([p[1] for p in bb.POSES]).reshape(-1, 1, 3)
            got = B.eval_poses(q, t)
            for k, p in enumerate(bb.POSES):
                c.check_sums({f: got[f][k] for f in got}, p, loss, ("weighted eval_poses", k), seen)
            c.report(seen, bb.POSES[1], loss, "weighted")
        finally:
            B.close(); c.close()
