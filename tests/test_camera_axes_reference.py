"""The extended-precision restatement of tests/border_band.py on an anisotropic, off-centre camera (border_band.camera_C:
fy = 1.37 fx, principal point 3.25 pixels right of and 2.5 pixels above the centre), before tests/test_gpu_camera_axes.py
holds every kernel to it.

(1) Mutation sensitivity.  A reference that reads the camera wrongly -- fx and fy swapped, fy := fx, cx and cy swapped,
the row's y-gradient taken with fx (r unchanged), cx or cy rebuilt from the extent -- must move away from the reference
at the true camera by at least 100 times the bound a kernel is held to (border_band.tolerances, fp64 and fp32): in r or
J, and in the sums.  That is a condition on the workload, not a measurement: with it, no kernel wrong in one of these
ways passes the GPU module.  Smallest ratios seen over all cases (each case prints its own as CAMERA-CPU lines):
fp64 rows 2.7e11, fp64 sums 8.2e9, fp32 rows 1.3e3, fp32 sums 8.2e2 (for the rows the smallest is the row-only mutation,
which moves J by 0.27 of its largest entry and leaves r alone).

(2) The two CPU checkers (oracle/ea_oracle.c, oracle/ea_numpy.py) at that camera, since the solves and producers of the
GPU module are compared with them; ea_numpy.pixel_cost against an integer-pixel loop written here.

(3) The transposed flavour of the restatement (rotation applied transposed, z_eps = 0.001, no z guard: what the ROS node
evaluates) against the C oracle's, and its rows against central differences of its own long-double residuals."""
import math

import numpy as np
import pytest

import border_band as bb
from oracle import ea_numpy as en

N = 1000
SHAPES = ((27, 41), (33, 257), (160, 120))
RATIO = 100.0
ROS = dict(z_guard=0.0, z_eps=0.001, rot_transposed=True)


def _mutations(K, H, W):
    fx, fy, cx, cy = K
    return (("fx<->fy", dict(K=(fy, fx, cx, cy))), ("fy:=fx", dict(K=(fx, fx, cx, cy))), ("cx<->cy", dict(K=(fx, fy, cy, cx))),
            ("row fy:=fx", dict(K=K, grad_K=(fx, fx))), ("cx:=centre", dict(K=(fx, fy, 0.5 * (W - 1), cy))),
            ("cy:=centre", dict(K=(fx, fy, cx, 0.5 * (H - 1)))))


def _cases():
    for H, W in SHAPES:
        for kind in bb.KINDS:
            yield pytest.param(H, W, kind, id="%dx%d-%s" % (H, W, kind))


def test_camera_C_is_anisotropic_off_centre_and_float32():
    for H, W in SHAPES + ((60, 80),):
        fx, fy, cx, cy = K = bb.camera_C(H, W)
        assert all(float(np.float32(k)) == k for k in K)
        assert fy > 1.3 * fx and cx - 0.5 * (W - 1) == 3.25 and cy - 0.5 * (H - 1) == -2.5
        assert len({fx, fy, cx, cy}) == 4


def test_default_clouds_keep_their_bits():
    """camera=None is the cloud the earlier modules see: the division by K[1] is the division by f it replaced"""
    pr = bb.band_problem(27, 41, 60, 7, "noise")
    f = pr["K"][0]
    assert pr["K"] == (f, f, 20.0, 13.0)
    u, v, z = pr["uv"][:, 0], pr["uv"][:, 1], pr["xyz"][:, 2]
    assert np.array_equal(pr["xyz"][:, 0], (u - 20.0) * z / f) and np.array_equal(pr["xyz"][:, 1], (v - 13.0) * z / f)
    c = bb.band_problem(27, 41, 60, 7, "noise", camera="C")
    assert np.array_equal(c["uv"], pr["uv"]) and np.array_equal(c["image"], pr["image"]) and c["K"] == bb.camera_C(27, 41)
    assert np.array_equal(c["xyz"][:, 2], z) and not np.array_equal(c["xyz"][:, :2], pr["xyz"][:, :2])


@pytest.mark.parametrize("H,W,kind", _cases())
def test_a_wrong_camera_axis_moves_the_reference_far_beyond_the_bounds(H, W, kind):
    pr = bb.problem(H, W, kind, n=N, camera="C")
    xyz32 = pr["xyz"].astype(np.float32).astype(np.float64)
    lines = []
    for pi, (q, t) in enumerate(bb.POSES):
        loss = bb.LOSSES[pi]
        worst = {}
        for ty, xyz in ((np.float64, pr["xyz"]), (np.float32, xyz32)):
            raw = bb.functor(pr["image"], pr["K"], xyz, q, t)
            assert raw["valid"].all() and not np.isnan(raw["J"].astype(np.float64)).any()
            share = float(raw["band"].mean())
            assert share >= 0.5, share
            ref = bb.with_loss(raw, *loss)
            tol = bb.tolerances(pr, xyz, q, t, loss, ty, ref_rows=ref)
            es = bb.sums(ref)
            for name, kw in _mutations(pr["K"], H, W):
                bad = bb.with_loss(bb.functor(pr["image"], kw["K"], xyz, q, t, grad_K=kw.get("grad_K")), *loss)
                dr, dJ, ds = bb.dev_r(bad["r"], ref["r"]), bb.dev_J(bad["J"], ref["J"]), bb.dev_sums(bb.sums(bad), es)
                if "grad_K" in kw:
                    assert dr == 0.0   # (only the row is wrong)
                rows, sums = max(dr / tol["r"], dJ / tol["J"]), ds / tol["sums"]
                where = (ty.__name__, pi, name, "r %.1e / %.1e  J %.1e / %.1e  sums %.1e / %.1e" % (dr, tol["r"], dJ, tol["J"], ds, tol["sums"]))
                assert rows >= RATIO, where
                assert sums >= RATIO, where
                k = ty.__name__
                worst[k] = (min(worst.get(k, (np.inf, np.inf))[0], rows), min(worst.get(k, (np.inf, np.inf))[1], sums))
        lines.append("CAMERA-CPU %dx%d %s pose %d share %.2f  smallest ratio to the bound: fp64 rows %.1e sums %.1e | fp32 rows %.1e sums %.1e"
                     % (H, W, kind, pi, share, *worst["float64"], *worst["float32"]))
    print("\n".join(lines))   # (shown with -s or -rP)


@pytest.mark.parametrize("H,W,kind", _cases())
def test_cpu_checkers_at_camera_C(oracle, H, W, kind):
    """ea_numpy.evaluate (unit quaternions) and the C oracle under Cauchy and Huber: sums within the project's fp64 bar"""
    pr = bb.problem(H, W, kind, n=N, camera="C")
    bar = bb.PROJECT[np.float64]["sums"]
    for pi, (q, t) in enumerate(bb.POSES):
        raw = bb.functor(pr["image"], pr["K"], pr["xyz"], q, t, np.float64)
        for loss in bb.LOSSES[1:]:
            es = bb.sums(bb.with_loss(raw, *loss))
            O = oracle.OracleProblem(pr["grid"], *pr["K"], loss=loss[0], loss_a=loss[1])
            for mode in (oracle.JAC_JET, oracle.JAC_ANALYTIC):
                e = O.eval(pr["xyz"], q, t, mode)
                d = bb.dev_sums(e, es)
                assert e["n_invalid"] == 0 and d <= bar, (pi, loss, mode, d)
            if pi < 2:
                g = en.evaluate(pr["grid"], pr["K"], pr["xyz"], q, t, loss_kind=loss[0], loss_a=loss[1])
                d = bb.dev_sums(g, es)
                assert g["n_invalid"] == 0 and d <= bar, (pi, loss, "ea_numpy", d)


def _pixel_cost_loop(xyz, q, t, K, image):
    """cost = image[(int) v][(int) u] of every warped point, one point at a time"""
    fx, fy, cx, cy = K
    w, x, y, z = [float(e) for e in q]
    R = ((1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)),
         (2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)),
         (2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)))
    H, W = image.shape
    costs, outside, best, best_px = [], 0, -1.0, (0.0, 0.0)
    for X in xyz:
        b = [R[k][0] * X[0] + R[k][1] * X[1] + R[k][2] * X[2] + t[k] for k in range(3)]
        u, v = fx * (b[0] / b[2]) + cx, fy * (b[1] / b[2]) + cy
        if not (-1.0 < u < W and -1.0 < v < H):   # (int) truncates (-1, 0) to pixel 0
            outside += 1
            continue
        c = float(image[int(v), int(u)])
        costs.append(c)
        if c > best:
            best, best_px = c, (u, v)
    return dict(total_cost=math.fsum(costs), count=len(costs), outside=outside, max_cost=best, max_pixel=best_px)


@pytest.mark.parametrize("H,W", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_numpy_pixel_cost_at_camera_C(H, W):
    pr = bb.problem(H, W, "noise", n=N, camera="C")
    for q, t in bb.POSES + (bb.POSE_FAR,):
        got = en.pixel_cost(pr["xyz"], q, t, *pr["K"], pr["image"])
        want = _pixel_cost_loop(pr["xyz"], q, t, pr["K"], pr["image"])
        assert got["count"] == want["count"] and got["outside"] == want["outside"] and got["count"] + got["outside"] == N
        assert (got["count"] > 0 and got["outside"] > N // 10) or t is bb.POSE_FAR[1]   # both sides of the border are populated
        assert got["total_cost"] == pytest.approx(want["total_cost"], rel=1e-13)
        assert got["max_cost"] == want["max_cost"] and got["max_pixel"] == pytest.approx(want["max_pixel"], rel=1e-13)
        # and a camera read in the wrong order counts other pixels
        fx, fy, cx, cy = pr["K"]
        for K in ((fy, fx, cx, cy), (fx, fy, cy, cx)):
            other = en.pixel_cost(pr["xyz"], q, t, *K, pr["image"])
            assert (other["count"], other["total_cost"]) != (got["count"], got["total_cost"]) or got["count"] == 0


@pytest.mark.parametrize("H,W,kind", _cases())
def test_transposed_flavour_against_the_c_oracle(oracle, H, W, kind):
    pr = bb.problem(H, W, kind, n=N, camera="C")
    for pi, (q, t) in enumerate(bb.POSES):
        raw = bb.functor(pr["image"], pr["K"], pr["xyz"], q, t, **ROS)
        assert raw["valid"].all() and raw["band"].mean() >= 0.5
        if pi:   # the transposition is not a no-op: the untransposed flavour is somewhere else
            plain = bb.functor(pr["image"], pr["K"], pr["xyz"], q, t, z_guard=0.0, z_eps=0.001)
            assert bb.dev_r(plain["r"], raw["r"]) > 1e-3
        loss = bb.LOSSES[pi]
        ref = bb.with_loss(raw, *loss)
        tol = bb.tolerances(pr, pr["xyz"], q, t, loss, np.float64, ref_rows=ref, **ROS)
        O = oracle.OracleProblem(pr["grid"], *pr["K"], loss=loss[0], loss_a=loss[1], **ROS)
        for mode in (oracle.JAC_JET, oracle.JAC_ANALYTIC):
            e = O.eval(pr["xyz"], q, t, mode, materialize=True)
            assert e["n_invalid"] == 0
            assert bb.dev_r(e["raw_r"], raw["r"]) <= tol["r"] and bb.dev_J(e["raw_J"], raw["J"]) <= tol["J"], (pi, mode)
            assert bb.dev_r(e["r"], ref["r"]) <= tol["r"] and bb.dev_J(e["J"], ref["J"]) <= tol["J"], (pi, mode)
            assert bb.dev_sums(e, bb.sums(ref)) <= tol["sums"], (pi, mode)


def _quat_plus(q, d):
    """Ceres' QuaternionParameterization::Plus in long double: [cos|d|, sin|d| d / |d|] * q"""
    n = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    a = [np.cos(n)] + [np.sin(n) / n * e for e in d]
    w, x, y, z = q
    return np.array([a[0] * w - a[1] * x - a[2] * y - a[3] * z, a[0] * x + a[1] * w + a[2] * z - a[3] * y,
                     a[0] * y - a[1] * z + a[2] * w + a[3] * x, a[0] * z + a[1] * y - a[2] * x + a[3] * w], dtype=np.longdouble)


@pytest.mark.parametrize("H,W", ((27, 41), (160, 120)), ids=("27x41", "160x120"))
def test_transposed_flavour_rows_are_the_derivative_of_its_residuals(H, W):
    """Central differences of the long-double r along quat_plus(q, h e_i) and t + h e_i, step h = 2^-28.

    With s = |d(u, v) / d parameter| <= 2 fy (1 + x^2 + y^2) / z < 2000 pixels per unit on these cases and third
    derivatives of the Catmull-Rom surface through texels in [0, 1] below 12, the truncation h^2 s^3 12 / 6 is below
    2.3e-7 and, typically, a thousandth of that; r carries a few long-double roundings of u (1e-19 x 160 pixels x
    gradient 1) -> 1e-17 / h = 3e-9.  Rows reach several hundred, so the bar is 1e-9 of the largest entry -- a
    transposition missing in one dR/dq_i is an error of order 1.  The surface is C1 only: where u or v is within
    4 h s of an integer the second derivative jumps inside the step, and those points (none or a handful) are left out."""
    pr = bb.problem(H, W, "noise", n=N, camera="C")
    ld = np.longdouble
    h = ld(2.0) ** -28
    for q, t in bb.POSES[1:]:
        q, t = np.asarray(q, dtype=ld), np.asarray(t, dtype=ld)
        raw = bb.functor(pr["image"], pr["K"], pr["xyz"], q, t, **ROS)
        D = np.zeros((N, 6), dtype=ld)
        for i in range(6):
            e = np.zeros(3, dtype=ld)
            e[i % 3] = h
            hi, lo = ((_quat_plus(q, e), t), (_quat_plus(q, -e), t)) if i < 3 else ((q, t + e), (q, t - e))
            D[:, i] = (bb.functor(pr["image"], pr["K"], pr["xyz"], *hi, **ROS)["r"] - bb.functor(pr["image"], pr["K"], pr["xyz"], *lo, **ROS)["r"]) / (2 * h)
        margin = float(4 * h * 2000)
        smooth = np.ones(N, bool)
        for c in (raw["u"], raw["v"]):
            c = c.astype(np.float64)
            smooth &= np.abs(c - np.round(c)) > margin
        assert smooth.sum() >= N - 10
        top = float(np.abs(raw["J"]).max())
        assert top > 50.0
        d = float(np.abs(D[smooth] - raw["J"][smooth]).max()) / top
        print("CAMERA-CPU %dx%d transposed rows against central differences: %.1e of the largest entry (%d points)" % (H, W, d, smooth.sum()))
        assert d <= 1e-9, d
