"""Border-band workloads and an extended-precision restatement of the residual functor (test helper, not a fixture).

The evaluation kernels never clamp a stencil tap: they read a copy of the image with three replicated texels on every
side and saturate the texel index.  Ceres' Grid2D + BiCubicInterpolator clamps each of the 16 taps on its own.  The two
agree only if padded copy, saturation, pitch and byte offsets are all right, and they can only disagree where a 4x4
stencil touches the border.  `band_problem` puts most of a point cloud there; `functor` is what the kernels are held to.

`functor` is written from the mathematics (EAResidue of the reference's standalone/utils.h, Ceres' cubic interpolation,
QuaternionParameterization and loss functions): warp, z + z_eps, projection, Catmull-Rom weights, every tap index
clamped by itself as Grid2D::GetValue does, the 1x6 row through dR/dq and the plus-Jacobian (valid for any |q|), the
three losses with Ceres' corrector.  No padded image, no saturated index, nothing shared with oracle/ or the kernels.
One function, the arithmetic type is a parameter: numpy.longdouble (64-bit mantissa on x86; the import fails where it
is no wider than float64 -- there is no mpmath path) is the reference,
numpy.float64 / numpy.float32 runs of the same formulas measure what plain arithmetic of the kernels' own precision loses
(`tolerances`)."""
import numpy as np

LOSS_TRIVIAL, LOSS_CAUCHY, LOSS_HUBER = 0, 1, 2
LOSSES = ((LOSS_TRIVIAL, 1.0), (LOSS_CAUCHY, 1.0), (LOSS_HUBER, 0.3))

# (H, W).  Smaller than the stencil; one pixel high / wide strips; W + 6 and H + 6 either side of the 32-texel tiles of
# the transposing upload (26, 27, 58, 59); every residue of W mod 4 (the pitch is W + 6 rounded up to 4 texels); tall,
# wide and square; one full frame.
SMALL_SHAPES = ((1, 1), (2, 5), (5, 3))
SHAPES = SMALL_SHAPES + ((3, 300), (7, 64), (160, 120), (33, 257), (480, 640),
                         (40, 26), (40, 27), (40, 58), (40, 59), (26, 40), (27, 41), (58, 42), (59, 43))
KINDS = ("noise", "dt")
# the shapes every kernel entry is run on (the rest are run through the per-point kernel and one fused evaluation)
CORE_SHAPES = ((5, 3), (160, 120), (33, 257), (27, 41), (480, 640))

assert np.finfo(np.longdouble).nmant > np.finfo(np.float64).nmant, \
    "numpy.longdouble is not wider than float64 on this machine: the extended-precision reference has nothing to stand on"


def quat_from_axis_angle(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    return np.concatenate([[np.cos(0.5 * angle)], np.sin(0.5 * angle) * a])


Q_ID, T_ID = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)
# (small: at fx = 704 and depth 0.5 it moves a point by up to ~2.5 pixels, so that the 7-pixel bands stay border bands)
Q_SMALL, T_SMALL = quat_from_axis_angle([1.0, -2.0, 0.5], np.deg2rad(0.12)), np.array([0.0008, -0.0006, 0.002])
Q_NONUNIT = quat_from_axis_angle([-0.3, 1.0, 2.0], np.deg2rad(0.2)) * 1.003   # the general Jacobian path
# identity, a small unit rotation + translation, a non-unit quaternion
POSES = ((Q_ID, T_ID), (Q_SMALL, T_SMALL), (Q_NONUNIT, np.array([-0.001, 0.002, -0.003])))
# swings most of the cloud out of the frame (every tap the same border texel for those points)
POSE_FAR = (quat_from_axis_angle([0.1, 1.0, 0.0], np.deg2rad(12.0)), np.array([0.6, -0.4, 0.1]))


def camera_C(H, W):
    """An anisotropic, off-centre camera for an H x W image: fy = 1.37 fx, the principal point 3.25 pixels right of and
    2.5 pixels above the centre.  Every intrinsic is float32-representable.  With fx != fy and cx - (W-1)/2 != cy - (H-1)/2
    != 0, reading one axis' intrinsic for the other, or rebuilding the principal point from the extent, moves u or v by
    pixels (tests/test_camera_axes_reference.py)."""
    f = np.float32(1.1 * max(H, W))
    return (float(f), float(np.float32(1.37 * f)), float(np.float32(0.5 * (W - 1) + 3.25)), float(np.float32(0.5 * (H - 1) - 2.5)))


def band_problem(H, W, n, seed, kind, camera=None):
    """-> dict(image (H, W) float64 holding float32 values, grid (W, H) the Grid2D view of it, K (fx, fy, cx, cy),
    xyz (n, 3), uv (n, 2) the target pixels).  Texels and intrinsics are float32-representable, so fp32 problems, fp64
    problems and the float32 mirror of an fp64 image hold the same numbers.  camera: None -- fx = fy, the principal
    point at the image centre; "C" -- camera_C(H, W), the same target pixels reached through that camera."""
    rng = np.random.default_rng(seed)
    if kind == "noise":      # every one of the 16 taps matters
        img = rng.random((H, W))
    elif kind == "dt":       # smooth, non-negative, distance-like: what the producers make
        vv, uu = np.mgrid[0:H, 0:W].astype(np.float64)
        sites = rng.random((6, 2)) * [W, H]
        img = np.min([np.hypot(uu - s[0], vv - s[1]) for s in sites], axis=0)
        img = img / max(img.max(), 1.0)
    else:
        raise ValueError(kind)
    img = img.astype(np.float32).astype(np.float64)
    m = n // 6
    u = rng.uniform(-6.0, W + 5.0, n)
    v = rng.uniform(-6.0, H + 5.0, n)
    u[0 * m:1 * m] = rng.uniform(-4.0, 3.0, m)                 # left band
    u[1 * m:2 * m] = W - 1 + rng.uniform(-3.0, 4.0, m)         # right band
    v[2 * m:3 * m] = rng.uniform(-4.0, 3.0, m)                 # top band
    v[3 * m:4 * m] = H - 1 + rng.uniform(-3.0, 4.0, m)         # bottom band
    # exact integer coordinates (fraction 0), -3 .. 0 and W - 1 .. W + 2 among them
    edge_u = np.concatenate([np.arange(-3, 1), np.arange(W - 1, W + 3)])
    edge_v = np.concatenate([np.arange(-3, 1), np.arange(H - 1, H + 3)])
    k = np.arange(m)
    u[4 * m:5 * m] = np.where(k % 2 == 0, edge_u[rng.integers(0, 8, m)], rng.integers(-3, W + 3, m))
    v[4 * m:5 * m] = np.where(k % 3 == 0, edge_v[rng.integers(0, 8, m)], rng.integers(-3, H + 3, m))
    f = float(np.float32(1.1 * max(H, W)))
    if camera is None:
        K = (f, f, 0.5 * (W - 1), 0.5 * (H - 1))
    elif camera == "C":
        K = camera_C(H, W)
    else:
        raise ValueError(camera)
    z = rng.uniform(0.5, 5.0, n)
    xyz = np.stack([(u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z], axis=1)
    return dict(image=img, grid=np.ascontiguousarray(img.T), K=K, xyz=xyz, uv=np.stack([u, v], axis=1), H=H, W=W, kind=kind)


def _weights(x, one):
    """Catmull-Rom weights of the taps at -1, 0, 1, 2 and their derivatives at fraction x"""
    h, two, three, four, five, nine, ten, eight = (one / 2, one * 2, one * 3, one * 4, one * 5, one * 9, one * 10, one * 8)
    x2 = x * x
    x3 = x2 * x
    w = [h * (two * x2 - x3 - x), h * (three * x3 - five * x2 + two), h * (four * x2 - three * x3 + x), h * (x3 - x2)]
    d = [h * (four * x - three * x2 - one), h * (nine * x2 - ten * x), h * (eight * x - nine * x2 + one), h * (three * x2 - two * x)]
    return w, d


def _rotation_and_derivatives(q):
    """R(q) as Eigen's toRotationMatrix gives it (no normalisation) and dR/dq_i, i = w, x, y, z"""
    w, x, y, z = q
    o = w * 0
    one = o + 1
    two = one * 2
    R = [[one - two * (y * y + z * z), two * (x * y - w * z), two * (x * z + w * y)],
         [two * (x * y + w * z), one - two * (x * x + z * z), two * (y * z - w * x)],
         [two * (x * z - w * y), two * (y * z + w * x), one - two * (x * x + y * y)]]
    dw = [[o, -z, y], [z, o, -x], [-y, x, o]]
    dx = [[o, y, z], [y, -two * x, -w], [z, w, -two * x]]
    dy = [[-two * y, x, w], [x, o, z], [-w, z, -two * y]]
    dz = [[-two * z, -w, x], [w, -two * z, y], [x, y, o]]
    return R, [[[two * e for e in row] for row in M] for M in (dw, dx, dy, dz)]


def _transposed(M):
    return [[M[j][i] for j in range(3)] for i in range(3)]


def _mat_vec(M, a):
    return [M[i][0] * a[0] + M[i][1] * a[1] + M[i][2] * a[2] for i in range(3)]


def functor(image, K, xyz, q, t, dtype=np.longdouble, z_guard=0.01, z_eps=0.0, distortion=None, T12=None, T12inv=None,
            rot_transposed=False, grad_K=None):
    """Residual and raw 1x6 row of every point in arithmetic `dtype` -> dict(r (n,), J (n, 6), u, v, valid,
    band: some tap outside [0, W) x [0, H)).  image: (H, W), [v][u].  distortion: (k1, k2, p1, p2, k3) of EAResidueEx;
    T12 (4x4): EAResidueSecondCam's rig transform (the pose acts between T12^-1 and T12).  rot_transposed: the point is
    warped by R(q)^T (the ROS node's functor indexes the row-major matrix column-wise), the row goes through
    (dR/dq_i)^T; with z_guard = 0 and z_eps = 0.001 that is the ROS flavour.  grad_K: (fx, fy) taken in the row only, r
    unchanged -- a deliberately wrong reference for tests/test_camera_axes_reference.py, never a kernel's yardstick."""
    ty = np.dtype(dtype).type
    img = np.asarray(image).astype(dtype)
    H, W = img.shape
    fx, fy, cx, cy = [ty(k) for k in K]
    P = np.asarray(xyz)[:, :3].astype(dtype)
    # (float64 poses, as every kernel takes them, pass unchanged; a longdouble pose keeps its bits for difference quotients)
    q = [ty(e) for e in np.asarray(q).astype(dtype)]
    t = [ty(e) for e in np.asarray(t).astype(dtype)]
    one = ty(1)
    a = [P[:, 0], P[:, 1], P[:, 2]]
    if T12 is not None:
        A = np.asarray(T12, dtype=np.float64).reshape(4, 4)
        Ai = np.asarray(T12inv, dtype=np.float64).reshape(4, 4) if T12inv is not None else np.linalg.inv(A)
        A, Ai = A.astype(dtype), Ai.astype(dtype)
        a = [m + Ai[i, 3] for i, m in enumerate(_mat_vec(Ai, a))]
    R, dR = _rotation_and_derivatives(q)
    if rot_transposed:
        R, dR = _transposed(R), [_transposed(M) for M in dR]
    c = [m + t[i] for i, m in enumerate(_mat_vec(R, a))]
    b = [m + A[i, 3] for i, m in enumerate(_mat_vec(A, c))] if T12 is not None else c
    valid = ~((b[2] < ty(z_guard)) & (b[2] > -ty(z_guard))) if z_guard > 0 else np.ones(len(P), bool)
    bz = np.where(valid, b[2], one) + ty(z_eps)
    x, y = b[0] / bz, b[1] / bz
    if distortion is not None:
        k1, k2, p1, p2, k3 = [ty(e) for e in distortion]
        two, three, six = one * 2, one * 3, one * 6
        r2 = x * x + y * y
        D = one + r2 * (k1 + r2 * (k2 + r2 * k3))
        Dp = k1 + r2 * (two * k2 + three * k3 * r2)
        xd = x * D + two * p1 * x * y + p2 * (r2 + two * x * x)
        yd = y * D + two * p2 * x * y + p1 * (r2 + two * y * y)
        xd_x = D + two * x * x * Dp + two * p1 * y + six * p2 * x
        xd_y = two * x * y * Dp + two * p1 * x + two * p2 * y
        yd_x = xd_y
        yd_y = D + two * y * y * Dp + two * p2 * x + six * p1 * y
    else:
        xd, yd, xd_x, xd_y, yd_x, yd_y = x, y, one, one * 0, one * 0, one
    u = fx * xd + cx
    v = fy * yd + cy
    big = ty(1e9)
    uf, vf = np.floor(np.clip(u, -big, big)), np.floor(np.clip(v, -big, big))
    iu, iv = uf.astype(np.int64), vf.astype(np.int64)
    wu, du = _weights(u - uf, one)
    wv, dv = _weights(v - vf, one)
    f = np.zeros(len(P), dtype)
    Fu = np.zeros(len(P), dtype)
    Fv = np.zeros(len(P), dtype)
    for k in range(4):
        vi = np.clip(iv - 1 + k, 0, H - 1)          # each tap index clamped on its own (Grid2D::GetValue)
        for l in range(4):
            ui = np.clip(iu - 1 + l, 0, W - 1)
            p = img[vi, ui]
            f = f + wv[k] * wu[l] * p
            Fu = Fu + wv[k] * du[l] * p
            Fv = Fv + dv[k] * wu[l] * p
    # d f / d b' through the projection (and the distortion), then back through T12 to the point the pose acts on
    gfx, gfy = (fx, fy) if grad_K is None else (ty(grad_K[0]), ty(grad_K[1]))
    gx = (Fu * gfx * xd_x + Fv * gfy * yd_x) / bz
    gy = (Fu * gfx * xd_y + Fv * gfy * yd_y) / bz
    gb = [gx, gy, -(gx * x + gy * y)]
    g = [A[0, i] * gb[0] + A[1, i] * gb[1] + A[2, i] * gb[2] for i in range(3)] if T12 is not None else gb
    Jq = []
    for M in dR:
        m = _mat_vec(M, a)
        Jq.append(g[0] * m[0] + g[1] * m[1] + g[2] * m[2])
    qw, qx, qy, qz = q
    # Ceres' QuaternionParameterization: x (+) delta = [cos|d|, sin|d| d / |d|] * x; its Jacobian at delta = 0
    plus = [[-qx, -qy, -qz], [qw, qz, -qy], [-qz, qw, qx], [qy, -qx, qw]]
    J = [sum(Jq[i] * plus[i][j] for i in range(4)) for j in range(3)] + g
    J = np.stack(J, axis=1)
    r = f.copy()
    r[~valid] = np.nan
    J[~valid] = np.nan
    band = (iu - 1 < 0) | (iu + 2 > W - 1) | (iv - 1 < 0) | (iv + 2 > H - 1)
    return dict(r=r, J=J, u=u, v=v, valid=valid, band=band)


def with_loss(raw, kind, a, weights=None):
    """Ceres' loss (rho, rho') at s = r^2 and its corrector (rho'' <= 0 for these three: both scale by sqrt(rho')) on the
    output of `functor` -> dict(r, J corrected, rho); the arithmetic type is the one of raw['r'].  weights: one per point,
    ceres::ScaledLoss(loss, w_i) per block -- rho and rho' times w_i, so rows scale by sqrt(w_i rho')"""
    r, J = raw["r"], raw["J"]
    ty = r.dtype.type
    s = r * r
    one = ty(1)
    if kind == LOSS_CAUCHY:
        b = ty(a) * ty(a)
        rho, w = b * np.log1p(s / b), one / (one + s / b)
    elif kind == LOSS_HUBER:
        b = ty(a) * ty(a)
        rt = np.sqrt(np.where(s > b, s, one))
        rho, w = np.where(s > b, ty(2) * ty(a) * rt - b, s), np.where(s > b, ty(a) / rt, one)
    else:
        rho, w = s, np.ones_like(s)
    if weights is not None:
        wt = np.asarray(weights).astype(r.dtype)
        assert wt.shape == r.shape
        rho, w = wt * rho, wt * w
    sq = np.sqrt(w)
    return dict(r=r * sq, J=J * sq[:, None], rho=rho)


def sums(rows):
    """cost, JtJ, Jtr of the valid rows, summed in the rows' own arithmetic type"""
    ok = ~np.isnan(rows["r"])
    r, J = rows["r"][ok], rows["J"][ok]
    ty = r.dtype.type
    return dict(cost=ty(0.5) * np.sum(rows["rho"][ok], dtype=r.dtype), JtJ=(J.T @ J), Jtr=(J.T @ r), n_invalid=int((~ok).sum()))


def dev_r(got, ref):
    """largest absolute deviation of residuals"""
    return float(np.abs(np.asarray(got).astype(np.longdouble) - ref).max())


def dev_rel(got, ref, floor=1e-300):
    """largest deviation relative to the largest entry of the reference, which counts as at least `floor`"""
    ref = np.asarray(ref, dtype=np.longdouble)
    return float(np.abs(np.asarray(got).astype(np.longdouble) - ref).max() / max(np.abs(ref).max(), np.longdouble(floor)))


def dev_J(got, ref):
    """rows and their sums: relative to the largest entry.  Entries are (image gradient) x d(u, v)/d pose with
    |d(u, v)/d pose| of order fx >= 1.1, so the largest is far above 1 for any image that has a gradient; on a 1 x 1
    image the gradient is exactly zero, every row is rounding noise, and the floor of 1 makes the comparison absolute."""
    return dev_rel(got, ref, floor=1.0)


def dev_sums(got, ref):
    """cost, JtJ and Jtr of an evaluation against sums(reference rows): the largest of the three relative deviations"""
    return max(dev_rel(got["cost"], ref["cost"]), dev_J(got["JtJ"], ref["JtJ"]), dev_J(got["Jtr"], ref["Jtr"]))


# the project's bounds (tests/test_gpu_rows.py, tests/test_gpu_shapes.py): set on 120 x 160 images of a smooth DT in [0, 1]
PROJECT = {np.float64: dict(r=1e-12, J=1e-12, sums=1e-11), np.float32: dict(r=2e-5, J=2e-4, sums=1e-4)}


def bounds(ref_rows, plain_rows, base, image):
    """Bounds for a kernel on one case: the larger of the project's bound `base` and 4x the deviation of the plain
    restatement IN THE KERNEL'S PRECISION (plain_rows) from the extended reference (ref_rows).  On large images of noise
    texels the rounding of u - floor(u) alone, ulp(u) x a gradient of order 1, exceeds the project's bounds, most clearly
    in fp32 at 640 pixels.  The factor 4 covers FMA contraction, rcp-based division and another operation order at equal
    precision.  Measured on the CPU against the reference, never against a device.
    -> dict(r, J, sums, plain_r, plain_J, plain_sums)"""
    d = dict(plain_r=dev_r(plain_rows["r"], ref_rows["r"]), plain_J=dev_J(plain_rows["J"], ref_rows["J"]),
             plain_sums=dev_sums(sums(plain_rows), sums(ref_rows)))
    # the project's absolute bound on r is stated for texels in [0, 1] (test_gpu_rows.py: "on a DT in [0, 1]"); absolute
    # rounding error grows with the magnitude of the texels, so it is in units of the image's largest texel where that
    # exceeds 1 (the un-normalised distance transform of set_now_frame_ros reaches 255).  J and the sums are relative already.
    scale = max(1.0, float(np.abs(np.asarray(image, dtype=np.float64)).max()))
    d.update(r=max(base["r"] * scale, 4 * d["plain_r"]), J=max(base["J"], 4 * d["plain_J"]), sums=max(base["sums"], 4 * d["plain_sums"]))
    return d


def tolerances(pr, xyz, q, t, loss, dtype, ref_rows=None, base=None, weights=None, **variant):
    """`bounds` for a kernel of precision `dtype` on problem pr at pose (q, t) under `loss` (with per-point `weights`:
    weighted plain-precision rows against weighted extended-precision rows)"""
    if ref_rows is None:
        ref_rows = with_loss(functor(pr["image"], pr["K"], xyz, q, t, np.longdouble, **variant), *loss, weights=weights)
    plain = with_loss(functor(pr["image"], pr["K"], xyz, q, t, dtype, **variant), *loss, weights=weights)
    return bounds(ref_rows, plain, base or PROJECT[dtype], pr["image"])


# ---- one image + cloud resident in a Problem of the library, with the reference rows and bounds of its poses ----------

N_GPU = 1000   # points per case in the GPU modules (the CPU module uses 4000)
VARIANT_BASE = {np.float64: dict(r=1e-12, J=1e-11, sums=1e-11), np.float32: dict(r=5e-5, J=5e-4, sums=1e-4)}  # tests/test_gpu_rows.py
# a problem with per-point weights runs the variant kernels with the plain functor: the bounds tests/test_gpu_weights.py holds
# its rows to (J 1e-11; fp32 rows as the plain kernels) and this module's bounds on the sums
WEIGHTED_BASE = {np.float64: dict(r=1e-12, J=1e-11, sums=1e-11), np.float32: dict(r=2e-5, J=2e-4, sums=1e-4)}
_CACHE = {}   # references are pure functions of (case, precision, pose): computed once per test session


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def problem(H, W, kind, n=N_GPU, camera=None):
    return _cached(("problem", H, W, kind, n, camera),
                   lambda: band_problem(H, W, n, 100 + SHAPES.index((H, W)) if (H, W) in SHAPES else 300 + H + W, kind, camera))


class Case:
    """band_problem(H, W) in a Problem of dtype `dtype`.  upload: "grid" (set_dt_grid), "device image"
    (set_dt_image_device of a torch tensor) or a callable(P) that fills the image itself (a frame producer; the reference
    then takes Problem.get_dt() as the image, and `tag` names the producer for the cache).  weights: (values (n,), name)
    -> Problem.set_weights; corrected rows, sums and bounds are then those of the weighted problem, with the weights the
    device holds (Problem.get_weights).  camera: as band_problem's.  flavour: (z_guard, z_eps, rot_transposed) ->
    Problem.set_flavour, and the reference is evaluated with the same three.  Raises the library's EAError when the
    upload is refused."""

    def __init__(self, hip, H, W, kind, dtype, tile=None, variant=None, vname="", upload="grid", tag="", weights=None,
                 camera=None, flavour=None):
        self.hip, self.H, self.W, self.kind, self.dtype = hip, H, W, kind, dtype
        self.np = np.float32 if dtype == hip.EA_F32 else np.float64
        self.pr = problem(H, W, kind, camera=camera)
        self.variant = dict(variant or {})
        if flavour is not None:
            self.variant.update(z_guard=float(flavour[0]), z_eps=float(flavour[1]), rot_transposed=bool(flavour[2]))
        self.base = (VARIANT_BASE if variant else WEIGHTED_BASE if weights is not None else PROJECT)[self.np]
        self.weights = None
        self.P = P = hip.Problem(*self.pr["K"], dtype=dtype)
        try:
            if tile is not None:
                P.set_point_order(tile)
            P.set_points(self.pr["xyz"])
            self.image = self.pr["image"]
            if upload == "grid":
                P.set_dt_grid(self.pr["grid"])
            elif upload == "device image":
                import torch
                img = torch.tensor(self.image, dtype=torch.float32 if dtype == hip.EA_F32 else torch.float64, device="cuda")
                torch.cuda.synchronize()
                P.set_dt_image_device(img.data_ptr(), H, W)
            else:
                upload(P)
                self.image = P.get_dt()
            if "distortion" in self.variant:
                P.set_distortion(*self.variant["distortion"])
            if "T12" in self.variant:
                P.set_second_camera(self.variant["T12"])
            if flavour is not None:
                P.set_flavour(*flavour)
            # the reference is fed the points the device holds: the caller's doubles, rounded once by an fp32 problem
            self.xyz = P.get_points()
            want = self.pr["xyz"] if self.np is np.float64 else self.pr["xyz"].astype(np.float32).astype(np.float64)
            assert np.array_equal(self.xyz, want)
            if weights is not None:
                P.set_weights(weights[0])
                self.weights = P.get_weights()
                assert np.array_equal(self.weights, np.asarray(weights[0]).astype(self.np).astype(np.float64))
        except BaseException:
            P.close()
            raise
        self.key = (H, W, kind, self.np.__name__, vname, tag, weights[1] if weights is not None else "", camera,
                    tuple(flavour) if flavour is not None else None)

    def name(self):
        return "%dx%d %s%s%s %s" % (self.H, self.W, self.key[5] or self.kind, " cam" + self.key[7] if self.key[7] else "",
                                    " ros" if self.key[8] else "", "fp32" if self.np is np.float32 else "fp64")

    def _functor(self, pose, dtype):
        k = self.key + (tuple(pose[0]), tuple(pose[1]), np.dtype(dtype).name)
        return _cached(k, lambda: functor(self.image, self.pr["K"], self.xyz, pose[0], pose[1], dtype, **self.variant))

    def raw(self, pose, min_share=0.5):
        """reference rows without the loss; asserts the workload: nothing in the z guard, no NaN, a border workload"""
        raw = self._functor(pose, np.longdouble)
        assert raw["valid"].all() and not np.isnan(raw["J"].astype(np.float64)).any(), self.name()
        assert raw["band"].mean() >= min_share, (self.name(), float(raw["band"].mean()))
        return raw

    def rows(self, pose, loss, corrected=True):
        if not corrected:
            return self.raw(pose, 0.0)
        return _cached(self.key + (tuple(pose[0]), tuple(pose[1]), tuple(loss), "rows"), lambda: with_loss(self.raw(pose, 0.0), *loss, weights=self.weights))

    def sums(self, pose, loss):
        return _cached(self.key + (tuple(pose[0]), tuple(pose[1]), tuple(loss), "sums"), lambda: sums(self.rows(pose, loss)))

    def tol(self, pose, loss):
        def make():
            ref, plain = self.rows(pose, loss), with_loss(self._functor(pose, self.np), *loss, weights=self.weights)
            return bounds(ref, plain, self.base, self.image)
        return _cached(self.key + (tuple(pose[0]), tuple(pose[1]), tuple(loss), "tol"), make)

    def check_rows(self, r, J, pose, loss, corrected, where, seen=None):
        """every row against the reference: r absolutely, J relative to the largest entry"""
        ref, tol = self.rows(pose, loss, corrected), self.tol(pose, loss)
        assert r.shape == ref["r"].shape and J.shape == ref["J"].shape, where
        assert not np.isnan(r).any() and not np.isnan(J).any(), where
        dr, dJ = dev_r(r, ref["r"]), dev_J(J, ref["J"])
        if seen is not None:
            seen["r"], seen["J"] = max(seen.get("r", 0.0), dr), max(seen.get("J", 0.0), dJ)
        assert dr <= tol["r"], (self.name(), where, "r", dr, tol["r"], "worst point", int(np.abs(r - ref["r"].astype(np.float64)).argmax()))
        assert dJ <= tol["J"], (self.name(), where, "J", dJ, tol["J"])

    def check_sums(self, g, pose, loss, where, seen=None):
        """cost / JtJ / Jtr of one evaluation (a dict as Batch.eval returns it, one problem) against the reference's sums"""
        tol, es = self.tol(pose, loss), self.sums(pose, loss)
        got = dict(cost=float(np.asarray(g["cost"]).reshape(-1)[0]), JtJ=np.asarray(g["JtJ"]).reshape(6, 6), Jtr=np.asarray(g["Jtr"]).reshape(6))
        assert int(np.asarray(g["n_invalid"]).reshape(-1)[0]) == 0, where
        d = dev_sums(got, es)
        if seen is not None:
            seen["sums"] = max(seen.get("sums", 0.0), d)
        assert d <= tol["sums"], (self.name(), where, "sums", d, tol["sums"])

    def report(self, seen, pose, loss, what):
        t = self.tol(pose, loss)
        print("BAND-GPU %-24s %-12s plain r %.1e J %.1e sums %.1e | bound r %.1e J %.1e sums %.1e | device r %.1e J %.1e sums %.1e"
              % (self.name(), what, t["plain_r"], t["plain_J"], t["plain_sums"], t["r"], t["J"], t["sums"],
                 seen.get("r", float("nan")), seen.get("J", float("nan")), seen.get("sums", float("nan"))))

    def close(self):
        self.P.close()


def make_case(hip, H, W, kind, dtype, **kw):
    """A Case, or None when the library REFUSES the image with an error code and a message -- allowed only for images
    smaller than the stencil; a silent different answer is caught by the comparisons."""
    try:
        return Case(hip, H, W, kind, dtype, **kw)
    except hip.EAError as e:
        assert (H, W) in SMALL_SHAPES and e.code != hip.EA_OK and hip.load().ea_last_error().decode(), (H, W, str(e))
        return None
