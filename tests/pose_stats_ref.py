"""ea_pose_stats restated in numpy fp64 from the definitions in include/ea_hip.h, and the fixtures of
tests/test_gpu_pose_stats.py: synthetic problems of edge_alignment_amd/synth.py on two small images, the problem kinds, the
poses, and the condition every fixture must meet so that the counts are decided well away from a rounding error."""
import numpy as np

from edge_alignment_amd import synth
from oracle import ea_numpy

IDENTITY_Q, IDENTITY_T = np.array([1.0, 0.0, 0.0, 0.0]), np.zeros(3)
DIST = (0.12, -0.21, -0.004, 0.003, 0.05)   # k1, k2, p1, p2, k3
T12 = synth.rigid_4x4(synth.quat_from_axis_angle([0.1, 1.0, -0.2], 0.05), (0.04, -0.01, 0.02))
INLIER = 0.11                                # of a DT normalised to [0, 1]: the threshold is the widest gap of |r| around it

# (H, W), camera, margin, seed
IMAGES = {
    "17x61": dict(H=17, W=61, K=(45.0, 44.0, 30.2, 8.1), margin=0, seed=11),
    "37x70": dict(H=37, W=70, K=(60.0, 58.0, 34.4, 18.3), margin=3, seed=12),
}
SIZES = (1, 63, 64, 65, 257, 1000)
# kind: (distortion, second camera, weights, flavour knobs or None)
KINDS = {
    "plain": (False, False, False, None),
    "weighted": (False, False, True, None),
    "distortion": (True, False, False, None),
    "second_camera": (False, True, False, None),
    "both": (True, True, False, None),
    "rot_transposed": (False, False, False, dict(z_guard=0.01, z_eps=0.0, rot_transposed=True)),
    "z_eps": (False, False, False, dict(z_guard=0.01, z_eps=0.001, rot_transposed=False)),
    "no_guard": (False, False, False, dict(z_guard=0.0, z_eps=0.0, rot_transposed=False)),
}
POSES = ("identity", "small", "far", "guard", "forward")


def image(name):
    im = IMAGES[name]
    pr = synth.make_problem(im["H"], im["W"], max(SIZES), 9, im["seed"], *im["K"], normalize=True, pixel_centres=False,
                            depth_range=(0.6, 4.0))
    xyz = pr["xyz"].copy()
    # three points that the identity does not see and a camera moved forward does: inside the guard, behind, behind
    xyz[5] = (0.0021, -0.0013, 0.0047)
    xyz[6] = (0.05, 0.02, -0.31)
    xyz[40] = (-0.08, 0.03, -0.22)
    return dict(grid=pr["grid"], xyz=xyz, **im)


def _affine(kind):
    """(Ai, di, A, d) of the second-camera functor: a' = Ai a + di, b = A (R a' + t) + d"""
    if not KINDS[kind][1]:
        return np.eye(3), np.zeros(3), np.eye(3), np.zeros(3)
    Ti = np.linalg.inv(T12)
    return Ti[:3, :3], Ti[:3, 3], T12[:3, :3], T12[:3, 3]


def pose(kind, name, xyz, k=0):
    """the five poses; `guard` puts a point near the middle at b_z = 0.005 -- inside the guard, away from 0 and from the
    guard.  k = 0, 1, ...: the same pose nudged (translation stretched by k per cent, the guard pose on the k-th next point),
    for the search that keeps every decision of a fixture away from its threshold (settle)"""
    stretch = 1.0 + 0.01 * k
    if name == "identity":
        return IDENTITY_Q.copy(), IDENTITY_T.copy()
    if name == "small":
        return synth.quat_from_axis_angle([0.3, -1.0, 0.5], 0.09), stretch * np.array([0.05, -0.03, 0.04])
    if name == "far":
        return synth.quat_from_axis_angle([0.1, 1.0, 0.05], 0.8), stretch * np.array([0.35, 0.02, -1.3])
    if name == "forward":
        return synth.quat_from_axis_angle([1.0, 0.2, -0.4], 0.03), stretch * np.array([0.01, -0.02, 0.8])
    Ai, di, A, d = _affine(kind)
    a = xyz[(len(xyz) // 2 + k) % len(xyz)]
    b0 = A @ (Ai @ a + di) + d
    return IDENTITY_Q.copy(), np.linalg.solve(A, np.array([0.0, 0.0, 0.005 - b0[2]]))


def project(im, kind, xyz, q, t):
    """(u, v, valid, divisor) of every point, fp64"""
    dist, _, _, knobs = KINDS[kind]
    knobs = knobs or dict(z_guard=0.01, z_eps=0.0, rot_transposed=False)
    fx, fy, cx, cy = im["K"]
    R = synth.quat_to_R(np.asarray(q, dtype=np.float64))
    if knobs["rot_transposed"]:
        R = R.T
    Ai, di, A, d = _affine(kind)
    ap = xyz @ Ai.T + di
    b = (ap @ R.T + t) @ A.T + d
    zg = knobs["z_guard"]
    valid = ~((b[:, 2] < zg) & (b[:, 2] > -zg)) if zg > 0 else np.ones(len(xyz), bool)
    div = b[:, 2] + knobs["z_eps"]
    with np.errstate(all="ignore"):
        x, y = b[:, 0] / div, b[:, 1] / div
        if dist:
            k1, k2, p1, p2, k3 = DIST
            r2 = x * x + y * y
            D = 1 + k1 * r2 + k2 * r2 ** 2 + k3 * r2 ** 3
            x, y = (x * D + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * D + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)
        u, v = fx * x + cx, fy * y + cy
    return u, v, valid, div


def reference(im, kind, xyz, q, t, margin, inlier_residual):
    """the statistics, and `slack`: how far the closest decision lies from its threshold -- (pixels from a visibility bound
    over the points in front, |r| from inlier_residual over the visible, depth from 0 and the guard over all)"""
    knobs = KINDS[kind][3] or dict(z_guard=0.01, z_eps=0.0)
    W, H = im["W"], im["H"]
    u, v, valid, div = project(im, kind, xyz, q, t)
    front = valid & (div > 0)
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u), np.floor(v)
        visible = front & (fu >= margin) & (fu <= W - 2 - margin) & (fv >= margin) & (fv <= H - 2 - margin)
    r = np.zeros(len(xyz))
    r[visible] = ea_numpy.bicubic(im["grid"], u[visible], v[visible])[0]
    inlier = visible & (np.abs(r) <= inlier_residual)
    u0, v0, valid0, div0 = project(im, kind, xyz, IDENTITY_Q, IDENTITY_T)
    flow = visible & valid0 & (div0 > 0)
    dist = np.sqrt((u[flow] - u0[flow]) ** 2 + (v[flow] - v0[flow]) ** 2)
    stats = dict(n=len(xyz), n_invalid=int((~valid).sum()), n_visible=int(visible.sum()), n_inlier=int(inlier.sum()),
                 n_flow=int(flow.sum()), sum_flow=float(dist.sum()))
    bounds = (float(margin), float(W - 1 - margin)), (float(margin), float(H - 1 - margin))
    px = np.inf
    for coord, bb in ((u[front], bounds[0]), (v[front], bounds[1])):
        c = coord[np.isfinite(coord)]
        for b in bb:
            if c.size:
                px = min(px, float(np.abs(c - b).min()))
    res = float(np.abs(np.abs(r[visible]) - inlier_residual).min()) if visible.any() else np.inf
    zg = knobs["z_guard"]
    depth = np.inf
    for dd in (div, div0):
        depth = min(depth, float(np.abs(dd).min()))
        bz = dd - knobs["z_eps"]
        if zg > 0:
            depth = min(depth, float(np.abs(np.abs(bz) - zg).min()))
    return stats, dict(pixels=px, residual=res, depth=depth)


# how close a fixture may come to a threshold: (pixels, residual, depth) per dtype name
SLACK = {"f64": (1e-9, 1e-9, 1e-9), "f32": (1e-3, 1e-4, 1e-3)}


def fixture_ok(slack, dtype_name):
    px, res, depth = SLACK[dtype_name]
    return slack["pixels"] > px and slack["residual"] > res and slack["depth"] > depth


def inlier_threshold(im, kind, xyz, q, t, margin):
    """the middle of the widest gap between neighbouring |r| of the visible points in [INLIER / 2, 2 INLIER]"""
    u, v, valid, div = project(im, kind, xyz, q, t)
    with np.errstate(all="ignore"):
        fu, fv = np.floor(u), np.floor(v)
        visible = valid & (div > 0) & (fu >= margin) & (fu <= im["W"] - 2 - margin) & (fv >= margin) & (fv <= im["H"] - 2 - margin)
    r = np.abs(ea_numpy.bicubic(im["grid"], u[visible], v[visible])[0]) if visible.any() else np.zeros(0)
    knots = np.sort(np.concatenate([[INLIER / 2, 2 * INLIER], r[(r > INLIER / 2) & (r < 2 * INLIER)]]))
    i = int(np.argmax(np.diff(knots)))
    return float(0.5 * (knots[i] + knots[i + 1]))


def settle(im, kind, xyz, pname, tries=200):
    """the first nudge of the pose at which the fixture meets the fp32 condition (and with it the fp64 one); computed on the
    CPU, and deterministic.  The test asserts the condition again on what comes back."""
    for k in range(tries):
        q, t = pose(kind, pname, xyz, k)
        thr = inlier_threshold(im, kind, xyz, q, t, im["margin"])
        stats, slack = reference(im, kind, xyz, q, t, im["margin"], thr)
        if fixture_ok(slack, "f32"):
            break
    return dict(q=q, t=t, inlier_residual=thr, stats=stats, slack=slack, nudge=k)


def cases():
    """every (image, kind, n, pose) of the file with its pose, threshold, margin and the fp64 reference"""
    out = []
    for iname in IMAGES:
        im = image(iname)
        for kind in KINDS:
            for n in SIZES:
                for pname in POSES:
                    c = settle(im, kind, im["xyz"][:n], pname)
                    c.update(image=iname, kind=kind, n=n, pose=pname, margin=im["margin"])
                    out.append(c)
    return out
