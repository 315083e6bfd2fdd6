"""numpy restatement of include/ea_hip.h's reprojection section: ea_pose_to_matrix / ea_matrix_to_pose, the 3x4 matrix of
step A (rig product included), the per-point projection of step B, the inside rule and the paint of the overlay.

Every sum is written out left to right on float64 arrays -- never `@`, dot or einsum, because BLAS may fuse or reorder -- so
that each element goes through the IEEE operations the header lists, in its order: the device is held to these bits."""
import numpy as np


def pose_to_matrix(q, t):
    """Eigen's Quaternion::toRotationMatrix arithmetic on q = (w, x, y, z) as given, t in column 3"""
    w, x, y, z = (np.float64(v) for v in q)
    two = np.float64(2.0)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = np.float64(1.0)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy, t[0]],
                     [txy + twz, one - (txx + tzz), tyz - twx, t[1]],
                     [txz - twy, tyz + twx, one - (txx + tyy), t[2]],
                     [0.0, 0.0, 0.0, 1.0]], dtype=np.float64)


def matrix_to_pose(m):
    """Eigen's quaternion from a rotation matrix; None where the library refuses (m33 != 1)"""
    m = np.asarray(m, dtype=np.float64).reshape(4, 4)
    if not m[3, 3] == 1.0:
        return None
    q = np.zeros(4)
    half = np.float64(0.5)
    with np.errstate(invalid="ignore", divide="ignore"):
        tr = (m[0, 0] + m[1, 1]) + m[2, 2]
        if tr > 0.0:
            s = np.sqrt(tr + np.float64(1.0))
            q[0] = half * s
            s = half / s
            q[1] = (m[2, 1] - m[1, 2]) * s
            q[2] = (m[0, 2] - m[2, 0]) * s
            q[3] = (m[1, 0] - m[0, 1]) * s
        else:
            i = 0
            if m[1, 1] > m[0, 0]:
                i = 1
            if m[2, 2] > m[i, i]:
                i = 2
            j = (i + 1) % 3
            k = (j + 1) % 3
            s = np.sqrt(((m[i, i] - m[j, j]) - m[k, k]) + np.float64(1.0))
            q[1 + i] = half * s
            s = half / s
            q[0] = (m[k, j] - m[j, k]) * s
            q[1 + j] = (m[j, i] + m[i, j]) * s
            q[1 + k] = (m[k, i] + m[i, k]) * s
    return q, m[:3, 3].copy()


def mul4(a, b):
    """4x4 product, every entry ((a0 b0 + a1 b1) + a2 b2) + a3 b3"""
    a, b = np.asarray(a, dtype=np.float64).reshape(4, 4), np.asarray(b, dtype=np.float64).reshape(4, 4)
    c = np.zeros((4, 4))
    for r in range(4):
        for col in range(4):
            c[r, col] = ((a[r, 0] * b[0, col] + a[r, 1] * b[1, col]) + a[r, 2] * b[2, col]) + a[r, 3] * b[3, col]
    return c


def rig_matrix(b_T_a, T12, T12inv):
    """(T12 b_T_a) T12inv, rows 0-2"""
    return mul4(mul4(T12, b_T_a), T12inv)[:3].copy()


def plain_matrix(b_T_a):
    return np.asarray(b_T_a, dtype=np.float64).reshape(4, 4)[:3].copy()


def reproject(xyz, M, K, dist=None):
    """(u, v) [n, 2] of the points xyz [n, >= 3] under the 3x4 (or 4x4: its rows 0-2) matrix M; K = (fx, fy, cx, cy);
    dist = (k1, k2, p1, p2, k3) BY NAME, or None for the overloads without distortion"""
    xyz = np.asarray(xyz, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    fx, fy, cx, cy = (np.float64(v) for v in K)
    with np.errstate(all="ignore"):
        bx = ((M[0, 0] * x + M[0, 1] * y) + M[0, 2] * z) + M[0, 3]
        by = ((M[1, 0] * x + M[1, 1] * y) + M[1, 2] * z) + M[1, 3]
        bz = ((M[2, 0] * x + M[2, 1] * y) + M[2, 2] * z) + M[2, 3]
        xn, yn = bx / bz, by / bz
        xd, yd = xn, yn
        if dist is not None:
            k1, k2, p1, p2, k3 = (np.float64(v) for v in dist)
            one, two = np.float64(1.0), np.float64(2.0)
            r2 = xn * xn + yn * yn
            r4 = r2 * r2
            r6 = r4 * r2
            rad = ((one + k1 * r2) + k2 * r4) + k3 * r6
            xd = (xn * rad + ((two * p1) * xn) * yn) + p2 * (r2 + (two * xn) * xn)
            yd = (yn * rad + ((two * p2) * xn) * yn) + p1 * (r2 + (two * yn) * yn)
        u = fx * xd + cx
        v = fy * yd + cy
    return np.stack([u, v], axis=1)


def inside_mask(uv, H, W):
    """ea_pixel_cost_kernel's rule on (u, v): finite, |.| < 1e9, 0 <= (int)u < W, 0 <= (int)v < H, u > -1, v > -1"""
    uv = np.asarray(uv, dtype=np.float64)
    u, v = uv[:, 0], uv[:, 1]
    with np.errstate(invalid="ignore"):
        fin = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
        iu = np.where(fin, np.trunc(np.where(fin, u, 0.0)), -1).astype(np.int64)
        iv = np.where(fin, np.trunc(np.where(fin, v, 0.0)), -1).astype(np.int64)
        return fin & (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H) & (u > -1.0) & (v > -1.0)


def overlay(image, uv, color=(0, 0, 255)):
    """s_overlay with the points outside skipped: (painted copy, dict n / inside / outside)"""
    out = np.array(image, dtype=np.uint8, copy=True)
    H, W = out.shape[:2]
    uv = np.asarray(uv, dtype=np.float64).reshape(-1, 2)
    ok = inside_mask(uv, H, W)
    iu = np.trunc(uv[ok, 0]).astype(np.int64)
    iv = np.trunc(uv[ok, 1]).astype(np.int64)
    out[iv, iu] = np.asarray(color, dtype=np.uint8)
    return out, dict(n=int(uv.shape[0]), inside=int(ok.sum()), outside=int((~ok).sum()))


def branch_quaternions():
    """unit quaternions for each branch of Eigen's conversion, signed as it returns them (w > 0, resp. q[i] > 0)"""
    rng = np.random.default_rng(21)
    out = {"trace": [], "x": [], "y": [], "z": []}
    while min(len(v) for v in out.values()) < 40:
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        if abs(q[0]) > 0.5:
            out["trace"].append(q * np.sign(q[0]))
        elif abs(q[0]) < 0.45:
            i = int(np.argmax(np.abs(q[1:])))
            out["xyz"[i]].append(q * np.sign(q[1 + i]))
    out["trace"].append(np.array([1.0, 0.0, 0.0, 0.0]))
    out["x"].append(np.array([0.0, 1.0, 0.0, 0.0]))
    out["y"].append(np.array([0.0, 0.0, 1.0, 0.0]))
    out["z"].append(np.array([0.0, 0.0, 0.0, 1.0]))
    s = float(np.sqrt(0.5))
    out["x"].append(np.array([0.0, s, s, 0.0]))     # m00 == m11: the tie goes to the first
    return out
