"""numpy restatement of include/ea_hip.h's depth gate section: the validity and conversion of a depth sample of either kind,
BEHIND / OUTSIDE, the window scan in raster order with its tie rule, the classification, the factor and the weight.

The matrix and the projection are tests/reproject_ref.py's (step A, step B); bz is written out here in the same order.  As
there, every element goes through the IEEE operations the header lists, in its order: the device and the host header are held
to these bytes and bits."""
import numpy as np

import reproject_ref as rr

BEHIND, OUTSIDE, UNKNOWN, CONSISTENT, OCCLUDED, FREE = range(6)
NAMES = ("n_behind", "n_outside", "n_unknown", "n_consistent", "n_occluded", "n_free")
DEFAULTS = dict(radius=1, abs_tol=0.02, rel_tol=0.02, w_occluded=0.0, w_free=0.0, w_unknown=1.0, apply=1)


def depth_metres(depth, z_scaling=5000.0):
    """(metric depth float64 [H, W], valid [H, W]) of a uint16 image (d / z_scaling, valid when d != 0) or a float32 one
    (metres, valid when > 0 and finite)"""
    depth = np.asarray(depth)
    if depth.dtype == np.uint16:
        return depth.astype(np.float64) / np.float64(z_scaling), depth != 0
    if depth.dtype == np.float32:
        with np.errstate(invalid="ignore"):
            return depth.astype(np.float64), (depth > 0) & np.isfinite(depth)
    raise ValueError("uint16 or float32")


def depth_of_points(xyz, M):
    """bz = ((M20 x + M21 y) + M22 z) + M23"""
    xyz = np.asarray(xyz, dtype=np.float64)
    M = np.asarray(M, dtype=np.float64)
    with np.errstate(all="ignore"):
        return ((M[2, 0] * xyz[:, 0] + M[2, 1] * xyz[:, 1]) + M[2, 2] * xyz[:, 2]) + M[2, 3]


def classify(xyz, M, K, depth, z_scaling=5000.0, radius=1, abs_tol=0.02, rel_tol=0.02, dist=None, details=False):
    """class bytes [n] of the points xyz under the 3x4 matrix M (step A done); with details also a dict: bz, the kept d, tol,
    diff, and `tie` -- the points whose window held a later valid sample as far from bz as the kept one but on the other side"""
    xyz = np.asarray(xyz, dtype=np.float64)
    n = xyz.shape[0]
    metres, valid = depth_metres(depth, z_scaling)
    H, W = metres.shape
    uv = rr.reproject(xyz, M, K, dist)
    bz = depth_of_points(xyz, M)
    with np.errstate(invalid="ignore"):
        behind = ~((bz > 0.0) & (bz < np.inf))
    inside = rr.inside_mask(uv, H, W)
    act = ~behind & inside
    cls = np.full(n, OUTSIDE, np.uint8)
    cls[behind] = BEHIND
    iu = np.trunc(np.where(act, uv[:, 0], 0.0)).astype(np.int64)
    iv = np.trunc(np.where(act, uv[:, 1], 0.0)).astype(np.int64)
    have = np.zeros(n, bool)
    tie = np.zeros(n, bool)
    best, best_e = np.zeros(n), np.zeros(n)
    r = int(radius)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                row, col = iv + dy, iu + dx
                inb = act & (row >= 0) & (row < H) & (col >= 0) & (col < W)
                rc, cc = np.clip(row, 0, H - 1), np.clip(col, 0, W - 1)
                ok = inb & valid[rc, cc]
                d = metres[rc, cc]
                e = np.abs(d - bz)
                tie |= ok & have & (e == best_e) & (e > 0.0) & (np.sign(d - bz) != np.sign(best - bz))
                take = ok & (~have | (e < best_e))
                best = np.where(take, d, best)
                best_e = np.where(take, e, best_e)
                have |= take
        tol = np.float64(abs_tol) + np.float64(rel_tol) * bz
        diff = best - bz
        consistent = np.abs(diff) <= tol
    cls[act & ~have] = UNKNOWN
    cls[act & have & consistent] = CONSISTENT
    cls[act & have & ~consistent & (diff < 0.0)] = OCCLUDED
    cls[act & have & ~consistent & ~(diff < 0.0)] = FREE
    if details:
        return cls, dict(bz=bz, d=best, tol=tol, diff=diff, tie=tie & act, have=have & act)
    return cls


def depth_factor(z, z_ref, power):
    """dd = min(1, (z_ref / z)^power) as the producers form it before their rounding; power <= 0: 1"""
    z = np.asarray(z, dtype=np.float64)
    if power <= 0:
        return np.ones_like(z)
    with np.errstate(all="ignore"):
        ratio = np.float64(z_ref) / z
        v = ratio.copy()
        for _ in range(power - 1):
            v = v * ratio
        return np.fmax(0.0, np.fmin(1.0, v))


def weights(cls, z, w_occluded=0.0, w_free=0.0, w_unknown=1.0, depth_weighting=None, f32=False):
    """w = g * dd, rounded once to the problem dtype (returned as float64); z: the stored point depths;
    depth_weighting = (z_ref, power) or None"""
    g = np.ones(len(cls))
    g[cls == UNKNOWN] = w_unknown
    g[cls == OCCLUDED] = w_occluded
    g[cls == FREE] = w_free
    dd = depth_factor(z, *depth_weighting) if depth_weighting else np.ones(len(cls))
    w = g * dd
    return w.astype(np.float32).astype(np.float64) if f32 else w


def stats(cls):
    out = dict(n=int(len(cls)))
    for c, name in enumerate(NAMES):
        out[name] = int((np.asarray(cls) == c).sum())
    return out


def params_ok(radius=1, abs_tol=0.02, rel_tol=0.02, w_occluded=0.0, w_free=0.0, w_unknown=1.0, apply=1):
    fin = all(np.isfinite(v) and v >= 0.0 for v in (abs_tol, rel_tol, w_occluded, w_free, w_unknown))
    return 0 <= radius <= 3 and fin


def now_depth_args_ok(kind, height, width, z_scaling):
    if kind not in (0, 1) or not (3 <= height <= 32768) or not (3 <= width <= 32768):
        return False
    return kind == 1 or (np.isfinite(z_scaling) and z_scaling > 0.0)
