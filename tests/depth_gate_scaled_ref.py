"""numpy restatement of step 3b of include/ea_hip.h's depth gate section: the gate on a depth image of 2^s times the extent of
the problem's distance transform.  Steps 1-3 (BEHIND, OUTSIDE at the DT extent H x W) and 5-6 are tests/depth_gate_ref.py's,
called or written out as there; step 4 runs on the depth image's own extent around (IV, IU) = ((int)V, (int)U) with
U = u * 2^s + c, V = v * 2^s + c, c = (2^s - 1) / 2.  With s = 0 this is depth_gate_ref.classify, which the tests assert.

As there, every element goes through the IEEE operations the header lists, in its order."""
import numpy as np

import depth_gate_ref as dg
import reproject_ref as rr

MAX_SHIFT = 8


def shift_of(H, W, depth_H, depth_W):
    """the s in 0..8 with (depth_H, depth_W) == (H << s, W << s) and H * W << 2 s <= 2^30, or None: the extent rule of
    ea_*_depth_gate"""
    for s in range(MAX_SHIFT + 1):
        if (H * W) << (2 * s) > 1 << 30:
            break
        if (H << s, W << s) == (depth_H, depth_W):
            return s
    return None


def scaled_pixel(uv, s):
    """(IU, IV, U, V) of inside points: the multiplication is exact, the addition rounds once, truncation toward zero"""
    scale = np.float64(1 << s)
    c = (scale - np.float64(1.0)) * np.float64(0.5)
    U = uv[:, 0] * scale + c
    V = uv[:, 1] * scale + c
    return np.trunc(U).astype(np.int64), np.trunc(V).astype(np.int64), U, V


def classify(xyz, M, K, depth, s, z_scaling=5000.0, radius=1, abs_tol=0.02, rel_tol=0.02, dist=None, details=False):
    """class bytes [n]; depth is (H << s) x (W << s) of either kind, the DT extent H x W follows from it.  details: also a dict
    with bz, the kept d and the window centres IU, IV"""
    xyz = np.asarray(xyz, dtype=np.float64)
    n = xyz.shape[0]
    metres, valid = dg.depth_metres(depth, z_scaling)
    DH, DW = metres.shape
    assert DH % (1 << s) == 0 and DW % (1 << s) == 0
    H, W = DH >> s, DW >> s
    uv = rr.reproject(xyz, M, K, dist)
    bz = dg.depth_of_points(xyz, M)
    with np.errstate(invalid="ignore"):
        behind = ~((bz > 0.0) & (bz < np.inf))
    act = ~behind & rr.inside_mask(uv, H, W)                       # steps 2-3: at the DT extent
    cls = np.full(n, dg.OUTSIDE, np.uint8)
    cls[behind] = dg.BEHIND
    IU, IV, _, _ = scaled_pixel(np.where(act[:, None], uv, 0.0), s)  # step 3b
    have = np.zeros(n, bool)
    best, best_e = np.zeros(n), np.zeros(n)
    r = int(radius)
    with np.errstate(all="ignore"):
        for dy in range(-r, r + 1):                                # step 4: on the depth image's own extent
            for dx in range(-r, r + 1):
                row, col = IV + dy, IU + dx
                inb = act & (row >= 0) & (row < DH) & (col >= 0) & (col < DW)
                rc, cc = np.clip(row, 0, DH - 1), np.clip(col, 0, DW - 1)
                ok = inb & valid[rc, cc]
                d = metres[rc, cc]
                e = np.abs(d - bz)
                take = ok & (~have | (e < best_e))
                best = np.where(take, d, best)
                best_e = np.where(take, e, best_e)
                have |= take
        tol = np.float64(abs_tol) + np.float64(rel_tol) * bz       # step 5
        diff = best - bz
        consistent = np.abs(diff) <= tol
    cls[act & ~have] = dg.UNKNOWN
    cls[act & have & consistent] = dg.CONSISTENT
    cls[act & have & ~consistent & (diff < 0.0)] = dg.OCCLUDED
    cls[act & have & ~consistent & ~(diff < 0.0)] = dg.FREE
    if details:
        return cls, dict(bz=bz, d=best, act=act, IU=np.where(act, IU, 0), IV=np.where(act, IV, 0))
    return cls


# ---- inputs shared by the host test and the GPU test ---------------------------------------------------------------------------

def depth_image(im, s, kind, z_scaling=1024.0, seed=9):
    """(H << s) x (W << s), multiples of 1/4 m (exact in both kinds at z_scaling = 1024): 1.5 m left of a depth step at 4/7 of
    the width and 2.5 m right of it, every fifth sample a hole, a hole block over the top-left 3 x 4 DT pixels in which the
    windows of every radius find nothing, and seeded 0.25 m ripples; F32 holes cycle through NaN, -1, 0, +Inf, -Inf, -0"""
    H, W = im["H"] << s, im["W"] << s
    rng = np.random.default_rng(seed + s)
    metres = np.where(np.arange(W)[None, :] < (4 * W) // 7, 1.5, 2.5) + rng.integers(-1, 2, (H, W)) / 4.0
    metres.reshape(-1)[::5] = 0.0
    metres[:3 << s, :4 << s] = 0.0
    if kind == "u16":
        return np.ascontiguousarray(metres * z_scaling).astype(np.uint16)
    out = metres.astype(np.float32)
    bad = (np.nan, -1.0, 0.0, np.inf, -np.inf, -0.0)
    rows, cols = np.nonzero(metres == 0.0)
    for k, (r, c) in enumerate(zip(rows, cols)):
        out[r, c] = bad[k % len(bad)]
    return out


def points(n, seed, im):
    """n >= 16 points for the identity: seeded ones inside and around the DT extent, and planted ones -- behind the camera,
    outside, in the hole block's corner (UNKNOWN at every radius and shift), -1 < u < 0 and -1 < v < 0 (IU, IV < 0 for s >= 1),
    just left of the last column's end and above the last row's (IU >= W << s, IV >= H << s for s >= 1)"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = im["K"]
    H, W = im["H"], im["W"]
    z = rng.uniform(0.75, 3.25, n)
    u = rng.uniform(-0.2 * W, 1.2 * W, n)
    v = rng.uniform(-0.2 * H, 1.2 * H, n)
    planted = [(3.5, 2.5, -1.0), (-1.5, 2.5, 1.5), (0.5, 0.5, 1.5), (-0.9, 3.5, 1.5), (5.5, -0.9, 2.5), (W - 0.1, 3.5, 2.5),
               (5.5, H - 0.1, 2.5), (W - 0.1, H - 0.1, 2.5), (-0.9, -0.9, 1.5), (5.5, 3.5, 2.5), (5.5, 3.5, 1.0), (5.5, 3.5, 4.0)]
    for k, (pu, pv, pz) in enumerate(planted):
        u[k], v[k], z[k] = pu, pv, pz
    return np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], axis=1)
