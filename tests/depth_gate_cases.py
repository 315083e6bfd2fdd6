"""Inputs of the depth gate tests, shared by the host-header test and the GPU test: the images, cameras and matrices of
tests/test_gpu_reproject.py (restated here so that the CPU test stands alone; the GPU test asserts they are the same), depth
images built from dyadic values with invalid samples of every sort, and points planted on exact class boundaries.

Depth values are multiples of 1/4 (U16: raw multiples of 256 with z_scaling = 1024; F32: the same metres), so d - bz is exact
for the planted dyadic point depths under the identity, where bz == z.  With rel_tol = 0 and abs_tol = 0.25 (TOL) the image
values 1.25, 1.75 and 2.5 put
  z = 2.0 and z = 1.0        exactly on the boundary, |d - bz| == tol: CONSISTENT,
  z = nextafter(2.0, 3)      one ulp (of the problem dtype) beyond it against 1.75: OCCLUDED,
  z = nextafter(1.0, 0)      one ulp beyond it against 1.25: FREE,
  z = 1.5                    between a 1.25 and a 1.75 of one window, both 0.25 away: the tie keeps the first in raster order
                             (with abs_tol = 0.125 the class says which one was kept)."""
import numpy as np

import reproject_ref as rr

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
SMALL = dict(H=5, W=7, K=(6.5, 5.25, 3.25, 2.5))
BIG = dict(H=48, W=64, K=(61.0, 57.5, 31.25, 24.5))
DIST = (0.11, -0.07, 0.013, -0.009, 0.021)            # k1, k2, p1, p2, k3
T12 = rr.pose_to_matrix([0.9998, 0.01, -0.012, 0.008], [0.11, -0.004, 0.006])
T12INV = np.linalg.inv(T12)
T12INV[3] = (0.0, 0.0, 0.0, 1.0)
VARIANTS = {"plain": (False, False), "distortion": (True, False), "rig": (False, True), "both": (True, True)}
MATRICES = {
    "identity": np.eye(4),
    "rigid": rr.pose_to_matrix([0.995, 0.03, -0.05, 0.07], [0.05, -0.02, 0.1]),
    "degenerate": np.array([[1.0, 0, 0, 0.015625], [0, 1.0, 0, -0.03125], [0, 0, 1.0, -1.0], [0, 0, 0, 1.0]]),
}
Z_SCALING = 1024.0
TOL = dict(abs_tol=0.25, rel_tol=0.0)

# metres; 0 marks "no measurement"
_SMALL_METRES = np.array([[1.25, 1.75, 0.0, 2.5, 1.25, 1.75, 0.0],
                          [1.75, 0.0, 1.25, 1.75, 2.5, 0.0, 1.25],
                          [0.0, 1.25, 1.75, 1.25, 1.75, 2.5, 1.75],
                          [2.5, 1.75, 1.25, 0.0, 1.25, 1.75, 1.25],
                          [1.25, 0.0, 2.5, 1.75, 0.0, 1.25, 2.5]])
_INVALID_F32 = (np.nan, -1.0, 0.0, np.inf, -np.inf, -0.0)


def _as_kind(metres, kind):
    """the image in its kind: U16 raw = metres * 1024 (0 stays 0); F32 metres with the invalid slots cycling through NaN,
    -1, 0, +Inf, -Inf, -0"""
    if kind == "u16":
        return np.ascontiguousarray(metres * Z_SCALING).astype(np.uint16)
    out = metres.astype(np.float32)
    rows, cols = np.nonzero(metres == 0.0)
    for k, (r, c) in enumerate(zip(rows, cols)):
        out[r, c] = _INVALID_F32[k % len(_INVALID_F32)]
    return out


def depth_image(im, kind, seed=5):
    """5 x 7: the pattern above.  Larger: seeded multiples of 1/4 in 0.5 .. 3.25, every eleventh sample invalid, and an
    invalid block of 16 x 20 in which windows of every radius find nothing"""
    if (im["H"], im["W"]) == (5, 7):
        return _as_kind(_SMALL_METRES, kind)
    rng = np.random.default_rng(seed)
    metres = rng.integers(2, 14, (im["H"], im["W"])).astype(np.float64) / 4.0
    metres.reshape(-1)[::11] = 0.0
    metres[4:20, 6:26] = 0.0
    return _as_kind(metres, kind)


def _at_pixel(u, v, z, K):
    fx, fy, cx, cy = K
    return ((u - cx) * z / fx, (v - cy) * z / fy, z)


def planted(f32):
    """the boundary points on the 5 x 7 image (under the identity): rows of (x, y, z) and what each is"""
    K = SMALL["K"]
    ft = np.float32 if f32 else np.float64
    up = float(np.nextafter(ft(2.0), ft(3.0)))
    down = float(np.nextafter(ft(1.0), ft(0.0)))
    pts, what = [], []
    for (u, v, z, name) in ((2.5, 2.5, 2.0, "boundary_below"),      # pixel (2, 2) holds 1.75: diff == -0.25
                            (3.5, 2.5, 1.0, "boundary_above"),      # pixel (2, 3) holds 1.25: diff == +0.25
                            (2.5, 2.5, up, "ulp_occluded"),
                            (3.5, 2.5, down, "ulp_free"),
                            (3.5, 2.5, 1.5, "tie_first_below"),     # radius >= 1: (1, 2) = 1.25 comes before any 1.75
                            (6.5, 3.5, 1.5, "tie_first_above")):    # radius 1: (2, 6) = 1.75 comes before (3, 6) = 1.25
        pts.append(_at_pixel(u, v, z, K))
        what.append(name)
    return np.array(pts), what


def points(n, seed, im, f32=False):
    """n points that project inside and around the image at the identity (as in tests/test_gpu_reproject.py: every seventh has
    z == 1 exactly, some z < 1); on the 5 x 7 image the planted boundary points come first, as many as fit"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = im["K"]
    z = rng.uniform(0.5, 3.0, n)
    z[::7] = 1.0
    u = rng.uniform(-0.2 * im["W"], 1.2 * im["W"], n)
    v = rng.uniform(-0.2 * im["H"], 1.2 * im["H"], n)
    xyz = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], axis=1)
    if (im["H"], im["W"]) == (5, 7) and n >= 63:
        pl, _ = planted(f32)
        xyz[:len(pl)] = pl
        xyz[7] = (-0.015625, 0.03125, 1.0)      # with the degenerate matrix: bx == by == bz == 0, 0 / 0 (NaN: BEHIND)
    return xyz


def matrix_for(variant, T):
    """step A for the variant"""
    return rr.rig_matrix(T, T12, T12INV) if VARIANTS[variant][1] else rr.plain_matrix(T)
