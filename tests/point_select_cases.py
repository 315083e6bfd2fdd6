"""Inputs shared by tests/test_point_select_host.py and tests/test_gpu_point_select.py: a camera on a 37 x 29 pixel grid (partial
cells on the right and bottom edges for cell_px = 4; fx != fy, the principal point off-centre) and point sets with several
points per pixel and per cell, points on cell borders, equal-z ties inside a cell, points outside the grid and points with
z <= 0, NaN or Inf."""
import numpy as np

H, W = 29, 37
K = (21.5, 19.25, 17.3, 13.6)
SIZES = (0, 1, 63, 64, 65, 1023, 1024, 1025, 2049)
CELLS = (0, 1, 4, 64)
# (stride, target as a function of n): stride > 1 and target > 0 do not go together
STRIDES = ((1, None), (2, None), (30, None), (1, lambda n: 5), (1, lambda n: n), (1, lambda n: n + 1))
Z_LEVELS = np.array([0.75, 1.0, 1.0, 1.5, 2.0, 2.0, 3.25])      # repeated depths: equal-z ties inside a cell


def back_project(u, v, z):
    """a producer's arithmetic (get_aX): X = (u - cx) * Z / fx"""
    fx, fy, cx, cy = K
    return np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], axis=1)


def points(n, seed):
    """n x 3 doubles; the kinds cycle through the point index so that every size holds every kind it has room for"""
    rng = np.random.default_rng(seed)
    kind = np.arange(n) % 16
    z = Z_LEVELS[rng.integers(0, len(Z_LEVELS), n)]
    pu = rng.integers(0, W, n).astype(np.float64)
    pv = rng.integers(0, H, n).astype(np.float64)
    u, v = pu.copy(), pv.copy()                                   # kinds 0-5: pixel centres, as a producer's points
    sub = (kind >= 6) & (kind <= 8)                               # anywhere inside the grid, and a little around it
    u[sub] = rng.uniform(-1.0, W + 0.5, sub.sum())
    v[sub] = rng.uniform(-1.0, H + 0.5, sub.sum())
    border = kind == 9                                            # u + 0.5 on a cell border of cell_px = 4 (and on 0 and W)
    u[border] = rng.choice(np.arange(0, W + 4, 4), border.sum()).clip(0, W) - 0.5
    vborder = kind == 10
    v[vborder] = rng.choice(np.arange(0, H + 4, 4), vborder.sum()).clip(0, H) - 0.5
    far = kind == 11                                              # well outside the grid
    u[far] = rng.choice([-40.0, -3.0, W + 2.0, 500.0], far.sum())
    same = kind == 12                                             # one crowded pixel with two depths
    u[same], v[same] = 9.0, 6.0
    z[same] = np.where(np.arange(same.sum()) % 3 == 0, 1.0, 2.0)
    xyz = back_project(u, v, z)
    bad = np.nonzero(kind == 13)[0]                               # z = 0, z < 0, NaN, +-Inf
    xyz[bad, 2] = np.resize(np.array([0.0, -1.0, np.nan, np.inf, -0.0, -np.inf]), len(bad))
    nanx = np.nonzero(kind == 14)[0]                              # a finite z with x or y that is not
    xyz[nanx, 0] = np.resize(np.array([np.nan, np.inf, 1e308]), len(nanx))
    big = np.nonzero(kind == 15)[0]                               # u beyond every int
    xyz[big, 1] = np.resize(np.array([1e300, -1e300, 4e9, -4e9]), len(big))
    return xyz


def ulp_points(f32=False):
    """points whose u + 0.5 (v + 0.5) sits on an integer -- 0, a cell border, the last column, `width` itself -- and up to three
    ulps either side of it, by stepping x (y) through its neighbouring values of the stored dtype"""
    T = np.float32 if f32 else np.float64

    def steps_of(c0):
        out = []
        for steps in range(-3, 4):
            c = T(c0)
            for _ in range(abs(steps)):
                c = np.nextafter(c, T(np.inf if steps > 0 else -np.inf))
            out.append(float(c))
        return out

    rows = []
    for k in (0, 1, 4, 8, 36, 37):
        for z in (1.0, 1.5):
            rows += [(x, (5 - K[3]) * z / K[1], z) for x in steps_of((k - 0.5 - K[2]) * z / K[0])]
    for k in (0, 4, 28, 29):
        for z in (1.0, 1.5):
            rows += [((7 - K[2]) * z / K[0], y, z) for y in steps_of((k - 0.5 - K[3]) * z / K[1])]
    return np.array(rows)


def stored(xyz, f32):
    """the points as a problem of the dtype holds them"""
    with np.errstate(all="ignore"):
        return xyz.astype(np.float32).astype(np.float64) if f32 else np.array(xyz, np.float64)


def weights(n, seed):
    """dyadic weights, exact in float32"""
    return np.random.default_rng(1000 + seed).integers(0, 65, n) / 64.0


def param_sets(n):
    """every combination of the GPU test for a point count n, as keyword dicts"""
    out = []
    for cell_px in CELLS:
        for cell_rule in (0, 1):
            for outside in (0, 1):
                for stride, target in STRIDES:
                    out.append(dict(cell_px=cell_px, cell_rule=cell_rule, outside=outside, stride=stride,
                                    target=0 if target is None else target(n)))
    return out
