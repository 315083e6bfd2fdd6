"""Inputs shared by tests/test_point_merge_host.py and tests/test_gpu_point_merge.py: point selection's camera on its 37 x 29 grid
(tests/point_select_cases.py), a DT image with values either side of the edge thresholds, four matrices, src point sets whose
images under the matrix are point selection's point kinds (several per pixel and per cell, on cell borders, equal-z ties,
outside the grid, z <= 0, NaN, Inf), and the case table of the merge: every filter alone and all together on sizes that
straddle the wavefront and workgroup edges of the 256-lane passes."""
import numpy as np

import point_select_cases as pc

H, W, K = pc.H, pc.W, pc.K
SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 2049)


def _rigid():
    q = np.array([0.9, 0.1, -0.2, 0.15])
    q /= np.linalg.norm(q)
    w, x, y, z = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                  [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                  [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = (0.11, -0.07, 0.23)
    return M


def _nonrigid():
    M = np.eye(4)
    M[:3, :3] = [[1.3, 0.2, -0.1], [0.05, 0.8, 0.3], [-0.15, 0.1, 1.1]]     # scale and shear
    M[:3, 3] = (-0.2, 0.1, 0.4)
    return M


def _translation():
    M = np.eye(4)
    M[:3, 3] = (0.3, -0.125, 0.0625)
    return M


MATRICES = dict(rigid=_rigid(), nonrigid=_nonrigid(), identity=np.eye(4), translation=_translation())
# a nearly-identity motion, as between a keyframe and the frame that replaces it
SMALL = np.eye(4)
SMALL[:3, :3] = [[1.0, -0.01, 0.02], [0.01, 1.0, -0.015], [-0.02, 0.015, 1.0]]
SMALL[:3, 3] = (0.03, -0.02, 0.05)


def dt_image(seed=0):
    """H x W doubles exact in float32, in [0, 3): either side of max_dt = 1 and 1.5"""
    return np.random.default_rng(seed).integers(0, 3 * 64, (H, W)).astype(np.float64) / 64.0


def dst_points(n, seed):
    return pc.points(n, 300 + seed)


def src_points(n, seed, M):
    """points whose image under M is one of point selection's kinds (up to the rounding of the inverse)"""
    target = pc.points(n, 500 + seed)
    Minv = np.linalg.inv(M)
    with np.errstate(all="ignore"):
        return target @ Minv[:3, :3].T + Minv[:3, 3]


def special_points():
    """NaN, +-Inf, +-0 and z <= 0 in every coordinate position"""
    vals = (np.nan, np.inf, -np.inf, 0.0, -0.0, -1.0, 1e308, 5e-324)
    rows = [(0.25, -0.5, 2.0)]
    for v in vals:
        rows += [(v, 0.5, 1.5), (0.5, v, 1.5), (0.25, 0.5, v), (v, v, v)]
    return np.array(rows)


FILTERS = (
    dict(),
    dict(require_pixel=1),
    dict(require_pixel=1, margin=3),
    dict(max_dt=1.0),
    dict(cell_px=1),
    dict(cell_px=1, cell_rule=1),
    dict(cell_px=4),
    dict(cell_px=4, cell_rule=1),
    dict(cell_px=64),
    dict(cell_px=64, cell_rule=1),
    dict(max_carried=1),
    dict(max_carried=5),
    dict(max_carried="n"),
    dict(require_pixel=1, margin=3, max_dt=1.5, cell_px=4, cell_rule=1, max_carried=5),
    dict(require_pixel=1, margin=0, max_dt=1.5, cell_px=4, cell_rule=0, max_carried="n"),
    dict(margin=3, max_dt=0.0, cell_px=1),
)
# (dst weighted, src weighted, weight_scale): the four combinations, each with both scales
WEIGHTS = tuple((dw, sw, s) for dw in (False, True) for sw in (False, True) for s in (1.0, 0.5))


def cases():
    """the case table: dicts of name, n_dst, n_src, matrix (name), dst_weighted, src_weighted and params.  Every filter set
    meets every src size; n_dst and the weight combination cycle with the case index so that each is met by each filter"""
    out = []
    k = 0
    for fi, flt in enumerate(FILTERS):
        for si, n_src in enumerate(SIZES):
            n_dst = SIZES[(si * 2 + fi) % len(SIZES)]
            dw, sw, scale = WEIGHTS[k % len(WEIGHTS)]
            prm = dict(flt)
            if prm.get("max_carried") == "n":
                prm["max_carried"] = max(n_src, 1)
            prm["weight_scale"] = scale
            matrix = ("rigid", "nonrigid", "identity", "translation")[k % 4] if n_src % 2 else "small"
            out.append(dict(name="%d-%d" % (fi, si), n_dst=n_dst, n_src=n_src, matrix=matrix, dst_weighted=dw, src_weighted=sw,
                            params=prm, seed=k))
            k += 1
    return out


def matrix(name):
    return SMALL if name == "small" else MATRICES[name]


def build(case, f32):
    """(dst_xyz, dst_w, src_xyz, src_w, M) of a case as a problem of the dtype stores them"""
    M = matrix(case["matrix"])
    dst = pc.stored(dst_points(case["n_dst"], case["seed"]), f32)
    src = pc.stored(src_points(case["n_src"], case["seed"], M), f32)
    dw = pc.weights(case["n_dst"], case["seed"]) if case["dst_weighted"] and case["n_dst"] else None
    sw = pc.weights(case["n_src"], 77 + case["seed"]) if case["src_weighted"] and case["n_src"] else None
    return dst, dw, src, sw, M


# what the argument checks refuse: fields of ea_point_merge, and (entry, value) of a 4 x 4 matrix
BAD_PARAMS = (dict(require_pixel=2), dict(require_pixel=-1), dict(margin=-1), dict(max_dt=float("nan")), dict(cell_px=-1),
              dict(cell_px=4097), dict(cell_rule=2), dict(cell_rule=-1), dict(height=-1, width=-1), dict(height=29), dict(width=37),
              dict(cell_px=1, height=8193, width=8192), dict(max_carried=-1), dict(weight_scale=0.0), dict(weight_scale=-1.0),
              dict(weight_scale=float("inf")), dict(weight_scale=float("nan")))
BAD_MATRICES = tuple((i, v) for i, v in ((12, 1e-300), (13, 1.0), (14, -1.0), (15, 0.0), (15, 2.0), (0, float("nan")), (3, float("inf")),
                                         (11, -float("inf")), (15, float("nan"))))
