"""The rules of include/ea_hip.h for ea_*_transform_points and ea_*_merge_points restated in numpy: the transform of a stored
point, the pixel and margin test, the edge test on the stored DT image, the cell step against the cells dst occupies, the cap,
the weights and the argument checks.  Every operation is one IEEE double operation in the header's order (numpy contracts
nothing), so the device and the host shim of edge_alignment_amd/csrc/ea_point_merge.h are held to it bit for bit.

Points, weights and the DT image come in AS STORED: an fp32 problem's values are the floats it holds, widened to double."""
import numpy as np

import point_select_ref as ps

STAT_KEYS = ("n_dst", "n_src", "no_pixel", "off_edge", "occupied", "lost_cell", "capped", "carried", "n_after")
DEFAULTS = dict(require_pixel=0, margin=0, max_dt=-1.0, cell_px=0, cell_rule=0, height=0, width=0, max_carried=0, weight_scale=1.0)


def matrix_ok(M):
    M = np.asarray(M, np.float64).reshape(16)
    return bool(np.isfinite(M[:12]).all() and M[12] == 0.0 and M[13] == 0.0 and M[14] == 0.0 and M[15] == 1.0)


def params_ok(**over):
    p = dict(DEFAULTS, **over)
    if p["require_pixel"] not in (0, 1) or p["margin"] < 0 or np.isnan(p["max_dt"]):
        return False
    if p["cell_px"] < 0 or p["cell_px"] > ps.MAX_CELL_PX or p["cell_rule"] not in (0, 1):
        return False
    if p["height"] < 0 or p["width"] < 0 or (p["height"] == 0) != (p["width"] == 0):
        return False
    if p["cell_px"] > 0 and p["height"] > 0 and ps.cells(p["cell_px"], p["height"], p["width"]) > ps.MAX_CELLS:
        return False
    if p["max_carried"] < 0 or not (p["weight_scale"] > 0.0 and np.isfinite(p["weight_scale"])):
        return False
    return True


def rounded(a, f32):
    """one rounding to the problem dtype, widened again"""
    with np.errstate(all="ignore"):
        return a.astype(np.float32).astype(np.float64) if f32 else np.array(a, np.float64)


def transform(xyz, M, f32=False):
    """x' = ((M00 x + M01 y) + M02 z) + M03 and alike, each rounded once to the dtype: n x 3 doubles as the problem stores them"""
    M = np.asarray(M, np.float64).reshape(4, 4)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    out = np.empty_like(xyz)
    with np.errstate(all="ignore"):
        for r in range(3):
            a = M[r, 0] * x
            b = M[r, 1] * y
            c = M[r, 2] * z
            out[:, r] = ((a + b) + c) + M[r, 3]
    return rounded(out, f32)


def merge(dst_xyz, dst_w, src_xyz, src_w, M, K=None, dt=None, f32=False, **over):
    """(points [n_after x 3], weights or None, stats dict, carried src indices) of the merge rule.  dst_w / src_w: None for an
    unweighted side.  dt: dst's DT image [H x W] as stored (doubles); height / width 0: its extent."""
    p = dict(DEFAULTS, **over)
    dst_xyz = np.asarray(dst_xyz, np.float64).reshape(-1, 3)
    src_xyz = np.asarray(src_xyz, np.float64).reshape(-1, 3)
    n_dst, n_src = len(dst_xyz), len(src_xyz)
    st = dict.fromkeys(STAT_KEYS, 0)
    st.update(n_dst=n_dst, n_src=n_src, n_after=n_dst)
    if n_src == 0:
        return dst_xyz, dst_w, st, np.zeros(0, np.int64)
    moved = transform(src_xyz, M, f32)                                    # step 1
    alive = np.ones(n_src, bool)
    need_pixel = p["require_pixel"] or p["max_dt"] >= 0 or p["cell_px"] > 0
    if need_pixel:
        H, W = (p["height"], p["width"]) if p["height"] > 0 else dt.shape
        has, pu, pv, _, _ = ps.pixel(moved, K, H, W)                      # step 2
        m = p["margin"]
        has &= (pu >= m) & (pu < W - m) & (pv >= m) & (pv < H - m)
        st["no_pixel"] = int((~has).sum())
        alive &= has
        if p["max_dt"] >= 0:                                              # step 3
            idx = np.nonzero(alive)[0]
            with np.errstate(invalid="ignore"):
                on = np.asarray(dt, np.float64)[pv[idx], pu[idx]] <= p["max_dt"]
            st["off_edge"] = int((~on).sum())
            alive[idx[~on]] = False
        if p["cell_px"] > 0:                                              # step 4
            c = p["cell_px"]
            d_has, d_pu, d_pv, _, _ = ps.pixel(dst_xyz, K, H, W)
            taken = np.zeros(ps.cells(c, H, W), bool)
            taken[ps.cell_of(d_pu[d_has], d_pv[d_has], c, W)] = True
            idx = np.nonzero(alive)[0]
            cell = ps.cell_of(pu[idx], pv[idx], c, W)
            occ = taken[cell]
            st["occupied"] = int(occ.sum())
            alive[idx[occ]] = False
            idx, cell = idx[~occ], cell[~occ]
            if p["cell_rule"] == 1:
                zbits = np.ascontiguousarray(moved[idx, 2]).view(np.uint64)
                order = np.lexsort((idx, zbits, cell))
            else:
                order = np.lexsort((idx, cell))
            sc = cell[order]
            first = np.ones(len(order), bool)
            first[1:] = sc[1:] != sc[:-1]
            win = np.zeros(n_src, bool)
            win[idx[order[first]]] = True
            st["lost_cell"] = int(len(idx) - first.sum())
            alive &= win
    survivors = np.nonzero(alive)[0]
    cap = p["max_carried"]
    kept = survivors[:cap] if cap > 0 else survivors                     # step 5
    st["capped"] = len(survivors) - len(kept)
    st["carried"] = len(kept)
    st["n_after"] = n_dst + len(kept)
    assert n_src == sum(st[k] for k in ("no_pixel", "off_edge", "occupied", "lost_cell", "capped", "carried"))
    if len(kept) == 0:
        return dst_xyz, dst_w, st, kept
    pts = np.concatenate([dst_xyz, moved[kept]])
    w = None
    if dst_w is not None or src_w is not None or p["weight_scale"] != 1.0:
        own = np.ones(n_dst) if dst_w is None else np.asarray(dst_w, np.float64)
        from_src = np.ones(n_src) if src_w is None else np.asarray(src_w, np.float64)
        w = np.concatenate([own, rounded(from_src[kept] * np.float64(p["weight_scale"]), f32)])
    return pts, w, st, kept
