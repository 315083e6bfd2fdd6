"""The point selection rule of include/ea_hip.h (ea_*_select_points) restated in numpy: the pixel of a stored point, its cell,
the cell step with both rules and both `outside` policies, the stride step and the argument checks.  Every operation is one
IEEE double operation in the header's order (numpy contracts nothing), so the device and the host shim of
edge_alignment_amd/csrc/ea_point_select.h are held to it bit for bit.

Points come in AS STORED: an fp32 problem's points are the floats it holds, widened to double."""
import numpy as np

CELL_FIRST, CELL_NEAREST = 0, 1
MAX_CELL_PX = 4096
MAX_CELLS = 1 << 26
STAT_KEYS = ("n_before", "no_pixel", "after_cells", "n_after", "stride_used")


def params_ok(cell_px=0, cell_rule=0, outside=0, height=0, width=0, stride=1, target=0):
    if cell_px < 0 or cell_px > MAX_CELL_PX:
        return False
    if cell_rule not in (CELL_FIRST, CELL_NEAREST) or outside not in (0, 1):
        return False
    if stride < 1 or target < 0 or (stride > 1 and target > 0):
        return False
    if height < 0 or width < 0 or (height == 0) != (width == 0):
        return False
    if cell_px > 0 and height > 0 and cells(cell_px, height, width) > MAX_CELLS:
        return False
    return True


def cells(cell_px, height, width):
    return -(-width // cell_px) * -(-height // cell_px)


def pixel(xyz, K, height, width):
    """(has, pu, pv, u, v): has-pixel flags, the pixel (int64, -1 where there is none) and the doubles u, v"""
    fx, fy, cx, cy = (np.float64(k) for k in K)
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    with np.errstate(all="ignore"):
        a = x / z
        b = y / z
        u = fx * a
        u = u + cx
        v = fy * b
        v = v + cy
        pu = np.floor(u + 0.5)
        pv = np.floor(v + 0.5)
        has = (z > 0.0) & np.isfinite(u) & np.isfinite(v) & (pu >= 0.0) & (pu < float(width)) & (pv >= 0.0) & (pv < float(height))
    ipu = np.where(has, pu, -1.0).astype(np.int64)
    ipv = np.where(has, pv, -1.0).astype(np.int64)
    return has, ipu, ipv, u, v


def cell_of(pu, pv, cell_px, width):
    return (pv // cell_px) * (-(-width // cell_px)) + pu // cell_px


def stride_used(m, stride=1, target=0):
    if target > 0:
        return m // target if m > target else 1
    return stride


def select(xyz, K=None, height=0, width=0, cell_px=0, cell_rule=CELL_FIRST, outside=0, stride=1, target=0):
    """(kept indices in point order, stats dict) of the rule on the stored points xyz (n x 3)"""
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    n = len(xyz)
    if n == 0:
        return np.zeros(0, np.int64), dict(n_before=0, no_pixel=0, after_cells=0, n_after=0, stride_used=1)
    no_pixel = 0
    if cell_px > 0:
        has, pu, pv, _, _ = pixel(xyz, K, height, width)
        no_pixel = int((~has).sum())
        idx = np.nonzero(has)[0]
        cell = cell_of(pu[idx], pv[idx], cell_px, width)
        if cell_rule == CELL_NEAREST:
            zbits = np.ascontiguousarray(xyz[idx, 2]).view(np.uint64)      # positive doubles order like their bit patterns
            order = np.lexsort((idx, zbits, cell))                         # by cell, then z, then index
        else:
            order = np.lexsort((idx, cell))
        sorted_cell = cell[order]
        first = np.ones(len(order), bool)
        first[1:] = sorted_cell[1:] != sorted_cell[:-1]
        flag = np.zeros(n, bool)
        flag[idx[order[first]]] = True
        if outside:
            flag |= ~has
        survivors = np.nonzero(flag)[0]
    else:
        survivors = np.arange(n)
    m = len(survivors)
    s = stride_used(m, stride, target)
    kept = survivors[::s]
    assert len(kept) == -(-m // s)
    return kept.astype(np.int64), dict(n_before=n, no_pixel=no_pixel, after_cells=m, n_after=len(kept), stride_used=int(s))
