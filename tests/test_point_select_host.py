"""edge_alignment_amd/csrc/ea_point_select.h -- the pixel of a stored point, the has-pixel rule, the cell, the stride the
survivors are thinned with and the argument checks -- built with the host compiler (-ffp-contract=off, as the other host
shims) and held to tests/point_select_ref.py exactly, on both stored dtypes, over the inputs of the GPU test
(tests/point_select_cases.py), with points whose u + 0.5 sits within an ulp or two of an integer and of `width`, and with
z = 0, z < 0, NaN and Inf.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import point_select_cases as pc
import point_select_ref as ps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = C.c_int64


@pytest.fixture(scope="module")
def shim():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "point_select_host.so")
    src = os.path.join(ROOT, "tests", "point_select_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_point_select.h"), os.path.join(csrc, "ea_reproject.h"), os.path.join(ROOT, "include", "ea_hip.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I", csrc,
                               "-o", so, src])
    lib = C.CDLL(so)
    lib.point_select_pixels_c.argtypes = [C.c_void_p, I64] + [C.c_double] * 4 + [C.c_int] * 3 + [C.c_void_p] * 4
    lib.point_select_pixels_c.restype = None
    for fn, args in ((lib.point_select_stride_used_c, [I64] * 3), (lib.point_select_count_after_c, [I64] * 2),
                     (lib.point_selection_cells_c, [C.c_int] * 3)):
        fn.argtypes, fn.restype = args, I64
    lib.point_selection_ok_c.argtypes = [C.c_int] * 5 + [I64] * 2
    lib.point_selection_is_identity_c.argtypes = [C.c_int, I64, I64]
    return lib


def _pixels(shim, xyz, cell_px, K=pc.K, height=pc.H, width=pc.W):
    xyz = np.ascontiguousarray(xyz, np.float64)
    n = len(xyz)
    has, pu, pv = (np.full(n, -9, np.int32) for _ in range(3))
    cell = np.full(n, -9, np.int64)
    shim.point_select_pixels_c(xyz.ctypes.data, n, *K, height, width, cell_px, has.ctypes.data, pu.ctypes.data, pv.ctypes.data,
                               cell.ctypes.data)
    return has.astype(bool), pu, pv, cell


def _check(shim, xyz, cell_px, **kw):
    has, pu, pv, cell = _pixels(shim, xyz, cell_px, **kw)
    K, height, width = kw.get("K", pc.K), kw.get("height", pc.H), kw.get("width", pc.W)
    w_has, w_pu, w_pv, _, _ = ps.pixel(xyz, K, height, width)
    assert np.array_equal(has, w_has) and np.array_equal(pu, w_pu) and np.array_equal(pv, w_pv)
    if cell_px > 0:
        want = np.where(w_has, ps.cell_of(w_pu, w_pv, cell_px, width), 0)
        assert np.array_equal(cell, want)
        assert cell[has].max(initial=0) < ps.cells(cell_px, height, width)
    return has, pu, pv


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_pixel_has_pixel_and_cell_are_the_restatement(shim, f32):
    seen_has = seen_none = 0
    for n in pc.SIZES:
        xyz = pc.stored(pc.points(n, 100 + n), f32)
        for cell_px in pc.CELLS:
            has, pu, pv = _check(shim, xyz, cell_px)
            seen_has += int(has.sum())
            seen_none += int((~has).sum())
    assert seen_has > 0 and seen_none > 0
    xyz = pc.points(2049, 2149)
    kind = np.arange(2049) % 16
    has, pu, pv = _check(shim, pc.stored(xyz, f32), 4)
    assert has[kind < 6].all()                                  # a producer's point lands on the pixel it came from
    assert not has[kind == 14].any() and not has[kind == 15].any() and not has[kind == 11].any()
    # z = 0, -0, < 0, NaN, -Inf: no pixel; z = +Inf is > 0 with finite u, v -- the principal point's pixel, as the rule says
    assert np.array_equal(has[kind == 13], xyz[kind == 13, 2] == np.inf) and has[kind == 13].any()
    assert 0 < has[kind == 9].sum() < (kind == 9).sum()         # on the borders: some on the grid, some past it


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_within_an_ulp_of_an_integer_and_of_width(shim, f32):
    """stepping x through neighbouring doubles moves u + 0.5 across the integer: both sides are seen, at 0 and `width` the
    has-pixel flag flips with it, and shim and restatement agree on every one"""
    xyz = pc.stored(pc.ulp_points(f32), f32)
    has, pu, pv = _check(shim, xyz, 4)
    _, _, _, u, v = ps.pixel(xyz, pc.K, pc.H, pc.W)
    for k in (0, 4, 36, 37):
        near = np.abs(u + 0.5 - k) < 1e-3
        assert near.any()
        below, above = near & (np.floor(u + 0.5) == k - 1), near & (np.floor(u + 0.5) == k)
        assert below.any() and above.any(), k
        if k == 0:
            assert not has[below].any() and has[above].all()
        if k == 37:
            assert has[below].all() and not has[above].any()
    if not f32:                                                 # doubles: u + 0.5 also hits an integer itself
        assert (u + 0.5 == np.round(u + 0.5)).any()
    for k in (0, 29):
        near = np.abs(v + 0.5 - k) < 1e-3
        assert (near & (np.floor(v + 0.5) == k - 1)).any() and (near & (np.floor(v + 0.5) == k)).any(), k


def test_degenerate_depths_have_no_pixel(shim):
    xyz = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, -0.0], [0.1, 0.1, -1.0], [0.0, 0.0, np.nan], [0.0, 0.0, np.inf], [0.0, 0.0, -np.inf],
                    [np.nan, 0.0, 1.0], [0.0, np.inf, 1.0], [0.0, 0.0, 1.0], [1e308, 0.0, 1.0], [0.0, 0.0, 5e-324]])
    has, pu, pv = _check(shim, xyz, 1)
    # +Inf depth projects every finite x, y onto the principal point: z > 0 and u, v finite -- it has a pixel, as the rule says
    assert has.tolist() == [False, False, False, False, True, False, False, False, True, False, True]
    assert (pu[8], pv[8]) == (17, 14) == (pu[4], pv[4])         # floor(17.3 + 0.5), floor(13.6 + 0.5)
    # comparisons happen in double: a pixel far beyond INT_MAX is simply outside
    _check(shim, np.array([[1e30, 0.0, 1.0], [-1e30, 0.0, 1.0], [0.0, 3e9, 1.0]]), 4, K=(1.0, 1.0, 0.0, 0.0))
    # the largest extent a call can name
    big = dict(K=(1.0, 1.0, 0.0, 0.0), height=3, width=2 ** 31 - 1)
    has, pu, pv = _check(shim, np.array([[2.0 ** 31 - 2, 2.0, 1.0], [2.0 ** 31 - 1, 2.0, 1.0], [5.0, 3.0, 1.0]]), 4096, **big)
    assert has.tolist() == [True, False, False] and pu[0] == 2 ** 31 - 2


def test_stride_used_and_count(shim):
    for m in (0, 1, 4, 5, 6, 9, 10, 11, 199, 200, 201, 399, 400, 44457, 2 ** 31 - 257):
        for stride, target in ((1, 0), (2, 0), (30, 0), (2 ** 40, 0), (1, 1), (1, 5), (1, 200), (1, m), (1, m + 1), (1, 2 ** 40)):
            s = shim.point_select_stride_used_c(m, stride, target)
            assert s == ps.stride_used(m, stride, target) >= 1, (m, stride, target)
            assert shim.point_select_count_after_c(m, s) == len(range(0, m, s))
    assert shim.point_select_stride_used_c(44457, 30, 0) == 30 and shim.point_select_count_after_c(44457, 30) == 1482
    assert shim.point_select_stride_used_c(1000, 1, 300) == 3          # the reference's iterStep = N / minNumOfPointsPerimage


def test_argument_checks(shim):
    ok = dict(cell_px=4, cell_rule=0, outside=0, height=0, width=0, stride=1, target=0)

    def both(**over):
        a = dict(ok, **over)
        got = shim.point_selection_ok_c(a["cell_px"], a["cell_rule"], a["outside"], a["height"], a["width"], a["stride"], a["target"])
        assert got == int(ps.params_ok(**a)), a
        return got

    assert both() == 1 and both(cell_px=0) == 1 and both(cell_px=4096) == 1 and both(cell_rule=1, outside=1) == 1
    assert both(stride=30) == 1 and both(target=200) == 1 and both(height=29, width=37) == 1 and both(stride=2 ** 40) == 1
    for bad in (dict(cell_px=-1), dict(cell_px=4097), dict(cell_rule=2), dict(cell_rule=-1), dict(outside=2), dict(outside=-1),
                dict(stride=0), dict(stride=-3), dict(target=-1), dict(stride=2, target=5), dict(height=-1, width=-1),
                dict(height=-1, width=5), dict(height=29, width=0), dict(height=0, width=37),
                dict(cell_px=1, height=8193, width=8192), dict(cell_px=2, height=2 ** 30, width=2 ** 30)):
        assert both(**bad) == 0, bad
    assert both(cell_px=1, height=8192, width=8192) == 1              # exactly 2^26 cells
    assert both(cell_px=0, height=2 ** 30, width=2 ** 30) == 1        # no cell step: no cells
    for cell_px, h, w in ((1, 29, 37), (4, 29, 37), (64, 29, 37), (4096, 3, 2 ** 31 - 1), (3, 480, 640)):
        assert shim.point_selection_cells_c(cell_px, h, w) == ps.cells(cell_px, h, w)
    assert ps.cells(4, 29, 37) == 10 * 8 and ps.cells(64, 29, 37) == 1
    assert shim.point_selection_is_identity_c(0, 1, 0) == 1
    assert not any(shim.point_selection_is_identity_c(*a) for a in ((1, 1, 0), (0, 2, 0), (0, 1, 1)))
    assert shim.point_select_seg_bytes_c() % 8 == 0 and shim.point_select_out_bytes_c() == 16


def test_the_restatement_on_a_case_worked_by_hand():
    """3 x 4 grid, unit camera: cells of 2 px; FIRST keeps the lowest index per cell, NEAREST the smallest z with ties by index"""
    K = (1.0, 1.0, 0.0, 0.0)
    uvz = [(0, 0, 2.0), (1, 1, 1.0), (1, 0, 1.0), (3, 2, 1.0), (2, 2, 1.0), (9, 9, 1.0), (0, 0, -1.0), (2, 0, 3.0)]
    xyz = np.array([(u * z, v * z, z) for u, v, z in uvz])
    kept, st = ps.select(xyz, K, 3, 4, cell_px=2)
    assert kept.tolist() == [0, 3, 7] and st == dict(n_before=8, no_pixel=2, after_cells=3, n_after=3, stride_used=1)
    kept, st = ps.select(xyz, K, 3, 4, cell_px=2, cell_rule=1)
    assert kept.tolist() == [1, 3, 7]
    kept, st = ps.select(xyz, K, 3, 4, cell_px=2, cell_rule=1, outside=1, stride=2)
    assert kept.tolist() == [1, 5, 7] and st == dict(n_before=8, no_pixel=2, after_cells=5, n_after=3, stride_used=2)
    kept, st = ps.select(xyz, K, 3, 4, cell_px=0, target=3)
    assert kept.tolist() == [0, 2, 4, 6] and st["stride_used"] == 2 and st["no_pixel"] == 0
    kept, st = ps.select(xyz, K, 3, 4, cell_px=0, target=8)
    assert kept.tolist() == list(range(8)) and st["stride_used"] == 1
