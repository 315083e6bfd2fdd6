"""edge_alignment_amd/csrc/ea_point_merge.h -- the transform of a stored point, the pixel and margin test of a carried point, the
carried weight, the cap and the argument checks -- built with the host compiler (-ffp-contract=off, as the other host shims) and
held to tests/point_merge_ref.py exactly, on both stored dtypes, over the inputs of the GPU test (tests/point_merge_cases.py)
and over points with NaN, +-Inf, +-0 and z <= 0.  The case table itself is held to account: each of no_pixel, off_edge, occupied,
lost_cell, capped and carried is non-zero in some case and zero in another, computed from the restatement alone.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import point_merge_cases as mc
import point_merge_ref as pm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64 = C.c_int64


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def shim():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "point_merge_host.so")
    src = os.path.join(ROOT, "tests", "point_merge_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(ROOT, "include", "ea_hip.h")] + [os.path.join(csrc, h) for h in
                                                               ("ea_point_merge.h", "ea_point_select.h", "ea_reproject.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I", csrc,
                               "-o", so, src])
    lib = C.CDLL(so)
    lib.point_merge_transform_c.argtypes = [C.c_void_p, I64, C.c_void_p, C.c_int, C.c_void_p]
    lib.point_merge_transform_c.restype = None
    lib.point_merge_pixels_c.argtypes = [C.c_void_p, I64] + [C.c_double] * 4 + [C.c_int] * 3 + [C.c_void_p] * 3
    lib.point_merge_pixels_c.restype = None
    lib.point_merge_weights_c.argtypes = [C.c_void_p, I64, C.c_double, C.c_int, C.c_void_p]
    lib.point_merge_weights_c.restype = None
    lib.point_merge_carried_c.argtypes, lib.point_merge_carried_c.restype = [I64, I64], I64
    lib.point_merge_weighted_c.argtypes = [C.c_int, C.c_int, C.c_double]
    lib.point_transform_ok_c.argtypes = [C.c_void_p]
    lib.point_merge_ok_c.argtypes = [C.c_int, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, I64, C.c_double]
    lib.point_merge_needs_pixel_c.argtypes = [C.c_int, C.c_double, C.c_int]
    return lib


def _transform(shim, xyz, M, f32):
    xyz, M = np.ascontiguousarray(xyz, np.float64), np.ascontiguousarray(M, np.float64)
    out = np.full_like(xyz, -9.0)
    shim.point_merge_transform_c(xyz.ctypes.data, len(xyz), M.ctypes.data, int(f32), out.ctypes.data)
    return out


def _pixels(shim, xyz, margin, height=mc.H, width=mc.W):
    xyz = np.ascontiguousarray(xyz, np.float64)
    has, pu, pv = (np.full(len(xyz), -9, np.int32) for _ in range(3))
    shim.point_merge_pixels_c(xyz.ctypes.data, len(xyz), *mc.K, height, width, margin, has.ctypes.data, pu.ctypes.data, pv.ctypes.data)
    return has.astype(bool), pu, pv


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_the_transform_is_the_restatement(shim, f32):
    for name, M in list(mc.MATRICES.items()) + [("small", mc.SMALL)]:
        for xyz in (mc.special_points(), mc.src_points(2049, 3, M), mc.dst_points(257, 4)):
            xyz = mc.pc.stored(xyz, f32)
            got, want = _transform(shim, xyz, M, f32), pm.transform(xyz, M, f32)
            assert np.array_equal(_bits(got), _bits(want)), name
            # two chained transforms round twice: the restatement's chain, which the product matrix does not give
            again = _transform(shim, got, mc.MATRICES["nonrigid"], f32)
            assert np.array_equal(_bits(again), _bits(pm.transform(want, mc.MATRICES["nonrigid"], f32))), name
    xyz = mc.pc.stored(mc.src_points(2049, 3, mc.MATRICES["rigid"]), f32)
    chain = pm.transform(pm.transform(xyz, mc.MATRICES["rigid"], f32), mc.MATRICES["nonrigid"], f32)
    product = pm.transform(xyz, mc.MATRICES["nonrigid"] @ mc.MATRICES["rigid"], f32)
    assert not np.array_equal(_bits(chain), _bits(product))
    # the identity and IEEE: x + 0 y + 0 z + 0 keeps finite values; NaN and Inf come out as IEEE has them
    sp = mc.pc.stored(mc.special_points(), f32)
    ident = pm.transform(sp, np.eye(4), f32)
    finite = np.isfinite(sp).all(axis=1)
    assert np.array_equal(ident[finite], sp[finite]) and np.isnan(ident[~finite]).any()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_the_pixel_and_margin_test_is_the_restatement(shim, f32):
    seen_in = seen_margin = seen_out = 0
    for n in mc.SIZES:
        moved = pm.transform(mc.pc.stored(mc.src_points(n, n, mc.SMALL), f32), mc.SMALL, f32)
        for margin in (0, 3, 14, 15, 40):
            has, pu, pv = _pixels(shim, moved, margin)
            w_has, w_pu, w_pv, _, _ = pm.ps.pixel(moved, mc.K, mc.H, mc.W)
            inside = (w_pu >= margin) & (w_pu < mc.W - margin) & (w_pv >= margin) & (w_pv < mc.H - margin)
            assert np.array_equal(has, w_has & inside), (n, margin)
            assert np.array_equal(pu[has], w_pu[has]) and np.array_equal(pv[has], w_pv[has])
            seen_in += int(has.sum())
            seen_margin += int((w_has & ~inside).sum())
            seen_out += int((~w_has).sum())
            if margin >= 15:                                    # 29 rows: no pixel is 15 inside
                assert not has.any()
    assert seen_in > 0 and seen_margin > 0 and seen_out > 0


def test_weights_cap_and_flags(shim):
    w = np.concatenate([mc.pc.weights(300, 1), [0.0, 1.0, 1e-300, 1e300, np.inf, np.nan, 1.0 / 3.0]])
    for scale in (1.0, 0.5, 1.0 / 3.0, 3.0, 1e-30):
        for f32 in (False, True):
            out = np.full_like(w, -9.0)
            shim.point_merge_weights_c(w.ctypes.data, len(w), scale, int(f32), out.ctypes.data)
            with np.errstate(all="ignore"):
                assert np.array_equal(_bits(out), _bits(pm.rounded(w * np.float64(scale), f32))), (scale, f32)
    for m in (0, 1, 4, 5, 6, 2049, 2 ** 31 - 1):
        for cap in (0, 1, 5, m, m + 1, 2 ** 40):
            assert shim.point_merge_carried_c(m, cap) == (min(m, cap) if cap > 0 else m)
    for dw in (0, 1):
        for sw in (0, 1):
            for scale in (1.0, 0.5):
                assert shim.point_merge_weighted_c(dw, sw, scale) == int(bool(dw or sw or scale != 1.0))
    assert shim.point_merge_needs_pixel_c(0, -1.0, 0) == 0
    assert all(shim.point_merge_needs_pixel_c(*a) == 1 for a in ((1, -1.0, 0), (0, 0.0, 0), (0, -1.0, 4)))
    assert shim.point_merge_seg_bytes_c() % 8 == 0 and shim.point_transform_seg_bytes_c() % 8 == 0
    assert shim.point_merge_out_bytes_c() == 32


def test_argument_checks(shim):
    def both(**over):
        a = dict(pm.DEFAULTS, **over)
        got = shim.point_merge_ok_c(a["require_pixel"], a["margin"], a["max_dt"], a["cell_px"], a["cell_rule"], a["height"], a["width"],
                                    a["max_carried"], a["weight_scale"])
        assert got == int(pm.params_ok(**a)), a
        return got

    assert both() == 1 and both(max_dt=-5.0) == 1 and both(max_dt=0.0) == 1 and both(max_dt=float("inf")) == 1
    assert both(require_pixel=1, margin=3, max_dt=1.5, cell_px=4096, cell_rule=1, height=29, width=37, max_carried=2 ** 40, weight_scale=0.5) == 1
    assert both(cell_px=1, height=8192, width=8192) == 1              # exactly 2^26 cells
    for bad in mc.BAD_PARAMS:
        assert both(**bad) == 0, bad
    for name, M in mc.MATRICES.items():
        assert shim.point_transform_ok_c(np.ascontiguousarray(M).ctypes.data) == 1 == int(pm.matrix_ok(M)), name
    for i, v in mc.BAD_MATRICES:
        M = np.ascontiguousarray(mc.MATRICES["rigid"]).copy().reshape(16)
        M[i] = v
        assert shim.point_transform_ok_c(M.ctypes.data) == 0 == int(pm.matrix_ok(M)), (i, v)


def test_the_case_table_is_not_vacuous():
    """from the restatement alone: every counter is non-zero in some case and zero in another, on both dtypes; every filter,
    weight combination, matrix and size is met"""
    table = mc.cases()
    dt = mc.dt_image()
    for f32 in (False, True):
        nonzero, zero = set(), set()
        weighted_out = set()
        for case in table:
            dst, dw, src, sw, M = mc.build(case, f32)
            pts, w, st, kept = pm.merge(dst, dw, src, sw, M, mc.K, dt, f32, **case["params"])
            assert len(pts) == st["n_after"] == case["n_dst"] + st["carried"]
            assert np.array_equal(_bits(pts[:case["n_dst"]]), _bits(dst))
            weighted_out.add(w is not None)
            for key in ("no_pixel", "off_edge", "occupied", "lost_cell", "capped", "carried"):
                if case["n_src"] > 1:
                    (nonzero if st[key] > 0 else zero).add(key)
        want = {"no_pixel", "off_edge", "occupied", "lost_cell", "capped", "carried"}
        assert nonzero == want and zero == want, (f32, want - nonzero, want - zero)
        assert weighted_out == {False, True}
    assert {c["n_src"] for c in table} == set(mc.SIZES) == {c["n_dst"] for c in table}
    assert {(c["dst_weighted"], c["src_weighted"], c["params"]["weight_scale"]) for c in table} == set(mc.WEIGHTS)
    assert {c["matrix"] for c in table} == {"rigid", "nonrigid", "identity", "translation", "small"}
    assert {c["params"].get("cell_px", 0) for c in table} == {0, 1, 4, 64}
    assert {c["params"].get("margin", 0) for c in table} == {0, 3}


def test_the_restatement_on_a_case_worked_by_hand():
    """4 x 3 grid, unit camera, cells of 2 px, a translation by (0, 0, 1): dst occupies cell 0; of the src points two share the
    free cell 1 (FIRST the lower index, NEAREST the smaller z'), one falls on the occupied cell, one has no pixel, one is off
    the edges"""
    Kc = (1.0, 1.0, 0.0, 0.0)
    dt = np.zeros((3, 4))
    dt[2, 3] = 9.0
    M = np.eye(4)
    M[2, 3] = 1.0
    dst = np.array([(0.0, 0.0, 1.0)])
    uvz = [(2, 0, 3.0), (3, 1, 2.0), (1, 1, 2.0), (9, 9, 2.0), (3, 2, 2.0), (0, 2, 2.0)]       # (pu, pv, z') after the move
    src = np.array([(u * z, v * z, z - 1.0) for u, v, z in uvz])
    pts, w, st, kept = pm.merge(dst, None, src, None, M, Kc, dt, cell_px=2, max_dt=1.0)
    assert kept.tolist() == [0, 5]
    assert st == dict(n_dst=1, n_src=6, no_pixel=1, off_edge=1, occupied=1, lost_cell=1, capped=0, carried=2, n_after=3) and w is None
    pts, w, st, kept = pm.merge(dst, None, src, np.arange(6) / 4.0, M, Kc, dt, cell_px=2, cell_rule=1, max_dt=1.0, max_carried=1,
                                weight_scale=0.5)
    assert kept.tolist() == [1] and st["capped"] == 1 and st["carried"] == 1
    assert w.tolist() == [1.0, 0.125] and np.array_equal(pts[1], (6.0, 2.0, 2.0))
    pts, w, st, kept = pm.merge(np.zeros((0, 3)), None, src, None, M)                        # a_X2 = T * a_X
    assert st["carried"] == 6 and np.array_equal(_bits(pts), _bits(pm.transform(src, M)))
