"""edge_alignment_amd/csrc/ea_depth_gate.h -- sample validity and conversion for both depth kinds, the projection, the window
scan with its tie rule, the classification, the factor and the weight formula, and the argument checks -- built with the host
compiler (-ffp-contract=off, as the other host shims) and held to tests/depth_gate_ref.py: class bytes equal byte for byte
and weights bit for bit, for both depth kinds, radius 0..3, with and without the depth-weighting factor (power 1 and 3), on
the inputs of the GPU test (tests/depth_gate_cases.py).  The shim reads points, matrix and depth image from a file.  No device."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np
import pytest

import depth_gate_cases as dc
import depth_gate_ref as dg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "depth_gate_host.so")
    src = os.path.join(ROOT, "tests", "depth_gate_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_depth_gate.h"), os.path.join(csrc, "ea_reproject.h"), os.path.join(ROOT, "include", "ea_hip.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I", csrc,
                               "-o", so, src])
    lib = C.CDLL(so)
    lib.depth_gate_file_c.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_int]
    lib.depth_gate_params_ok_c.argtypes = [C.c_int] + [C.c_double] * 5
    lib.depth_gate_factors_fit_float_c.argtypes = [C.c_double] * 3
    lib.now_depth_args_ok_c.argtypes = [C.c_int, C.c_int, C.c_int, C.c_double]
    assert lib.depth_gate_header_bytes_c() == 256
    return lib


def _run(shim, path, xyz, M, im, depth, radius, dist, f32, dw, prm):
    kind = 0 if depth.dtype == np.uint16 else 1
    z_ref, power = dw if dw else (1.0, 0)
    with open(path, "wb") as f:
        f.write(struct.pack("<8i", len(xyz), im["H"], im["W"], kind, radius, int(dist is not None), int(f32), power))
        f.write(np.asarray(M, np.float64).reshape(12).tobytes())
        f.write(struct.pack("<4d", *im["K"]))
        f.write(struct.pack("<5d", *(dist if dist is not None else (0.0,) * 5)))
        f.write(struct.pack("<7d", dc.Z_SCALING, prm["abs_tol"], prm["rel_tol"], prm["w_occluded"], prm["w_free"], prm["w_unknown"], z_ref))
        f.write(np.ascontiguousarray(xyz[:, :3], np.float64).tobytes())
        f.write(np.ascontiguousarray(depth).tobytes())
    cls, w = np.full(len(xyz), 99, np.uint8), np.full(len(xyz), -7.0)
    assert shim.depth_gate_file_c(path.encode(), cls.ctypes.data, w.ctypes.data, len(xyz)) == 0
    return cls, w


def _stored(xyz, f32):
    """the points as a problem of the dtype holds them"""
    return xyz.astype(np.float32).astype(np.float64) if f32 else xyz


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_classes_and_weights_are_the_restatement(shim, tmp_path, kind, f32):
    path = str(tmp_path / "case.bin")
    prm = dict(w_occluded=0.125, w_free=0.3, w_unknown=0.7, **dc.TOL)
    seen = np.zeros(6, np.int64)
    saw_tie = saw_boundary = saw_ulp_occluded = saw_ulp_free = 0
    for im, sizes in ((dc.SMALL, dc.SIZES), (dc.BIG, (513,))):
        depth = dc.depth_image(im, kind)
        for n in sizes:
            xyz = _stored(dc.points(n, 100 + n, im, f32), f32)
            for variant, (use_dist, _) in dc.VARIANTS.items():
                dist = dc.DIST if use_dist else None
                for name, T in dc.MATRICES.items():
                    M = dc.matrix_for(variant, T)
                    for radius in range(4):
                        want, det = dg.classify(xyz, M, im["K"], depth, dc.Z_SCALING, radius, dist=dist, details=True, **dc.TOL)
                        for dw in (None, (1.0, 1), (1.25, 3)):
                            got, w = _run(shim, path, xyz, M, im, depth, radius, dist, f32, dw, prm)
                            assert np.array_equal(got, want), (kind, f32, n, variant, name, radius)
                            ww = dg.weights(want, xyz[:, 2], prm["w_occluded"], prm["w_free"], prm["w_unknown"], dw, f32)
                            assert np.array_equal(w.view(np.uint64), ww.view(np.uint64)), (kind, f32, n, variant, name, radius, dw)
                        seen += np.bincount(want, minlength=6)
                        if name == "identity" and variant == "plain":
                            on = det["have"]
                            saw_tie += int(det["tie"].sum())
                            saw_boundary += int((on & (np.abs(det["diff"]) == det["tol"]) & (want == dg.CONSISTENT)).sum())
                            beyond = on & (np.abs(det["diff"]) > det["tol"]) & (np.abs(det["diff"]) - det["tol"] < 2.0 ** -20)
                            saw_ulp_occluded += int((beyond & (want == dg.OCCLUDED)).sum())
                            saw_ulp_free += int((beyond & (want == dg.FREE)).sum())
    assert (seen > 0).all(), seen                      # no class is vacuous
    assert saw_tie > 0 and saw_boundary > 0 and saw_ulp_occluded > 0 and saw_ulp_free > 0


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_the_tie_keeps_the_first_sample_in_raster_order(shim, tmp_path, kind):
    """z = 1.5 between a 1.25 and a 1.75 of one window, both 0.25 away; with abs_tol = 0.125 the class names the kept one"""
    xyz, what = dc.planted(False)
    depth = dc.depth_image(dc.SMALL, kind)
    prm = dict(w_occluded=0.0, w_free=0.0, w_unknown=1.0, abs_tol=0.125, rel_tol=0.0)
    want, det = dg.classify(xyz, np.eye(4)[:3], dc.SMALL["K"], depth, dc.Z_SCALING, 1, abs_tol=0.125, rel_tol=0.0, details=True)
    below, above = what.index("tie_first_below"), what.index("tie_first_above")
    assert det["tie"][below] and det["tie"][above]
    assert want[below] == dg.OCCLUDED and want[above] == dg.FREE
    assert det["d"][below] == 1.25 and det["d"][above] == 1.75 and det["bz"][below] == 1.5
    got, _ = _run(shim, str(tmp_path / "tie.bin"), xyz, np.eye(4)[:3], dc.SMALL, depth, 1, None, False, None, prm)
    assert np.array_equal(got, want)


def test_sample_validity(shim, tmp_path):
    """U16: only 0 is invalid; F32: NaN, -1, 0, -0, +Inf, -Inf are invalid, the smallest subnormal and FLT_MAX are not"""
    im = dict(H=3, W=3, K=(1.0, 1.0, 1.5, 1.5))
    xyz = np.array([[0.0, 0.0, 1.0]])                          # lands on pixel (1, 1) at the identity, bz = 1
    prm = dict(w_occluded=0.0, w_free=0.0, w_unknown=1.0, abs_tol=0.25, rel_tol=0.0)
    for value, want in ((np.nan, dg.UNKNOWN), (-1.0, dg.UNKNOWN), (0.0, dg.UNKNOWN), (-0.0, dg.UNKNOWN), (np.inf, dg.UNKNOWN),
                        (-np.inf, dg.UNKNOWN), (1.0, dg.CONSISTENT), (1e-45, dg.OCCLUDED), (3.4028234663852886e38, dg.FREE)):
        depth = np.zeros((3, 3), np.float32)
        depth[1, 1] = value
        got, _ = _run(shim, str(tmp_path / "v.bin"), xyz, np.eye(4)[:3], im, depth, 0, None, False, None, prm)
        assert got[0] == want == dg.classify(xyz, np.eye(4)[:3], im["K"], depth, dc.Z_SCALING, 0, 0.25, 0.0)[0], value
    for raw, want in ((0, dg.UNKNOWN), (1, dg.OCCLUDED), (1024, dg.CONSISTENT), (65535, dg.FREE)):
        depth = np.zeros((3, 3), np.uint16)
        depth[1, 1] = raw
        got, _ = _run(shim, str(tmp_path / "v.bin"), xyz, np.eye(4)[:3], im, depth, 0, None, False, None, prm)
        assert got[0] == want == dg.classify(xyz, np.eye(4)[:3], im["K"], depth, dc.Z_SCALING, 0, 0.25, 0.0)[0], raw


def test_argument_checks(shim):
    bad = (float("nan"), float("inf"), -1e-300, -float("inf"))
    assert shim.depth_gate_params_ok_c(1, 0.02, 0.02, 0.0, 0.0, 1.0) == 1
    assert shim.depth_gate_params_ok_c(0, 0.0, 0.0, 1e300, 0.0, 0.0) == 1 and shim.depth_gate_params_ok_c(3, 1.0, 1.0, 1.0, 1.0, 1.0) == 1
    for radius in (-1, 4, 1 << 30):
        assert shim.depth_gate_params_ok_c(radius, 0.02, 0.02, 0.0, 0.0, 1.0) == 0
    for slot in range(5):
        for v in bad:
            args = [0.02, 0.02, 0.0, 0.0, 1.0]
            args[slot] = v
            assert shim.depth_gate_params_ok_c(1, *args) == 0 == int(dg.params_ok(1, *args)), (slot, v)
    assert shim.depth_gate_factors_fit_float_c(3.4028234663852886e38, 0.0, 1.0) == 1
    for slot in range(3):
        args = [0.0, 0.0, 1.0]
        args[slot] = 3.5e38
        assert shim.depth_gate_factors_fit_float_c(*args) == 0
    for kind, h, w, zs in ((0, 480, 640, 5000.0), (1, 3, 3, float("nan")), (1, 32768, 32768, -1.0), (0, 5, 7, 1e-300)):
        assert shim.now_depth_args_ok_c(kind, h, w, zs) == 1 == int(dg.now_depth_args_ok(kind, h, w, zs))
    for kind, h, w, zs in ((2, 480, 640, 5000.0), (-1, 480, 640, 5000.0), (0, 2, 640, 5000.0), (0, 480, 2, 5000.0),
                           (1, 32769, 640, 1.0), (1, 480, 32769, 1.0), (0, 480, 640, 0.0), (0, 480, 640, -5000.0),
                           (0, 480, 640, float("nan")), (0, 480, 640, float("inf"))):
        assert shim.now_depth_args_ok_c(kind, h, w, zs) == 0 == int(dg.now_depth_args_ok(kind, h, w, zs)), (kind, h, w, zs)
    assert shim.depth_gate_seg_bytes_c() % 8 == 0
