"""Step 3b of the depth gate -- a depth image at 2^s times the DT extent -- in edge_alignment_amd/csrc/ea_depth_gate.h, built
with the host compiler (-ffp-contract=off) as a stand-alone program (tests/depth_gate_scaled_host_shim.cpp) and held to
tests/depth_gate_scaled_ref.py: class bytes equal byte for byte, counts equal, weights bit for bit; s in 0..3, both depth
kinds, radius 0, 1 and 3, both problem dtypes, with and without the depth-weighting factor and distortion.  The restatement
itself is held to tests/depth_gate_ref.py at s = 0.  No device."""
import os
import struct
import subprocess

import numpy as np
import pytest

import depth_gate_cases as dc
import depth_gate_ref as dg
import depth_gate_scaled_ref as ds

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IM = dc.SMALL
SHIFTS = (0, 1, 2, 3)
RADII = (0, 1, 3)
PRM = dict(w_occluded=0.125, w_free=0.3, w_unknown=0.7, **dc.TOL)
N = 257


@pytest.fixture(scope="module")
def shim():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "depth_gate_scaled_host")
    src = os.path.join(ROOT, "tests", "depth_gate_scaled_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_depth_gate.h"), os.path.join(csrc, "ea_reproject.h"), os.path.join(ROOT, "include", "ea_hip.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-I", csrc, "-o", exe, src])
    return exe


def _run(exe, tmp, xyz, M, s, depth, radius, dist, f32, dw):
    kind = 0 if depth.dtype == np.uint16 else 1
    z_ref, power = dw if dw else (1.0, 0)
    assert depth.shape == (IM["H"] << s, IM["W"] << s)
    src, dst = str(tmp / "case.bin"), str(tmp / "out.bin")
    with open(src, "wb") as f:
        f.write(struct.pack("<10i", len(xyz), IM["H"], IM["W"], kind, radius, int(dist is not None), int(f32), power, s, 0))
        f.write(np.asarray(M, np.float64).reshape(12).tobytes())
        f.write(struct.pack("<4d", *IM["K"]))
        f.write(struct.pack("<5d", *(dist if dist is not None else (0.0,) * 5)))
        f.write(struct.pack("<7d", dc.Z_SCALING, PRM["abs_tol"], PRM["rel_tol"], PRM["w_occluded"], PRM["w_free"], PRM["w_unknown"], z_ref))
        f.write(np.ascontiguousarray(xyz[:, :3], np.float64).tobytes())
        f.write(np.ascontiguousarray(depth).tobytes())
    assert subprocess.run([exe, src, dst]).returncode == 0
    raw = open(dst, "rb").read()
    n = len(xyz)
    assert len(raw) == 9 * n
    return np.frombuffer(raw[:n], np.uint8), np.frombuffer(raw[n:], np.float64)


def _stored(xyz, f32):
    return xyz.astype(np.float32).astype(np.float64) if f32 else xyz


def test_the_restatement_is_depth_gate_ref_at_shift_zero():
    for kind in ("u16", "f32"):
        for depth in (dc.depth_image(IM, kind), ds.depth_image(IM, 0, kind)):
            for xyz in (dc.points(N, 100 + N, IM), ds.points(N, 5, IM)):
                for name, T in dc.MATRICES.items():
                    for dist in (None, dc.DIST):
                        for radius in range(4):
                            want = dg.classify(xyz, T[:3], IM["K"], depth, dc.Z_SCALING, radius, dist=dist, **dc.TOL)
                            got = ds.classify(xyz, T[:3], IM["K"], depth, 0, dc.Z_SCALING, radius, dist=dist, **dc.TOL)
                            assert np.array_equal(got, want), (kind, name, radius)


def test_the_extent_rule():
    assert [ds.shift_of(5, 7, 5 << s, 7 << s) for s in range(10)] == list(range(9)) + [None]
    assert ds.shift_of(5, 7, 6, 7) is None and ds.shift_of(5, 7, 10, 7) is None and ds.shift_of(5, 7, 15, 21) is None
    assert ds.shift_of(5, 7, 10, 28) is None and ds.shift_of(10, 14, 5, 7) is None
    assert ds.shift_of(1 << 14, 1 << 14, 1 << 15, 1 << 15) == 1 and ds.shift_of(1 << 14, 1 << 14, 1 << 16, 1 << 16) is None   # 2^30 pixels


@pytest.mark.parametrize("kind", ["u16", "f32"])
def test_every_class_and_both_borders_occur_in_the_restatement(kind):
    """asserted on the reference first: for every s >= 1 and radius each of the six classes is non-empty, and window centres
    left of column 0, above row 0, past the last column and past the last row occur among the inside points"""
    xyz = ds.points(N, 5, IM)
    for s in SHIFTS[1:]:
        depth = ds.depth_image(IM, s, kind)
        for radius in RADII:
            cls, det = ds.classify(xyz, np.eye(4)[:3], IM["K"], depth, s, dc.Z_SCALING, radius, details=True, **dc.TOL)
            assert (np.bincount(cls, minlength=6) > 0).all(), (s, radius, np.bincount(cls, minlength=6))
            act = det["act"]
            assert (det["IU"][act] < 0).any() and (det["IV"][act] < 0).any(), s
            assert (det["IU"][act] >= IM["W"] << s).any() and (det["IV"][act] >= IM["H"] << s).any(), s
            assert cls[2] == dg.UNKNOWN, (s, radius)          # the planted point in the hole block's corner


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("kind", ["u16", "f32"])
@pytest.mark.parametrize("s", SHIFTS)
def test_classes_counts_and_weights_are_the_restatement(shim, tmp_path, s, kind, f32):
    depth = ds.depth_image(IM, s, kind)
    xyz = _stored(ds.points(N, 5, IM), f32)
    for name in ("identity", "rigid"):
        M = dc.MATRICES[name][:3]
        for dist in (None, dc.DIST):
            for radius in RADII:
                want = ds.classify(xyz, M, IM["K"], depth, s, dc.Z_SCALING, radius, dist=dist, **dc.TOL)
                if s == 0:
                    assert np.array_equal(want, dg.classify(xyz, M, IM["K"], depth, dc.Z_SCALING, radius, dist=dist, **dc.TOL))
                for dw in ((None, (1.25, 3)) if radius == 1 else (None,)):
                    got, w = _run(shim, tmp_path, xyz, M, s, depth, radius, dist, f32, dw)
                    where = (s, kind, f32, name, dist is not None, radius, dw)
                    assert np.array_equal(got, want), where + (np.flatnonzero(got != want)[:8],)
                    assert dg.stats(got) == dg.stats(want), where
                    ww = dg.weights(want, xyz[:, 2], PRM["w_occluded"], PRM["w_free"], PRM["w_unknown"], dw, f32)
                    assert np.array_equal(w.view(np.uint64), ww.view(np.uint64)), where
