"""edge_alignment_amd/csrc/ea_reproject.h -- the matrix of step A that the reprojection kernel applies, the pose <-> matrix
conversions and the check of a pose argument -- built with the host compiler (-ffp-contract=off, as the other host shims)
and held to tests/reproject_ref.py bit for bit: the plain row copy, the rig product (T12 b_T_a) T12^-1 in its fixed order on
seeded rigid and on general affine matrices, and the conversions on seeded quaternions.  No device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reproject_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def shim():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "reproject_host.so")
    src = os.path.join(ROOT, "tests", "reproject_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_reproject.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I", csrc,
                               "-o", so, src])
    return C.CDLL(so)


def _dp(a):
    return a.ctypes.data_as(DP)


def _rigid(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return rr.pose_to_matrix(q, rng.normal(size=3))


def _affine(rng):
    m = np.eye(4)
    m[:3] = rng.normal(size=(3, 4)) * 10.0 ** rng.integers(-3, 4)
    return m


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_plain_matrix_is_the_row_copy(shim):
    rng = np.random.default_rng(11)
    for _ in range(20):
        T = _affine(rng)
        M = np.zeros((3, 4))
        shim.reproject_matrix_c(_dp(T), None, None, _dp(M))
        assert np.array_equal(_bits(M), _bits(rr.plain_matrix(T)))


@pytest.mark.parametrize("kind", ["rigid", "affine"])
def test_rig_matrix_bit_for_bit(shim, kind):
    rng = np.random.default_rng(12 if kind == "rigid" else 13)
    make = _rigid if kind == "rigid" else _affine
    differs_from_other_association = 0
    for _ in range(200):
        T, T12 = make(rng), make(rng)
        T12inv = np.linalg.inv(T12)
        T12inv[3] = (0.0, 0.0, 0.0, 1.0)
        M = np.zeros((3, 4))
        shim.reproject_matrix_c(_dp(T), _dp(T12), _dp(T12inv), _dp(M))
        want = rr.rig_matrix(T, T12, T12inv)
        assert np.array_equal(_bits(M), _bits(want))
        other = rr.mul4(T12, rr.mul4(T, T12inv))[:3]
        differs_from_other_association += int(not np.array_equal(_bits(other), _bits(want)))
        assert np.allclose(other, want, rtol=1e-9, atol=1e-9 * np.abs(want).max())
    assert differs_from_other_association > 0   # the order is a definition, not a formality


def test_conversions_bit_for_bit(shim):
    rng = np.random.default_rng(14)
    for k in range(200):
        q = rng.normal(size=4) * (1.0 if k % 2 else 10.0 ** rng.integers(-2, 3))
        if k % 2:
            q /= np.linalg.norm(q)
        t = rng.normal(size=3)
        m = np.zeros((4, 4))
        shim.pose_to_matrix_c(_dp(q), _dp(t), _dp(m))
        want = rr.pose_to_matrix(q, t)
        assert np.array_equal(_bits(m), _bits(want))
        q2, t2 = np.zeros(4), np.zeros(3)
        assert shim.matrix_to_pose_c(_dp(m), _dp(q2), _dp(t2)) == 1
        wq, wt = rr.matrix_to_pose(want)
        assert np.array_equal(_bits(q2), _bits(wq)) and np.array_equal(_bits(t2), _bits(wt))
    m = rr.pose_to_matrix([1.0, 0, 0, 0], [0.0, 0, 0])
    m[3, 3] = np.nextafter(1.0, 2.0)
    assert shim.matrix_to_pose_c(_dp(m), _dp(np.zeros(4)), _dp(np.zeros(3))) == 0


def test_pose_argument_check(shim):
    good = rr.pose_to_matrix([0.5, 0.5, 0.5, 0.5], [1.0, 2.0, 3.0])
    assert shim.reproject_pose_ok_c(_dp(good)) == 1
    for idx, val in (((3, 3), 2.0), ((3, 0), 1e-300), ((3, 1), -1.0), ((3, 2), float("nan")), ((0, 0), float("nan")),
                     ((1, 3), float("inf")), ((2, 1), -float("inf")), ((3, 3), float("nan"))):
        bad = good.copy()
        bad[idx] = val
        assert shim.reproject_pose_ok_c(_dp(bad)) == 0, (idx, val)
    neg0 = good.copy()
    neg0[3, 0] = -0.0     # compares equal to 0: accepted
    assert shim.reproject_pose_ok_c(_dp(neg0)) == 1
    assert shim.reproject_seg_bytes_c() % 8 == 0
