"""The reprojection section of include/ea_hip.h through the loaded library, without a GPU: ea_pose_to_matrix and
ea_matrix_to_pose are host functions and give the bits of tests/reproject_ref.py on 200 seeded quaternions (unit and not) and
on every branch of Eigen's conversion; m33 != 1 is refused; and ea_*_reproject / ea_*_overlay refuse their bad arguments with
EA_ERR_INVALID_ARG before a handle is looked at or a device is looked for (the batch forms need the batch's problem count
to read their count x 16 matrices, so here they are given NULLs only; a bad matrix in a real batch is refused in
tests/test_gpu_reproject.py).  The stub's OverlayStats is laid out as the C compiler lays out ea_overlay_stats."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reproject_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
DP = C.POINTER(C.c_double)


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_conversions_are_the_restatement_bit_for_bit(lib):
    from edge_alignment_amd import capi
    rng = np.random.default_rng(31)
    qs = []
    for k in range(200):
        q = rng.normal(size=4)
        qs.append(q / np.linalg.norm(q) if k % 2 else q * 10.0 ** rng.integers(-2, 3))   # every other one is not unit
    qs += [q for branch in rr.branch_quaternions().values() for q in branch]
    for q in qs:
        t = rng.normal(size=3)
        m = capi.pose_to_matrix(q, t)
        want = rr.pose_to_matrix(q, t)
        assert m.shape == (4, 4) and np.array_equal(_bits(m), _bits(want)), q
        q2, t2 = capi.matrix_to_pose(m)
        wq, wt = rr.matrix_to_pose(want)
        assert np.array_equal(_bits(q2), _bits(wq)) and np.array_equal(_bits(t2), _bits(wt)), q


def test_matrix_to_pose_refuses_m33_not_one(lib):
    from edge_alignment_amd import capi
    m = np.eye(4)
    q, t = np.full(4, 7.0), np.full(3, 7.0)
    for bad in (2.0, 0.0, np.nextafter(1.0, 0.0), float("nan")):
        m[3, 3] = bad
        assert lib.ea_matrix_to_pose(m.ctypes.data_as(DP), q.ctypes.data_as(DP), t.ctypes.data_as(DP)) == capi.EA_ERR_INVALID_ARG == -1
        assert b"T(3,3)" in lib.ea_last_error()
    assert (q == 7.0).all() and (t == 7.0).all()
    with pytest.raises(capi.EAError) as ei:
        capi.matrix_to_pose(m)
    assert ei.value.code == capi.EA_ERR_INVALID_ARG
    one = (C.c_double * 16)()
    assert lib.ea_pose_to_matrix(None, one, one) == -1 and lib.ea_pose_to_matrix(one, None, one) == -1
    assert lib.ea_pose_to_matrix(one, one, None) == -1
    assert lib.ea_matrix_to_pose(None, one, one) == -1 and lib.ea_matrix_to_pose(one, None, one) == -1
    assert lib.ea_matrix_to_pose(one, one, None) == -1


def _fake_handle():
    """a non-NULL handle that must not be looked at: the word behind it stays 0"""
    word = C.c_uint64(0)
    return word, C.cast(C.pointer(word), C.c_void_p)


def _bad_matrices():
    good = rr.pose_to_matrix([1.0, 0, 0, 0], [0.0, 0, 0])
    out = []
    for idx, val in (((3, 3), 2.0), ((3, 0), 1.0), ((3, 2), 1e-300), ((0, 1), float("nan")), ((2, 3), float("inf")),
                     ((3, 1), float("nan"))):
        m = good.copy()
        m[idx] = val
        out.append(m)
    return good, out


def test_problem_forms_refuse_bad_arguments_without_a_device(lib):
    from edge_alignment_amd import capi
    word, h = _fake_handle()
    good, bad = _bad_matrices()
    g = good.ctypes.data_as(DP)
    uv = np.zeros((4, 2))
    img = np.zeros((5, 7, 3), np.uint8)
    ip = img.ctypes.data_as(C.c_void_p)
    st = capi.OverlayStats()
    E = capi.EA_ERR_INVALID_ARG
    assert lib.ea_problem_reproject(None, g, uv.ctypes.data_as(DP), 4) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_problem_reproject(h, None, uv.ctypes.data_as(DP), 4) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_problem_reproject(h, g, None, 4) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_problem_overlay(None, g, ip, 5, 7, None, ip, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_problem_overlay(h, None, ip, 5, 7, None, ip, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_problem_overlay(h, g, None, 5, 7, None, ip, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_problem_overlay(h, g, ip, 5, 7, None, None, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    for m in bad:
        mp = m.ctypes.data_as(DP)
        assert lib.ea_problem_reproject(h, mp, uv.ctypes.data_as(DP), 4) == E and b"0 0 0 1" in lib.ea_last_error()
        assert lib.ea_problem_overlay(h, mp, ip, 5, 7, None, ip, C.byref(st)) == E and b"0 0 0 1" in lib.ea_last_error()
    assert E == -1 and word.value == 0 and not img.any() and not uv.any()


def test_batch_forms_refuse_null_arguments_without_a_device(lib):
    from edge_alignment_amd import capi
    word, h = _fake_handle()
    good, _ = _bad_matrices()
    g = good.ctypes.data_as(DP)
    uv = np.zeros((4, 2))
    up = uv.ctypes.data_as(DP)
    arr = (C.c_void_p * 1)(uv.ctypes.data)
    st = capi.OverlayStats()
    E = capi.EA_ERR_INVALID_ARG
    for fn, out in ((lib.ea_batch_reproject, up), (lib.ea_batch_reproject_device, C.c_void_p(uv.ctypes.data))):
        assert fn(None, g, out, 4) == E and b"NULL" in lib.ea_last_error()
        assert fn(h, None, out, 4) == E and b"NULL" in lib.ea_last_error()
        assert fn(h, g, None, 4) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_batch_overlay(None, g, arr, 5, 7, None, arr, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_batch_overlay(h, None, arr, 5, 7, None, arr, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_batch_overlay(h, g, None, 5, 7, None, arr, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_batch_overlay(h, g, arr, 5, 7, None, None, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_batch_overlay_device(None, g, arr, 5, 7, None, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_batch_overlay_device(h, None, arr, 5, 7, None, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_batch_overlay_device(h, g, None, 5, 7, None, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert word.value == 0


def test_the_stub_lays_overlay_stats_out_as_the_c_compiler_does(tmp_path):
    from edge_alignment_amd import capi
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ea_hip.h"', "int main(void) {",
             '  printf("sizeof %zu\\n", sizeof(ea_overlay_stats));']
    for f, _ in capi.OverlayStats._fields_:
        lines.append('  printf("%s %%zu\\n", offsetof(ea_overlay_stats, %s));' % (f, f))
    lines += ["  return 0;", "}"]
    src, exe = tmp_path / "overlay_layout.c", tmp_path / "overlay_layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    got = [ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    want = [["sizeof", str(C.sizeof(capi.OverlayStats))]]
    want += [[f, str(getattr(capi.OverlayStats, f).offset)] for f, _ in capi.OverlayStats._fields_]
    assert got == want and C.sizeof(capi.OverlayStats) == 24
