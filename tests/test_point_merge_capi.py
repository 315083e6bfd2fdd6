"""Point transform, merge and carry through the C-ABI without a device: the defaults, the struct layouts the ctypes mirrors must
match, every rejected parameter and matrix -- EA_ERR_INVALID_ARG before a handle is looked at or a device is looked for --, and
the plain-C example building against the header.  The rows that need a problem to exist (an index of sel out of range or twice,
dst == src, differing dtypes, EA_ERR_STATE for a storage order, a missing extent or DT image, a tracker outside keyframe mode)
are in tests/test_gpu_point_merge.py: no problem exists without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from point_merge_cases import BAD_MATRICES, BAD_PARAMS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = (C.c_double * 16)(*np.eye(4).reshape(16))


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def test_defaults_and_layouts(lib):
    from edge_alignment_amd import capi
    prm = capi.default_point_merge()
    assert (prm.require_pixel, prm.margin, prm.max_dt, prm.cell_px, prm.cell_rule, prm.height, prm.width, prm.max_carried,
            prm.weight_scale) == (0, 0, -1.0, 0, capi.CELL_FIRST, 0, 0, 0, 1.0)
    lib.ea_default_point_merge(None)                                         # like free(NULL)
    assert C.sizeof(capi.PointMerge) == 48 and C.sizeof(capi.PointMergeStats) == 9 * 8
    assert (capi.PointMerge.max_dt.offset, capi.PointMerge.cell_px.offset, capi.PointMerge.max_carried.offset,
            capi.PointMerge.weight_scale.offset) == (8, 16, 32, 40)
    with pytest.raises(TypeError):
        capi.default_point_merge(cells=4)
    probe = r'''
#include <stddef.h>
#include <stdio.h>
#include "ea_hip.h"
int main(void) {
  printf("%d %d %d %d %d %d\n", (int)sizeof(ea_point_merge), (int)offsetof(ea_point_merge, max_dt), (int)offsetof(ea_point_merge, cell_px),
         (int)offsetof(ea_point_merge, max_carried), (int)offsetof(ea_point_merge, weight_scale), (int)sizeof(ea_point_merge_stats));
  return 0;
}
'''
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    src, exe = os.path.join(out_dir, "point_merge_layout.c"), os.path.join(out_dir, "point_merge_layout")
    with open(src, "w") as f:
        f.write(probe)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    assert subprocess.check_output([exe]).split() == [b"48", b"8", b"16", b"32", b"40", b"72"]


def test_parameter_errors_come_before_any_handle_or_device(lib):
    from edge_alignment_amd import capi
    st = capi.PointMergeStats()
    for bad in BAD_PARAMS:
        prm = capi.default_point_merge(**bad)
        assert lib.ea_problem_merge_points(None, None, EYE, C.byref(prm), C.byref(st)) == capi.EA_ERR_INVALID_ARG, bad
        assert b"NULL" not in lib.ea_last_error(), (bad, lib.ea_last_error())  # the parameter is named, not the handle
        assert lib.ea_batch_merge_points(None, None, 0, None, EYE, C.byref(prm), None) == capi.EA_ERR_INVALID_ARG, bad
        assert b"NULL" not in lib.ea_last_error(), (bad, lib.ea_last_error())
        assert lib.ea_tracker_batch_set_point_carry(None, C.byref(prm)) == capi.EA_ERR_INVALID_ARG, bad
        assert b"NULL" not in lib.ea_last_error(), (bad, lib.ea_last_error())
    ok = capi.default_point_merge(cell_px=4, max_dt=1.0, weight_scale=0.5)
    for i, v in BAD_MATRICES:
        M = np.eye(4).reshape(16)
        M[i] = v
        M = (C.c_double * 16)(*M)
        assert lib.ea_problem_transform_points(None, M) == capi.EA_ERR_INVALID_ARG, (i, v)
        assert b"last row" in lib.ea_last_error(), (i, v, lib.ea_last_error())
        assert lib.ea_problem_merge_points(None, None, M, C.byref(ok), None) == capi.EA_ERR_INVALID_ARG, (i, v)
        assert b"last row" in lib.ea_last_error(), (i, v, lib.ea_last_error())
    for call in (lambda: lib.ea_problem_transform_points(None, EYE), lambda: lib.ea_problem_transform_points(None, None),
                 lambda: lib.ea_batch_transform_points(None, None, 0, EYE), lambda: lib.ea_batch_transform_points(None, None, 0, None),
                 lambda: lib.ea_problem_merge_points(None, None, EYE, C.byref(ok), None),
                 lambda: lib.ea_problem_merge_points(None, None, EYE, None, None),
                 lambda: lib.ea_problem_merge_points(None, None, None, C.byref(ok), None),
                 lambda: lib.ea_batch_merge_points(None, None, 0, None, EYE, C.byref(ok), None),
                 lambda: lib.ea_batch_merge_points(None, None, 0, None, EYE, None, None),
                 lambda: lib.ea_tracker_batch_set_point_carry(None, C.byref(ok)), lambda: lib.ea_tracker_batch_set_point_carry(None, None),
                 lambda: lib.ea_tracker_batch_last_point_carry(None, C.byref(st), 1)):
        assert call() == capi.EA_ERR_INVALID_ARG
        assert b"NULL" in lib.ea_last_error()
    # inside the tracker a stream uses its own DT extent: a named extent is refused
    named = capi.default_point_merge(cell_px=4, height=48, width=64)
    assert lib.ea_tracker_batch_set_point_carry(None, C.byref(named)) == capi.EA_ERR_INVALID_ARG
    assert b"height and width must be 0" in lib.ea_last_error()


def test_the_example_builds(lib):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "model_prior_demo"])
    assert os.path.exists(os.path.join(ROOT, "examples", "model_prior_demo"))
