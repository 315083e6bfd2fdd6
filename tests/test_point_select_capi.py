"""Point selection through the C-ABI without a device: the defaults, the struct layouts the ctypes mirrors must match, every
rejected parameter combination -- EA_ERR_INVALID_ARG before a handle is looked at or a device is looked for --, and the plain-C
example building against the header."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BAD = (dict(cell_px=-1), dict(cell_px=4097), dict(cell_rule=2), dict(cell_rule=-1), dict(outside=2), dict(outside=-1), dict(stride=0),
       dict(stride=-5), dict(target=-1), dict(stride=2, target=5), dict(height=-1, width=-1), dict(height=29), dict(width=37),
       dict(cell_px=1, height=8193, width=8192))


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def test_defaults_and_layouts(lib):
    from edge_alignment_amd import capi
    prm = capi.default_point_selection()
    assert (prm.cell_px, prm.cell_rule, prm.outside, prm.height, prm.width, prm.stride, prm.target) == (0, capi.CELL_FIRST, 0, 0, 0, 1, 0)
    lib.ea_default_point_selection(None)                                     # like free(NULL)
    assert C.sizeof(capi.PointSelection) == 5 * 4 + 4 + 2 * 8               # five ints, padding, two int64
    assert capi.PointSelection.stride.offset == 24 and capi.PointSelection.target.offset == 32
    assert C.sizeof(capi.PointSelectionStats) == 5 * 8
    with pytest.raises(TypeError):
        capi.default_point_selection(cells=4)
    # the C compiler lays the structs out the same way
    probe = r'''
#include <stddef.h>
#include <stdio.h>
#include "ea_hip.h"
int main(void) {
  printf("%d %d %d %d\n", (int)sizeof(ea_point_selection), (int)offsetof(ea_point_selection, stride),
         (int)offsetof(ea_point_selection, target), (int)sizeof(ea_point_selection_stats));
  return EA_CELL_FIRST == 0 && EA_CELL_NEAREST == 1 ? 0 : 1;
}
'''
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    src, exe = os.path.join(out_dir, "point_select_layout.c"), os.path.join(out_dir, "point_select_layout")
    with open(src, "w") as f:
        f.write(probe)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
    assert subprocess.check_output([exe]).split() == [b"40", b"24", b"32", b"40"]


def test_parameter_errors_come_before_any_handle_or_device(lib):
    from edge_alignment_amd import capi
    st = capi.PointSelectionStats()
    for bad in BAD:
        prm = capi.default_point_selection(**bad)
        assert lib.ea_problem_select_points(None, C.byref(prm), C.byref(st)) == capi.EA_ERR_INVALID_ARG, bad
        assert b"NULL" not in lib.ea_last_error(), (bad, lib.ea_last_error())  # the parameter is named, not the handle
        assert lib.ea_batch_select_points(None, None, 0, C.byref(prm), None) == capi.EA_ERR_INVALID_ARG, bad
        assert lib.ea_tracker_batch_set_point_selection(None, C.byref(prm)) == capi.EA_ERR_INVALID_ARG, bad
        assert b"NULL" not in lib.ea_last_error(), (bad, lib.ea_last_error())
    ok = capi.default_point_selection(cell_px=4, target=200)
    for call in (lambda: lib.ea_problem_select_points(None, C.byref(ok), None), lambda: lib.ea_problem_select_points(None, None, None),
                 lambda: lib.ea_batch_select_points(None, None, 0, C.byref(ok), None),
                 lambda: lib.ea_tracker_batch_set_point_selection(None, C.byref(ok)), lambda: lib.ea_tracker_batch_set_point_selection(None, None),
                 lambda: lib.ea_tracker_batch_last_point_selection(None, C.byref(st), 1)):
        assert call() == capi.EA_ERR_INVALID_ARG
        assert b"NULL" in lib.ea_last_error()
    # inside the tracker every level uses its own DT extent: a named extent is refused
    named = capi.default_point_selection(cell_px=4, height=48, width=64)
    assert lib.ea_tracker_batch_set_point_selection(None, C.byref(named)) == capi.EA_ERR_INVALID_ARG
    assert b"height and width must be 0" in lib.ea_last_error()


def test_the_example_builds(lib):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "point_selection_demo"])
    assert os.path.exists(os.path.join(ROOT, "examples", "point_selection_demo"))
