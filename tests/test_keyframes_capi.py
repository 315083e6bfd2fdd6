"""The boundary of the pose statistics and of the tracker's keyframe mode without a GPU: ea_problem_pose_stats,
ea_batch_pose_stats and ea_tracker_batch_set_keyframes refuse their bad arguments with EA_ERR_INVALID_ARG before a handle is
looked at or a device is looked for, the stub's three structures are laid out as a C compiler lays out the header's, and
ea_default_keyframe_params gives the documented values."""
import ctypes as C
import math
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def _fake_handle():
    """a non-NULL handle that must not be looked at: the word behind it stays 0"""
    word = C.c_uint64(0)
    return word, C.cast(C.pointer(word), C.c_void_p)


@pytest.mark.parametrize("name", ["ea_problem_pose_stats", "ea_batch_pose_stats"])
def test_pose_stats_refuses_bad_arguments_without_a_device(lib, name):
    from edge_alignment_amd import capi
    fn = getattr(lib, name)
    q, t, out = (C.c_double * 4)(1, 0, 0, 0), (C.c_double * 3)(), capi.PoseStats()
    word, h = _fake_handle()
    inf = float("inf")
    assert fn(None, q, t, 0, inf, C.byref(out)) == capi.EA_ERR_INVALID_ARG and b"NULL" in lib.ea_last_error()
    assert fn(h, None, t, 0, inf, C.byref(out)) == capi.EA_ERR_INVALID_ARG and b"NULL" in lib.ea_last_error()
    assert fn(h, q, None, 0, inf, C.byref(out)) == capi.EA_ERR_INVALID_ARG and b"NULL" in lib.ea_last_error()
    assert fn(h, q, t, 0, inf, None) == capi.EA_ERR_INVALID_ARG and b"NULL" in lib.ea_last_error()
    assert fn(h, q, t, -1, inf, C.byref(out)) == capi.EA_ERR_INVALID_ARG and b"margin" in lib.ea_last_error()
    assert fn(h, q, t, 0, -1e-300, C.byref(out)) == capi.EA_ERR_INVALID_ARG and b"inlier_residual" in lib.ea_last_error()
    assert fn(h, q, t, 0, float("nan"), C.byref(out)) == capi.EA_ERR_INVALID_ARG and b"inlier_residual" in lib.ea_last_error()
    assert fn(h, q, t, 0, -inf, C.byref(out)) == capi.EA_ERR_INVALID_ARG
    assert capi.EA_ERR_INVALID_ARG == -1 and word.value == 0


FLOAT_FIELDS = ("min_visible_fraction", "min_inlier_fraction", "inlier_residual", "max_mean_flow")


def test_set_keyframes_refuses_bad_arguments_without_a_device(lib):
    from edge_alignment_amd import capi
    prm = capi.KeyframeParams()
    lib.ea_default_keyframe_params(C.byref(prm))
    assert lib.ea_tracker_batch_set_keyframes(None, C.byref(prm)) == capi.EA_ERR_INVALID_ARG and b"NULL" in lib.ea_last_error()
    assert lib.ea_tracker_batch_set_keyframes(None, None) == capi.EA_ERR_INVALID_ARG
    word, h = _fake_handle()
    for f in FLOAT_FIELDS:
        bad = capi.keyframe_params(**{f: float("nan")})
        assert lib.ea_tracker_batch_set_keyframes(h, C.byref(bad)) == capi.EA_ERR_INVALID_ARG, f
        assert b"NaN" in lib.ea_last_error()
    bad = capi.keyframe_params(margin=-1)
    assert lib.ea_tracker_batch_set_keyframes(h, C.byref(bad)) == capi.EA_ERR_INVALID_ARG
    st = capi.KeyframeState()
    assert lib.ea_tracker_batch_keyframe_state(None, 0, C.byref(st)) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_tracker_batch_keyframe_state(h, 0, None) == capi.EA_ERR_INVALID_ARG
    assert word.value == 0


def test_default_keyframe_params(lib):
    from edge_alignment_amd import capi
    prm = capi.KeyframeParams()
    C.memset(C.byref(prm), 0xff, C.sizeof(prm))
    lib.ea_default_keyframe_params(C.byref(prm))
    assert prm.min_visible_fraction == 0.75
    assert (prm.min_inlier_fraction, prm.inlier_residual, prm.max_mean_flow, prm.max_frames, prm.margin) == (0.0, 0.0, 0.0, 0, 0)
    lib.ea_default_keyframe_params(None)   # like free(NULL)
    assert not math.isnan(capi.keyframe_params(max_frames=3).min_visible_fraction)
    with pytest.raises(TypeError):
        capi.keyframe_params(no_such_field=1)
    assert (capi.KEY_FIRST, capi.KEY_SOLVE_FAILED, capi.KEY_VISIBLE, capi.KEY_INLIERS, capi.KEY_FLOW, capi.KEY_AGE) == (1, 2, 4, 8, 16, 32)


STRUCTS = (("ea_pose_stats", "PoseStats"), ("ea_keyframe_params", "KeyframeParams"), ("ea_keyframe_state", "KeyframeState"))


def _layout_program():
    from edge_alignment_amd import capi
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ea_hip.h"', "int main(void) {"]
    for cname, pyname in STRUCTS:
        lines.append('  printf("%s sizeof %%zu\\n", sizeof(%s));' % (cname, cname))
        for f, _ in getattr(capi, pyname)._fields_:
            lines.append('  printf("%s %s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f))
    lines.append('  printf("enum %d %d %d %d %d %d\\n", EA_KEY_FIRST, EA_KEY_SOLVE_FAILED, EA_KEY_VISIBLE, EA_KEY_INLIERS, EA_KEY_FLOW, EA_KEY_AGE);')
    lines += ["  return 0;", "}"]
    return "\n".join(lines) + "\n"


def test_the_stub_lays_the_structs_out_as_the_c_compiler_does(tmp_path):
    from edge_alignment_amd import capi
    src, exe = tmp_path / "keyframe_layout.c", tmp_path / "keyframe_layout"
    src.write_text(_layout_program())
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    got = [ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    want = []
    for cname, pyname in STRUCTS:
        cls = getattr(capi, pyname)
        want.append([cname, "sizeof", str(C.sizeof(cls))])
        want += [[cname, f, str(getattr(cls, f).offset)] for f, _ in cls._fields_]
    want.append(["enum", "1", "2", "4", "8", "16", "32"])
    assert got == want
    assert C.sizeof(capi.PoseStats) == 48 and C.sizeof(capi.KeyframeParams) == 40 and C.sizeof(capi.KeyframeState) == 64
