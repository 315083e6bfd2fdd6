"""The boundary of the coarse-to-fine calls without a GPU: ea_resize_half_levels, ea_batch_set_frames_ros_pyramid[_device],
ea_batch_solve_pyramid, ea_tracker_batch_create_pyramid, ea_tracker_batch_level_problem and ea_tracker_batch_last_summaries are
declared in include/ea_hip.h with the signatures a C compiler checks below, bound by the ctypes stub, NULL and range misuse is
refused with EA_ERR_INVALID_ARG before a device is looked for, and the call as the header documents it is plain C99."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = ("ea_resize_half_levels", "ea_batch_set_frames_ros_pyramid", "ea_batch_set_frames_ros_pyramid_device",
         "ea_batch_solve_pyramid", "ea_tracker_batch_create_pyramid", "ea_tracker_batch_level_problem",
         "ea_tracker_batch_last_summaries")


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def test_header_and_stub_declare_the_calls(lib):
    from edge_alignment_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(INCLUDE, "ea_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in capi.EXPORTED, name
        assert hasattr(lib, name), name
    for name in ("resize_half_levels", "set_frames_ros_pyramid", "solve_pyramid_batch"):
        assert hasattr(capi, name), name
    assert hasattr(capi.TrackerBatch, "level_problem") and hasattr(capi.TrackerBatch, "last_summaries")


SIGNATURES_PROGRAM = r"""
#include <stddef.h>
#include "ea_hip.h"

/* an assignment to a pointer of the declared type compiles without a diagnostic only when the header agrees */
int (*const p_levels)(int, int, const void *, int, int, int, int, void *const *) = ea_resize_half_levels;
int (*const p_frames)(ea_batch *const *, int, const uint8_t *const *, const float *const *, const uint8_t *const *,
                      const ea_ros_frame_params *) = ea_batch_set_frames_ros_pyramid;
int (*const p_frames_device)(ea_batch *const *, int, const uint8_t *const *, const float *const *, const uint8_t *const *,
                             const ea_ros_frame_params *) = ea_batch_set_frames_ros_pyramid_device;
int (*const p_solve)(ea_batch *const *, int, const ea_options *, double *, double *, ea_summary *) = ea_batch_solve_pyramid;
int (*const p_create)(ea_tracker_batch **, const ea_camera *, int, int, int, int, int) = ea_tracker_batch_create_pyramid;
ea_problem *(*const p_level_problem)(ea_tracker_batch *, int, int) = ea_tracker_batch_level_problem;
int (*const p_last)(ea_tracker_batch *, int, ea_summary *) = ea_tracker_batch_last_summaries;

/* N cameras, 1280 x 960 frames, the node's halving and three levels: the frames of a push go up once */
int track_coarse_to_fine(const ea_camera *cams_3_levels, int n, const uint8_t *const *bgr, const void *const *depth_m, double *q,
                         double *t, int *aligned, ea_summary *per_level_of_stream_0) {
  ea_tracker_batch *tb;
  int64_t levels = 0;
  int l, rc = ea_tracker_batch_create_pyramid(&tb, cams_3_levels, n, 3, EA_F64, 0, 1);
  if (rc != EA_OK) return rc;
  for (l = 0; l < 3 && rc == EA_OK; ++l) rc = ea_problem_set_loss(ea_tracker_batch_level_problem(tb, l, 0), EA_LOSS_CAUCHY, 1.0);
  if (rc == EA_OK) rc = ea_tracker_batch_push_frames(tb, bgr, depth_m, 960, 1280, 0.0, NULL, q, t, NULL, aligned);
  if (rc == EA_OK) rc = ea_tracker_batch_last_summaries(tb, 0, per_level_of_stream_0);
  if (rc == EA_OK) rc = ea_tracker_batch_get_info(tb, "levels", &levels);
  ea_tracker_batch_destroy(tb);
  return rc == EA_OK && levels != 3 ? EA_ERR_STATE : rc;
}

/* the producers and the solve by themselves: levels[l] = a batch of the same pairs' problems at full >> (1 + l) */
int align_pairs_coarse_to_fine(ea_batch *const *levels, int nlevels, const uint8_t *const *ref_bgr, const float *const *ref_depth,
                               const uint8_t *const *now_bgr, double *q, double *t, ea_summary *summaries, int64_t *uploaded) {
  ea_ros_frame_params prm;
  int rc;
  ea_default_ros_frame_params(&prm, 960, 1280);
  prm.halvings = 1;
  rc = ea_batch_set_frames_ros_pyramid(levels, nlevels, ref_bgr, ref_depth, now_bgr, &prm);
  if (rc != EA_OK) return rc; /* EA_ERR_STATE: ea_last_error() names the first (level, frame) without an edge */
  rc = ea_batch_get_info(levels[0], "frames_uploaded", uploaded);
  return rc != EA_OK ? rc : ea_batch_solve_pyramid(levels, nlevels, NULL, q, t, summaries);
}
"""


def test_declared_signatures_and_documented_use_are_plain_c99(tmp_path):
    src = tmp_path / "pyramid_doc.c"
    src.write_text(SIGNATURES_PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, str(src)])


def test_resize_half_levels_refuses_misuse_without_a_device(lib):
    from edge_alignment_amd import capi
    buf = (C.c_uint8 * (8 * 12 * 3))()
    out = (C.c_uint8 * (8 * 12 * 3))()
    dst = (C.c_void_p * 2)(C.addressof(out), C.addressof(out))
    bad = [(0, None, 8, 12, 1, 1, dst), (0, buf, 8, 12, 1, 1, None), (0, buf, 8, 12, 1, 1, (C.c_void_p * 1)()),
           (3, buf, 8, 12, 1, 1, dst), (-1, buf, 8, 12, 1, 1, dst),
           (0, buf, 8, 12, 1, 0, dst), (0, buf, 8, 12, -1, 1, dst), (0, buf, 8, 12, 8, 2, dst),   # keep < 1, skip < 0, 9 steps
           (0, buf, 8, 12, 3, 1, dst), (0, buf, 7, 12, 1, 1, dst), (0, buf, 0, 12, 0, 1, dst), (0, buf, 8, 40000, 1, 1, dst)]
    for kind, src, h, w, skip, keep, d in bad:
        assert lib.ea_resize_half_levels(0, kind, src, h, w, skip, keep, d) == capi.EA_ERR_INVALID_ARG, (kind, h, w, skip, keep)
        assert lib.ea_last_error()
    # level 0 alone is the frame itself and needs no device
    buf[5] = 77
    assert lib.ea_resize_half_levels(0, 0, buf, 8, 12, 0, 1, dst) == capi.EA_OK and out[5] == 77


@pytest.mark.parametrize("name", NAMES[1:3])
def test_the_producers_refuse_missing_arguments_without_a_device(lib, name):
    from edge_alignment_amd import capi
    fn = getattr(lib, name)
    prm = capi.RosFrameParams()
    lib.ea_default_ros_frame_params(C.byref(prm), 480, 640)
    one = (C.c_void_p * 1)()
    word = C.c_uint64(0)
    handle = (C.c_void_p * 2)(C.cast(C.pointer(word), C.c_void_p), None)   # (any non-NULL handle will do for the checks in front)
    assert fn(None, 1, one, one, one, C.byref(prm)) == capi.EA_ERR_INVALID_ARG and b"NULL" in lib.ea_last_error()
    assert fn(handle, 1, one, one, one, None) == capi.EA_ERR_INVALID_ARG and b"NULL" in lib.ea_last_error()
    assert fn(handle, 0, one, one, one, C.byref(prm)) == capi.EA_ERR_INVALID_ARG
    assert fn(handle, 10, one, one, one, C.byref(prm)) == capi.EA_ERR_INVALID_ARG
    assert fn(handle, 2, one, one, one, C.byref(prm)) == capi.EA_ERR_INVALID_ARG and b"NULL level" in lib.ea_last_error()
    prm.halvings = 8
    assert fn(handle, 1, one, one, one, C.byref(prm)) == capi.EA_ERR_INVALID_ARG     # 480 is not divisible by 256
    prm.halvings = -1
    assert fn(handle, 1, one, one, one, C.byref(prm)) == capi.EA_ERR_INVALID_ARG
    assert word.value == 0


def test_solve_and_tracker_refuse_misuse_without_a_device(lib):
    from edge_alignment_amd import capi
    q, t = (C.c_double * 4)(), (C.c_double * 3)()
    word = C.c_uint64(0)
    handle = (C.c_void_p * 2)(C.cast(C.pointer(word), C.c_void_p), None)
    assert lib.ea_batch_solve_pyramid(None, 1, None, q, t, None) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_batch_solve_pyramid(handle, 0, None, q, t, None) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_batch_solve_pyramid(handle, 1, None, None, t, None) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_batch_solve_pyramid(handle, 1, None, q, None, None) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_batch_solve_pyramid((C.c_void_p * 1)(), 1, None, q, t, None) == capi.EA_ERR_INVALID_ARG
    cams = (capi.Camera * 4)(*[capi.Camera(500.0, 500.0, 31.5, 23.5)] * 4)
    h = C.c_void_p()
    for count, levels, halvings, with_cams, with_out, says in ((2, 0, 0, True, True, b"levels"), (2, -1, 0, True, True, b"levels"),
                                                              (2, 3, 7, True, True, b"levels"), (2, 2, 9, True, True, b"halvings"),
                                                              (0, 2, 0, True, True, b"1..65535"), (2, 2, 0, False, True, b"NULL"),
                                                              (2, 2, 0, True, False, b"NULL"), (2, 2, -1, True, True, b"halvings")):
        rc = lib.ea_tracker_batch_create_pyramid(C.byref(h) if with_out else None, cams if with_cams else None, count, levels, 0, 0, halvings)
        assert rc == capi.EA_ERR_INVALID_ARG and says in lib.ea_last_error(), (count, levels, halvings, lib.ea_last_error())
        assert not h.value
    assert lib.ea_tracker_batch_level_problem(None, 0, 0) is None
    s = capi.Summary()
    assert lib.ea_tracker_batch_last_summaries(None, 0, C.byref(s)) == capi.EA_ERR_INVALID_ARG and b"NULL" in lib.ea_last_error()
    with pytest.raises(capi.EAError) as ei:
        capi.TrackerBatch([[(500.0, 500.0, 31.5, 23.5)] * 2] * 2, flavour=1, levels=2)   # levels belong to the ROS flavour
    assert ei.value.code == capi.EA_ERR_INVALID_ARG
