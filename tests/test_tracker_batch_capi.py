"""The boundary of the multi-stream tracker without a GPU: the ea_tracker_batch_* entry points are declared in
include/ea_hip.h and bound by the ctypes stub, every invalid argument that can be told without a tracker is refused with
EA_ERR_INVALID_ARG and a message before a device is looked for, NULL handles are accepted where free(NULL) would be, and the
call as the header documents it is plain C99.  (What a push refuses once a tracker exists -- NULL entries, extents,
z_scaling, host memory handed to the _device form -- needs a tracker and therefore a device: tests/test_gpu_tracker_batch.py.)"""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = ("ea_tracker_batch_create", "ea_tracker_batch_destroy", "ea_tracker_batch_count", "ea_tracker_batch_problem",
         "ea_tracker_batch_push_frames", "ea_tracker_batch_push_frames_device", "ea_tracker_batch_reset",
         "ea_tracker_batch_set_covariance", "ea_tracker_batch_last_covariance", "ea_tracker_batch_set_motion_prior",
         "ea_tracker_batch_get_info")


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
    assert hasattr(capi, "TrackerBatch")


CREATE_CASES = [
    # (count, dtype, flavour, halvings, cameras given, handle given) -> what the message names
    ((0, 0, 0, 0, True, True), b"1..65535"),
    ((-3, 0, 0, 0, True, True), b"1..65535"),
    ((65536, 0, 0, 0, True, True), b"1..65535"),
    ((2, 0, 3, 0, True, True), b"flavour"),
    ((2, 0, -1, 0, True, True), b"flavour"),
    ((2, 0, 0, 1, True, True), b"halvings"),
    ((2, 0, 1, 2, True, True), b"halvings"),
    ((2, 0, 2, 9, True, True), b"halvings"),
    ((2, 0, 2, -1, True, True), b"halvings"),
    ((2, 0, 0, 0, False, True), b"NULL"),
    ((2, 0, 0, 0, True, False), b"NULL"),
    ((2, 7, 0, 0, True, True), b"dtype"),
]


@pytest.mark.parametrize("case,says", CREATE_CASES, ids=lambda v: "-".join(map(str, v)) if isinstance(v, tuple) else None)
def test_create_refuses_invalid_arguments_without_a_device(lib, case, says):
    from edge_alignment_amd import capi
    count, dtype, flavour, halvings, with_cams, with_out = case
    cams = (capi.Camera * 2)(capi.Camera(500.0, 500.0, 31.5, 23.5), capi.Camera(510.0, 505.0, 32.0, 24.0))
    h = C.c_void_p()
    rc = lib.ea_tracker_batch_create(C.byref(h) if with_out else None, cams if with_cams else None, count, dtype, 0, flavour, halvings)
    assert rc == capi.EA_ERR_INVALID_ARG
    assert says in lib.ea_last_error(), lib.ea_last_error()
    assert not h.value


def test_a_camera_that_no_problem_takes_is_refused(lib):
    from edge_alignment_amd import capi
    cams = (capi.Camera * 2)(capi.Camera(500.0, 500.0, 31.5, 23.5), capi.Camera(0.0, 505.0, 32.0, 24.0))
    h = C.c_void_p()
    rc = lib.ea_tracker_batch_create(C.byref(h), cams, 2, 0, 0, 0, 0)
    # (with a device the first stream's problem exists by then and is destroyed again; without one the device is what fails)
    assert rc == (capi.EA_ERR_INVALID_ARG if capi.device_count() > 0 else capi.EA_ERR_NO_DEVICE) and not h.value


def test_null_handles(lib):
    from edge_alignment_amd import capi
    lib.ea_tracker_batch_destroy(None)                        # like free(NULL)
    assert lib.ea_tracker_batch_count(None) == 0
    assert lib.ea_tracker_batch_problem(None, 0) is None
    one = (C.c_void_p * 1)()
    q, t = (C.c_double * 4)(), (C.c_double * 3)()
    for fn in (lib.ea_tracker_batch_push_frames, lib.ea_tracker_batch_push_frames_device):
        assert fn(None, one, one, 48, 64, 5000.0, None, q, t, None, None) == capi.EA_ERR_INVALID_ARG
        assert b"NULL" in lib.ea_last_error()
    assert lib.ea_tracker_batch_reset(None, -1) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_tracker_batch_set_covariance(None, None) == capi.EA_ERR_INVALID_ARG
    cov = capi.Covariance()
    assert lib.ea_tracker_batch_last_covariance(None, 0, C.byref(cov)) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_tracker_batch_set_motion_prior(None, 0.1, 0.1) == capi.EA_ERR_INVALID_ARG
    v = C.c_int64()
    assert lib.ea_tracker_batch_get_info(None, b"aligned", C.byref(v)) == capi.EA_ERR_INVALID_ARG
    assert b"NULL" in lib.ea_last_error()


def test_the_stub_refuses_to_build_a_tracker_without_a_device(lib):
    from edge_alignment_amd import capi
    if capi.device_count() > 0:
        tb = capi.TrackerBatch([(500.0, 500.0, 31.5, 23.5)] * 2, flavour=2, halvings=1)
        assert len(tb) == 2 and tb.info("aligned") == 0 and tb.info("edge_passes") == 0
        tb.close()
        return
    with pytest.raises(capi.EAError) as ei:
        capi.TrackerBatch([(500.0, 500.0, 31.5, 23.5)] * 2)
    assert ei.value.code == capi.EA_ERR_NO_DEVICE                # no CPU fall-back
    with pytest.raises(capi.EAError) as ei:
        capi.TrackerBatch([], flavour=1)
    assert ei.value.code == capi.EA_ERR_INVALID_ARG


DOC_PROGRAM = r"""
#include <stddef.h>
#include "ea_hip.h"

/* N cameras of the node, 640 x 480 frames halved once: one push per set of frames, poses out */
int track(const ea_camera *cams, int n, const uint8_t *const *bgr, const void *const *depth_m, double *q, double *t,
          int *aligned, int64_t *bare) {
  ea_tracker_batch *tb;
  ea_options opt;
  int rc = ea_tracker_batch_create(&tb, cams, n, EA_F32, 0, 2, 1);
  if (rc != EA_OK) return rc;
  ea_default_options(&opt);
  rc = ea_problem_set_loss_auto_scale(ea_tracker_batch_problem(tb, 0), 3.536, 0.5, 1e-6);
  if (rc == EA_OK) rc = ea_tracker_batch_set_motion_prior(tb, 0.05, 0.2);
  if (rc == EA_OK) rc = ea_tracker_batch_push_frames(tb, bgr, depth_m, 480, 640, 0.0, &opt, q, t, NULL, aligned);
  if (rc == EA_OK) rc = ea_tracker_batch_get_info(tb, "frames_without_edges", bare);
  if (rc == EA_OK) rc = ea_tracker_batch_reset(tb, -1);
  ea_tracker_batch_destroy(tb);
  return rc;
}
"""


def test_documented_use_is_plain_c99(tmp_path):
    src = tmp_path / "tracker_batch_doc.c"
    src.write_text(DOC_PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-pedantic", "-fsyntax-only", "-I", INCLUDE, str(src)])
