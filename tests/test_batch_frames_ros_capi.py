"""The boundary of the batched ROS producers without a GPU: ea_batch_set_frames_ros, ea_batch_set_frames_ros_device and
ea_default_ros_frame_params are declared in include/ea_hip.h and bound by the ctypes stub, the stub's RosFrameParams is laid
out as a C compiler lays out the header's struct, missing arguments are refused before any device is looked for, and the
call as the header documents it is plain C99."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NAMES = ("ea_default_ros_frame_params", "ea_batch_set_frames_ros", "ea_batch_set_frames_ros_device")
FIELDS = ("full_height", "full_width", "halvings", "threshold1", "threshold2")


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
    assert "ea_ros_frame_params" in text


LAYOUT_PROGRAM = r"""
#include <stddef.h>
#include <stdio.h>
#include "ea_hip.h"
int main(void) {
  printf("sizeof %zu\n", sizeof(ea_ros_frame_params));
@FIELDS@
  return 0;
}
""".replace("@FIELDS@", "\n".join('  printf("%s %%zu\\n", offsetof(ea_ros_frame_params, %s));' % (f, f) for f in FIELDS))


def test_the_stub_lays_the_params_out_as_the_c_compiler_does(tmp_path):
    from edge_alignment_amd import capi
    src, exe = tmp_path / "ros_params_layout.c", tmp_path / "ros_params_layout"
    src.write_text(LAYOUT_PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    lines = [ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert lines[0][0] == "sizeof" and int(lines[0][1]) == C.sizeof(capi.RosFrameParams)
    # the header's field order is the order of the offsets the program printed, and the stub's
    assert [ln[0] for ln in lines[1:]] == list(FIELDS) == [f[0] for f in capi.RosFrameParams._fields_]
    offsets = [int(ln[1]) for ln in lines[1:]]
    assert offsets == sorted(offsets)
    assert offsets == [getattr(capi.RosFrameParams, f).offset for f in FIELDS]


def test_default_ros_frame_params(lib):
    from edge_alignment_amd import capi
    prm = capi.RosFrameParams()
    lib.ea_default_ros_frame_params(C.byref(prm), 480, 640)
    assert (prm.full_height, prm.full_width, prm.halvings, prm.threshold1, prm.threshold2) == (480, 640, 0, 150.0, 100.0)
    lib.ea_default_ros_frame_params(None, 480, 640)   # like free(NULL)


@pytest.mark.parametrize("name", NAMES[1:])
def test_missing_arguments_are_refused_without_a_device(lib, name):
    from edge_alignment_amd import capi
    fn = getattr(lib, name)
    prm = capi.RosFrameParams()
    lib.ea_default_ros_frame_params(C.byref(prm), 480, 640)
    one = (C.c_void_p * 1)()
    assert fn(None, one, one, one, C.byref(prm)) == capi.EA_ERR_INVALID_ARG
    assert b"NULL" in lib.ea_last_error()
    # NULL params: refused before the batch is looked at (any non-NULL handle will do)
    word = C.c_uint64(0)
    assert fn(C.cast(C.pointer(word), C.c_void_p), one, one, one, None) == capi.EA_ERR_INVALID_ARG
    assert word.value == 0


DOC_PROGRAM = r"""
#include <stddef.h>
#include "ea_hip.h"

/* N frame pairs as the ROS callbacks receive them (640 x 480) -> points and DT images of the N problems of `b` at the node's
 * 320 x 240, then one solve for all of them; *bare: current frames that had no edge (their problems keep the image they had) */
int align_pairs_ros(ea_batch *b, const uint8_t *const *ref_bgr, const float *const *ref_depth, const uint8_t *const *now_bgr,
                    int full_height, int full_width, double *q, double *t, ea_summary *summaries, int64_t *bare) {
  ea_ros_frame_params prm;
  ea_options opt;
  int rc, rc_info;
  ea_default_ros_frame_params(&prm, full_height, full_width);
  prm.halvings = 1; /* ea.cpp: cv::resize(..., 0.5, 0.5) */
  rc = ea_batch_set_frames_ros(b, ref_bgr, ref_depth, now_bgr, &prm);
  rc_info = ea_batch_get_info(b, "frames_without_edges", bare);
  if (rc != EA_OK && rc != EA_ERR_STATE) return rc;
  if (rc_info != EA_OK) return rc_info;
  if (rc == EA_ERR_STATE) return rc; /* ea_last_error() names the first edge-less frame */
  ea_default_options(&opt);
  return ea_batch_solve(b, &opt, q, t, summaries);
}

/* the same from frames a decoder left in device memory; only the current frames change from pair to pair */
int next_frames_on_device_ros(ea_batch *b, const uint8_t *const *now_bgr_dev, int full_height, int full_width) {
  ea_ros_frame_params prm;
  ea_default_ros_frame_params(&prm, full_height, full_width);
  prm.halvings = 1;
  prm.threshold1 = 150.0;
  prm.threshold2 = 100.0;
  return ea_batch_set_frames_ros_device(b, NULL, NULL, now_bgr_dev, &prm);
}
"""


def test_documented_use_is_plain_c99(tmp_path):
    src = tmp_path / "batch_frames_ros_doc.c"
    src.write_text(DOC_PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", INCLUDE, str(src)])
