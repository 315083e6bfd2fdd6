"""The boundary of the batched frame producers without a GPU: ea_batch_set_frames, ea_batch_set_frames_device and
ea_default_frame_params are declared in include/ea_hip.h and bound by the ctypes stub, refuse missing arguments before any
device is looked for, and the call as the header documents it is plain C99."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ea_default_frame_params", "ea_batch_set_frames", "ea_batch_set_frames_device")


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def test_header_and_stub_declare_the_calls(lib):
    from edge_alignment_amd import capi
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ea_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in capi.EXPORTED, name
        assert hasattr(lib, name), name
    assert "ea_frame_params" in text
    # the struct as the C compiler lays it out: 2 ints, a double, 4 ints
    assert C.sizeof(capi.FrameParams) == 32
    assert [f[0] for f in capi.FrameParams._fields_] == ["height", "width", "z_scaling", "ref_threshold", "now_threshold",
                                                         "now_median", "now_normalize"]


def test_default_frame_params(lib):
    from edge_alignment_amd import capi
    prm = capi.FrameParams()
    lib.ea_default_frame_params(C.byref(prm), 480, 640)
    assert (prm.height, prm.width, prm.z_scaling) == (480, 640, 5000.0)
    assert (prm.ref_threshold, prm.now_threshold, prm.now_median, prm.now_normalize) == (35, 35, 1, 1)
    lib.ea_default_frame_params(None, 480, 640)   # like free(NULL)


@pytest.mark.parametrize("name", NAMES[1:])
def test_missing_arguments_are_refused_without_a_device(lib, name):
    from edge_alignment_amd import capi
    fn = getattr(lib, name)
    prm = capi.FrameParams()
    lib.ea_default_frame_params(C.byref(prm), 480, 640)
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

/* N frame pairs of one extent -> points and DT images of the N problems of `b`, then one solve for all of them */
int align_pairs(ea_batch *b, const uint8_t *const *ref_bgr, const uint16_t *const *ref_depth, const uint8_t *const *now_bgr,
                int height, int width, double *q, double *t, ea_summary *summaries) {
  ea_frame_params prm;
  ea_options opt;
  int rc;
  ea_default_frame_params(&prm, height, width);
  prm.now_median = 1;
  rc = ea_batch_set_frames(b, ref_bgr, ref_depth, now_bgr, &prm);
  if (rc != EA_OK) return rc;
  ea_default_options(&opt);
  return ea_batch_solve(b, &opt, q, t, summaries);
}

/* the same from frames a decoder left in device memory; only the current frames change from pair to pair */
int next_frames_on_device(ea_batch *b, const uint8_t *const *now_bgr_dev, int height, int width) {
  ea_frame_params prm;
  ea_default_frame_params(&prm, height, width);
  return ea_batch_set_frames_device(b, NULL, NULL, now_bgr_dev, &prm);
}
"""


def test_documented_use_is_plain_c99(tmp_path):
    src = tmp_path / "batch_frames_doc.c"
    src.write_text(DOC_PROGRAM)
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), str(src)])
