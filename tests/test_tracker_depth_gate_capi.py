"""ea_tracker_batch_set_depth_gate / ea_tracker_batch_last_depth_gate through the loaded library, without a GPU: the symbols
are exported, edge_alignment_amd/capi.py binds them as include/ea_hip.h declares them (a C translation unit assigns them to
function pointers of the expected types), and bad arguments -- a NULL handle, a NULL `out`, a negative stream or level, every
parameter error of ea_batch_depth_gate -- are EA_ERR_INVALID_ARG (-1) before the handle is looked at or a device is looked for
(the handle given is a word that must stay untouched).  What needs a real tracker -- a stream or level past the end, the state
rule, a factor that overflows the float of an fp32 tracker -- is in tests/test_gpu_tracker_depth_gate.py."""
import ctypes as C
import os
import subprocess

import pytest

from test_depth_gate_capi import _bad_params, _fake_handle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
NEW = ("ea_tracker_batch_set_depth_gate", "ea_tracker_batch_last_depth_gate")


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def test_the_symbols_are_exported_and_bound_as_declared(lib, tmp_path):
    from edge_alignment_amd import build, capi
    dynamic = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB], text=True)
    for name in NEW:
        assert name in capi.EXPORTED and (" T " + name + "\n") in dynamic, name
    vp = C.c_void_p
    assert lib.ea_tracker_batch_set_depth_gate.argtypes == [vp, C.POINTER(capi.DepthGateParams)]
    assert lib.ea_tracker_batch_last_depth_gate.argtypes == [vp, C.c_int, C.c_int, C.POINTER(capi.DepthGateStats)]
    src = tmp_path / "decl.c"
    src.write_text('#include "ea_hip.h"\n'
                   "int (*set_gate)(ea_tracker_batch *, const ea_depth_gate_params *) = ea_tracker_batch_set_depth_gate;\n"
                   "int (*last_gate)(ea_tracker_batch *, int, int, ea_depth_gate_stats *) = ea_tracker_batch_last_depth_gate;\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-c", "-o",
                           str(tmp_path / "decl.o"), str(src)])
    assert hasattr(capi.TrackerBatch, "set_depth_gate") and hasattr(capi.TrackerBatch, "last_depth_gate")


def test_bad_arguments_are_refused_before_the_handle_or_a_device_is_looked_at(lib):
    from edge_alignment_amd import capi
    word, h = _fake_handle()
    E = capi.EA_ERR_INVALID_ARG
    good = capi.default_depth_gate_params()
    st = capi.DepthGateStats(n=7)
    assert lib.ea_tracker_batch_set_depth_gate(None, C.byref(good)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_tracker_batch_set_depth_gate(None, None) == E and b"NULL" in lib.ea_last_error()
    for bad in _bad_params():
        where = (bad.radius, bad.abs_tol, bad.rel_tol, bad.w_occluded, bad.w_free, bad.w_unknown)
        assert lib.ea_tracker_batch_set_depth_gate(h, C.byref(bad)) == E, where
        assert b"NULL" not in lib.ea_last_error(), where
        assert lib.ea_tracker_batch_set_depth_gate(None, C.byref(bad)) == E and b"NULL" not in lib.ea_last_error(), where
    assert lib.ea_tracker_batch_last_depth_gate(None, 0, 0, C.byref(st)) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_tracker_batch_last_depth_gate(h, 0, 0, None) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_tracker_batch_last_depth_gate(h, -1, 0, C.byref(st)) == E and b"level" in lib.ea_last_error()
    assert lib.ea_tracker_batch_last_depth_gate(h, 0, -1, C.byref(st)) == E and b"stream" in lib.ea_last_error()
    assert E == -1 and word.value == 0 and st.n == 7


def test_creating_a_tracker_still_asks_for_a_device(lib):
    """EA_ERR_NO_DEVICE where there is none, as before; with one the tracker reports the gate off"""
    from edge_alignment_amd import capi
    h = C.c_void_p()
    cam = (capi.Camera * 1)(capi.Camera(50.0, 50.0, 32.0, 24.0))
    rc = lib.ea_tracker_batch_create(C.byref(h), cam, 1, capi.EA_F64, 0, 0, 0)
    assert rc in (capi.EA_OK, capi.EA_ERR_NO_DEVICE)
    if rc == capi.EA_OK:
        v = C.c_int64(-1)
        assert lib.ea_tracker_batch_get_info(h, b"depth_gate", C.byref(v)) == capi.EA_OK and v.value == 0
        assert lib.ea_tracker_batch_get_info(h, b"gated", C.byref(v)) == capi.EA_OK and v.value == 0
        lib.ea_tracker_batch_destroy(h)
    else:
        assert not h
