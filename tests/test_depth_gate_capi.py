"""The depth gate section of include/ea_hip.h through the loaded library, without a GPU: ea_*_set_now_depth* and
ea_*_depth_gate* refuse their bad arguments with EA_ERR_INVALID_ARG (-1) before a handle is looked at or a device is looked
for (the handle given is a word that must stay untouched), the defaults are the documented ones, and the stub's structs are
laid out as the C compiler lays out the header's.  (What depends on a real problem -- a capacity that is too small, a weight
factor that overflows the float of an fp32 problem, a bad matrix in a real batch -- is refused in tests/test_gpu_depth_gate.py;
the batch forms read their count x 16 matrices by the batch's problem count, so here they get a bad parameter block or NULLs.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import reproject_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
DP = C.POINTER(C.c_double)
BAD_VALUES = (-1e-300, -1.0, float("nan"), float("inf"), -float("inf"))


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def _fake_handle():
    """a non-NULL handle that must not be looked at: the word behind it stays 0"""
    word = C.c_uint64(0)
    return word, C.cast(C.pointer(word), C.c_void_p)


def _bad_params():
    from edge_alignment_amd import capi
    out = [capi.default_depth_gate_params(radius=r) for r in (-1, 4, 1000)]
    for field in ("abs_tol", "rel_tol", "w_occluded", "w_free", "w_unknown"):
        out += [capi.default_depth_gate_params(**{field: v}) for v in BAD_VALUES]
    return out


def test_defaults_are_the_documented_ones(lib):
    from edge_alignment_amd import capi
    prm = capi.DepthGateParams(radius=9, abs_tol=9, rel_tol=9, w_occluded=9, w_free=9, w_unknown=9, apply=9)
    lib.ea_default_depth_gate_params(C.byref(prm))
    assert (prm.radius, prm.abs_tol, prm.rel_tol, prm.w_occluded, prm.w_free, prm.w_unknown, prm.apply) == (1, 0.02, 0.02, 0.0, 0.0, 1.0, 1)
    lib.ea_default_depth_gate_params(None)              # like free(NULL)
    assert (capi.EA_DEPTH_U16, capi.EA_DEPTH_F32) == (0, 1)
    assert (capi.GATE_BEHIND, capi.GATE_OUTSIDE, capi.GATE_UNKNOWN, capi.GATE_CONSISTENT, capi.GATE_OCCLUDED, capi.GATE_FREE) == tuple(range(6))


def test_set_now_depth_refuses_bad_arguments_without_a_device(lib):
    from edge_alignment_amd import capi
    word, h = _fake_handle()
    img = np.zeros((5, 7), np.uint16)
    ip = img.ctypes.data_as(C.c_void_p)
    arr = (C.c_void_p * 1)(img.ctypes.data)
    E = capi.EA_ERR_INVALID_ARG
    bad = [(2, 5, 7, 5000.0), (-1, 5, 7, 5000.0), (0, 2, 7, 5000.0), (0, 5, 2, 5000.0), (1, 32769, 7, 1.0), (1, 5, 32769, 1.0),
           (0, 0, 0, 5000.0), (0, 5, 7, 0.0), (0, 5, 7, -5000.0), (0, 5, 7, float("nan")), (0, 5, 7, float("inf"))]
    for fn, first in ((lib.ea_problem_set_now_depth, ip), (lib.ea_problem_set_now_depth_device, ip),
                      (lib.ea_batch_set_now_depth, arr), (lib.ea_batch_set_now_depth_device, arr)):
        assert fn(None, first, 0, 5, 7, 5000.0) == E and b"NULL" in lib.ea_last_error()
        for kind, height, width, zs in bad:
            assert fn(h, first, kind, height, width, zs) == E, (kind, height, width, zs)
    assert b"z_scaling" in lib.ea_last_error()
    assert E == -1 and word.value == 0 and not img.any()


def test_depth_gate_refuses_bad_arguments_without_a_device(lib):
    from edge_alignment_amd import capi
    word, h = _fake_handle()
    good = rr.pose_to_matrix([1.0, 0, 0, 0], [0.0, 0, 0])
    g = good.ctypes.data_as(DP)
    prm = capi.default_depth_gate_params()
    pp = C.byref(prm)
    cls = np.zeros(4, np.uint8)
    cp = cls.ctypes.data_as(C.c_void_p)
    st = capi.DepthGateStats()
    sp = C.byref(st)
    E = capi.EA_ERR_INVALID_ARG
    # NULL arguments (cls is nullable everywhere, stats in the batch forms)
    assert lib.ea_problem_depth_gate(None, g, pp, cp, 4, sp) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_problem_depth_gate(h, None, pp, cp, 4, sp) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_problem_depth_gate(h, g, None, cp, 4, sp) == E and b"NULL" in lib.ea_last_error()
    assert lib.ea_problem_depth_gate(h, g, pp, cp, 4, None) == E and b"NULL" in lib.ea_last_error()
    for fn in (lib.ea_batch_depth_gate, lib.ea_batch_depth_gate_device):
        assert fn(None, g, pp, cp, 4, sp) == E and b"NULL" in lib.ea_last_error()
        assert fn(h, None, pp, cp, 4, sp) == E and b"NULL" in lib.ea_last_error()
        assert fn(h, g, None, cp, 4, sp) == E and b"NULL" in lib.ea_last_error()
    # a matrix that ea_*_reproject refuses
    for idx, val in (((3, 3), 2.0), ((3, 0), 1.0), ((3, 2), 1e-300), ((0, 1), float("nan")), ((2, 3), float("inf")), ((3, 1), float("nan"))):
        m = good.copy()
        m[idx] = val
        assert lib.ea_problem_depth_gate(h, m.ctypes.data_as(DP), pp, cp, 4, sp) == E and b"0 0 0 1" in lib.ea_last_error()
    # radius, tolerances, weight factors: every form, before its handle is looked at
    for bad in _bad_params():
        for fn in (lib.ea_problem_depth_gate, lib.ea_batch_depth_gate, lib.ea_batch_depth_gate_device):
            assert fn(h, g, C.byref(bad), cp, 4, sp) == E, (bad.radius, bad.abs_tol, bad.rel_tol, bad.w_occluded, bad.w_free, bad.w_unknown)
    assert E == -1 and word.value == 0 and not cls.any() and st.n == 0


def test_the_stub_lays_the_structs_out_as_the_c_compiler_does(tmp_path):
    from edge_alignment_amd import capi
    lines = ["#include <stddef.h>", "#include <stdio.h>", '#include "ea_hip.h"', "int main(void) {"]
    want = []
    for cname, st in (("ea_depth_gate_params", capi.DepthGateParams), ("ea_depth_gate_stats", capi.DepthGateStats)):
        lines.append('  printf("sizeof %%zu\\n", sizeof(%s));' % cname)
        want.append(["sizeof", str(C.sizeof(st))])
        for f, _ in st._fields_:
            lines.append('  printf("%s %%zu\\n", offsetof(%s, %s));' % (f, cname, f))
            want.append([f, str(getattr(st, f).offset)])
    lines += ['  printf("enums %d %d %d %d\\n", EA_DEPTH_U16, EA_DEPTH_F32, EA_GATE_BEHIND, EA_GATE_FREE);', "  return 0;", "}"]
    src, exe = tmp_path / "gate_layout.c", tmp_path / "gate_layout"
    src.write_text("\n".join(lines) + "\n")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", INCLUDE, "-o", str(exe), str(src)])
    got = [ln.split() for ln in subprocess.check_output([str(exe)], text=True).splitlines()]
    assert got == want + [["enums", "0", "1", "0", "5"]]
    assert C.sizeof(capi.DepthGateParams) == 56 and C.sizeof(capi.DepthGateStats) == 56
