"""keyframe_decide (edge_alignment_amd/csrc/ea_keyframe.h), the host function behind the tracker's keyframe mode, against the
restatement of the header's rule in tests/keyframe_rule.py: tests/keyframe_host_shim.cpp built with the host compiler and
loaded with ctypes, no device.  The grid holds equality on every threshold (a fraction times n that is exact, and one that is
not), one count either side of it, n_flow == 0, every rule off (0 and negative), ages around max_frames, and the unaligned
and failed-solve cases, alone and in every combination of the four rules."""
import ctypes as C
import itertools
import os
import subprocess

import pytest

from keyframe_rule import KEY_AGE, KEY_FIRST, KEY_FLOW, KEY_INLIERS, KEY_SOLVE_FAILED, KEY_VISIBLE, keyframe_decide

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "keyframe_host.so")
    src = os.path.join(ROOT, "tests", "keyframe_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_keyframe.h"), os.path.join(ROOT, "include", "ea_hip.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-shared", "-fPIC", "-I", csrc,
                               "-o", so, src])
    return C.CDLL(so)


def _call(shim, stats, params, age, aligned, failed):
    from edge_alignment_amd import capi
    s = capi.PoseStats(**stats)
    p = capi.KeyframeParams(**params)
    return shim.keyframe_decide_c(C.byref(s), C.byref(p), age, int(aligned), int(failed))


OFF = dict(min_visible_fraction=0.0, min_inlier_fraction=0.0, inlier_residual=0.0, max_mean_flow=0.0, max_frames=0, margin=0)


def _stats(n=1000, n_invalid=0, n_visible=0, n_inlier=0, n_flow=0, sum_flow=0.0):
    return dict(n=n, n_invalid=n_invalid, n_visible=n_visible, n_inlier=n_inlier, n_flow=n_flow, sum_flow=sum_flow)


def test_grid_against_the_restatement(shim):
    checked, seen = 0, set()
    fractions = [0.75, 0.3, 1.0, 1e-9, 0.0, -0.5]          # 0.75 * 1000 is exact, 0.3 * 1001 is not
    for n in (1, 7, 1000, 1001, 123457):
        for fv, fi in itertools.product(fractions, repeat=2):
            counts_v = sorted({0, n, *(max(0, min(n, int(fv * n) + d)) for d in (-1, 0, 1))})
            counts_i = sorted({0, *(max(0, min(n, int(fi * n) + d)) for d in (-1, 0, 1))})
            for nv, ni in itertools.product(counts_v, counts_i):
                for max_flow, n_flow, sum_flow in ((0.0, 5, 1e9), (-1.0, 5, 1e9), (2.5, 0, 1e9), (2.5, 4, 10.0), (2.5, 4, 10.000000000000002),
                                                   (2.5, 4, 9.999999999999998), (0.1, 3, 0.30000000000000004), (0.1, 3, 0.3)):
                    for max_frames, age in ((0, 100), (-1, 100), (3, 2), (3, 3), (3, 4), (1, 1)):
                        prm = dict(OFF, min_visible_fraction=fv, min_inlier_fraction=fi, max_mean_flow=max_flow, max_frames=max_frames)
                        st = _stats(n=n, n_visible=nv, n_inlier=ni, n_flow=n_flow, sum_flow=sum_flow)
                        want = keyframe_decide(st, prm, age, True, False)
                        assert _call(shim, st, prm, age, True, False) == want, (st, prm, age)
                        seen.add(want)
                        checked += 1
    assert checked > 50000
    # every combination of the four rule bits occurs, 0 (keep) among them
    assert seen == {v | i | f | a for v in (0, KEY_VISIBLE) for i in (0, KEY_INLIERS) for f in (0, KEY_FLOW) for a in (0, KEY_AGE)}


def test_equality_keeps_and_one_less_replaces(shim):
    prm = dict(OFF, min_visible_fraction=0.75, min_inlier_fraction=0.5, max_mean_flow=2.5, max_frames=4)
    at = _stats(n=1000, n_visible=750, n_inlier=500, n_flow=4, sum_flow=10.0)
    assert _call(shim, at, prm, 3, True, False) == 0
    assert _call(shim, dict(at, n_visible=749), prm, 3, True, False) == KEY_VISIBLE
    assert _call(shim, dict(at, n_inlier=499), prm, 3, True, False) == KEY_INLIERS
    assert _call(shim, dict(at, sum_flow=10.000000000000002), prm, 3, True, False) == KEY_FLOW
    assert _call(shim, at, prm, 4, True, False) == KEY_AGE
    assert _call(shim, dict(at, n_visible=0, n_inlier=0, sum_flow=1e9), prm, 9, True, False) == KEY_VISIBLE | KEY_INLIERS | KEY_FLOW | KEY_AGE
    # n_flow == 0: no mean to compare; every rule off: nothing replaces
    assert _call(shim, dict(at, n_flow=0, sum_flow=1e9), prm, 3, True, False) == 0
    assert _call(shim, _stats(n=1000), OFF, 10 ** 6, True, False) == 0


def test_unaligned_and_failed_streams(shim):
    prm = dict(OFF, min_visible_fraction=0.75, max_frames=1)
    for st in (_stats(), _stats(n_visible=1000)):
        assert _call(shim, st, prm, 1, False, False) == KEY_FIRST == keyframe_decide(st, prm, 1, False, False)
        assert _call(shim, st, prm, 1, False, True) == KEY_FIRST == keyframe_decide(st, prm, 1, False, True)
        assert _call(shim, st, prm, 1, True, True) == KEY_SOLVE_FAILED == keyframe_decide(st, prm, 1, True, True)


def test_params_ok(shim):
    from edge_alignment_amd import capi
    nan = float("nan")
    assert shim.keyframe_params_ok_c(C.byref(capi.KeyframeParams(**OFF))) == 1
    assert shim.keyframe_params_ok_c(C.byref(capi.KeyframeParams(**dict(OFF, inlier_residual=float("inf"), min_visible_fraction=-3.0)))) == 1
    for f in ("min_visible_fraction", "min_inlier_fraction", "inlier_residual", "max_mean_flow"):
        assert shim.keyframe_params_ok_c(C.byref(capi.KeyframeParams(**dict(OFF, **{f: nan})))) == 0
    assert shim.keyframe_params_ok_c(C.byref(capi.KeyframeParams(**dict(OFF, margin=-1)))) == 0
    assert shim.keyframe_params_ok_c(C.byref(capi.KeyframeParams(**dict(OFF, inlier_residual=-1.0)))) == 0
