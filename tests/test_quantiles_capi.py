"""CPU-side checks of the residual-quantile and auto-scale boundary: the new symbols are exported and bound by the stub, and
every argument check fails with EA_ERR_INVALID_ARG before anything touches a device (this box has none: a call that got as
far as the device would return EA_ERR_NO_DEVICE instead).  The setting's get / set round trip on a live problem needs a
device (ea_problem_create has no CPU form) and is in tests/test_gpu_quantiles.py; here the getters are checked on NULL and the
Python binding's packing on a stand-in library."""
import ctypes as C

import numpy as np
import pytest

NEW = ("ea_problem_residual_quantiles", "ea_batch_residual_quantiles", "ea_problem_get_loss", "ea_problem_set_loss_auto_scale",
       "ea_problem_get_loss_auto_scale", "ea_selftest_select")


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def test_new_symbols_exported_and_bound(lib):
    from edge_alignment_amd import capi
    for name in NEW:
        assert name in capi.EXPORTED and hasattr(lib, name)
    for name in ("residual_quantiles", "get_loss", "set_loss_auto_scale", "get_loss_auto_scale"):
        assert callable(getattr(capi.Problem, name))
    assert callable(capi.Batch.residual_quantiles) and callable(capi.selftest_select)


def _d(*v):
    return (C.c_double * len(v))(*v)


def test_quantile_arguments_are_checked_without_a_device(lib):
    from edge_alignment_amd import capi
    q, t, out = _d(1, 0, 0, 0), _d(0, 0, 0), _d(*([0.0] * 17))
    m = C.c_int64()
    h = C.c_void_p(1)  # (never dereferenced: the argument checks come first)
    ok = _d(0.5)
    for fn in (lib.ea_problem_residual_quantiles, lib.ea_batch_residual_quantiles):
        assert fn(None, q, t, ok, 1, out, C.byref(m)) == capi.EA_ERR_INVALID_ARG
        assert b"NULL" in lib.ea_last_error()
        assert fn(h, None, t, ok, 1, out, C.byref(m)) == capi.EA_ERR_INVALID_ARG
        assert fn(h, q, t, None, 1, out, C.byref(m)) == capi.EA_ERR_INVALID_ARG
        assert fn(h, q, t, ok, 1, None, C.byref(m)) == capi.EA_ERR_INVALID_ARG
        for nq in (0, 17, -1):
            assert fn(h, q, t, _d(*([0.5] * 17)), nq, out, C.byref(m)) == capi.EA_ERR_INVALID_ARG
            assert b"nq" in lib.ea_last_error()
        for bad in (-0.1, 1.1, float("nan"), float("inf")):
            assert fn(h, q, t, _d(0.5, bad), 2, out, C.byref(m)) == capi.EA_ERR_INVALID_ARG, bad
            assert b"prob" in lib.ea_last_error()
    off = (C.c_int64 * 2)(0, 1)
    v = _d(1.0)
    assert lib.ea_selftest_select(0, v, None, 1, ok, 1, out, None) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_selftest_select(0, v, off, 0, ok, 1, out, None) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_selftest_select(0, v, off, 1, ok, 17, out, None) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_selftest_select(0, v, off, 1, _d(1.5), 1, out, None) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_selftest_select(0, v, (C.c_int64 * 2)(1, 0), 1, ok, 1, out, None) == capi.EA_ERR_INVALID_ARG
    assert lib.ea_selftest_select(0, None, off, 1, ok, 1, out, None) == capi.EA_ERR_INVALID_ARG


def test_auto_scale_arguments_are_checked_before_the_problem(lib):
    """each check is seen by its message, on a NULL problem: the problem is looked at last"""
    from edge_alignment_amd import capi
    inf, nan = float("inf"), float("nan")
    cases = [((-1.0, 0.5, 1e-6), b"factor"), ((inf, 0.5, 1e-6), b"factor"), ((nan, 0.5, 1e-6), b"factor"),
             ((2.385, -0.1, 1e-6), b"prob"), ((2.385, 1.1, 1e-6), b"prob"), ((2.385, nan, 1e-6), b"prob"),
             ((2.385, 0.5, 0.0), b"a_min"), ((2.385, 0.5, -1.0), b"a_min"), ((2.385, 0.5, inf), b"a_min"), ((2.385, 0.5, nan), b"a_min"),
             ((2.385, 0.5, 1e-6), b"NULL problem"), ((0.0, 0.5, 1e-6), b"NULL problem")]
    for args, msg in cases:
        assert lib.ea_problem_set_loss_auto_scale(None, *args) == capi.EA_ERR_INVALID_ARG, args
        assert msg in lib.ea_last_error(), (args, lib.ea_last_error())
    f, p, a = C.c_double(), C.c_double(), C.c_double()
    assert lib.ea_problem_get_loss_auto_scale(None, C.byref(f), C.byref(p), C.byref(a)) == capi.EA_ERR_INVALID_ARG
    k = C.c_int()
    assert lib.ea_problem_get_loss(None, C.byref(k), C.byref(a)) == capi.EA_ERR_INVALID_ARG


def test_python_binding_round_trip_on_a_stand_in(monkeypatch):
    """Problem.set_loss_auto_scale / get_loss_auto_scale / get_loss hand their arguments through unchanged (defaults prob =
    0.5, a_min = 1e-6) and unpack the getters' outputs"""
    from edge_alignment_amd import capi

    class Stand:
        stored = None

        def ea_problem_set_loss_auto_scale(self, h, f, p, a):
            Stand.stored = (f, p, a)
            return 0

        def ea_problem_get_loss_auto_scale(self, h, f, p, a):
            f._obj.value, p._obj.value, a._obj.value = Stand.stored
            return 0

        def ea_problem_get_loss(self, h, k, a):
            k._obj.value, a._obj.value = 2, 0.75
            return 0

    monkeypatch.setattr(capi, "load", lambda: Stand())
    P = capi.Problem.__new__(capi.Problem)
    P._h = C.c_void_p()
    P.set_loss_auto_scale(2.385)
    assert P.get_loss_auto_scale() == (2.385, 0.5, 1e-6)
    P.set_loss_auto_scale(1.994, prob=0.25, a_min=1e-3)
    assert P.get_loss_auto_scale() == (1.994, 0.25, 1e-3)
    assert P.get_loss() == (2, 0.75)


def test_selftest_binding_reaches_the_device_check():
    """well-formed arguments pass every check: without a device the call ends in EA_ERR_NO_DEVICE (no CPU fallback), with one
    it returns the order statistic"""
    from edge_alignment_amd import capi
    if capi.device_count() == 0:
        with pytest.raises(capi.EAError) as ei:
            capi.selftest_select(np.array([1.0, 2.0]), [0, 2], [0.5])
        assert ei.value.code == -3  # EA_ERR_NO_DEVICE
    else:
        out, m = capi.selftest_select(np.array([3.0, -1.0, 2.0]), [0, 3], [0.5])
        assert out[0, 0] == 2.0 and m[0] == 3
