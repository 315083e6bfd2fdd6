"""ea_batch_solve_starts / ea_solve_starts at the C boundary, without a device: both are exported, reject missing arguments
and an out-of-range K before they touch a handle or a device, answer EA_ERR_NO_DEVICE like every compute entry point, and a
C99 translation unit that calls both compiles under -Wall -Werror."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def test_exports_and_argument_checks(lib):
    from edge_alignment_amd import capi
    assert "ea_batch_solve_starts" in capi.EXPORTED and "ea_solve_starts" in capi.EXPORTED
    q = (C.c_double * 8)(1, 0, 0, 0, 1, 0, 0, 0)
    t = (C.c_double * 6)()
    dummy = C.c_void_p(8)   # never dereferenced: the checks below come first
    for fn in (lib.ea_batch_solve_starts, lib.ea_solve_starts):
        assert fn(None, 2, None, q, t, None, None) == capi.EA_ERR_INVALID_ARG
        assert b"NULL" in lib.ea_last_error()
        assert fn(dummy, 2, None, None, t, None, None) == capi.EA_ERR_INVALID_ARG
        assert fn(dummy, 2, None, q, None, None, None) == capi.EA_ERR_INVALID_ARG
        for K in (0, -3, 16385):                    # K x count <= 16384 cannot hold for any count >= 1
            assert fn(dummy, K, None, q, t, None, None) == capi.EA_ERR_INVALID_ARG
            assert b"16384" in lib.ea_last_error()


def test_no_device_no_fallback(lib):
    from edge_alignment_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a gfx950 device is visible; the no-device path is exercised on the CPU box")
    q = (C.c_double * 4)(1, 0, 0, 0)
    t = (C.c_double * 3)()
    dummy = C.c_void_p(8)
    best = C.c_int(7)
    assert lib.ea_batch_solve_starts(dummy, 1, None, q, t, None, C.byref(best)) == capi.EA_ERR_NO_DEVICE
    assert lib.ea_solve_starts(dummy, 1, None, q, t, None, C.byref(best)) == capi.EA_ERR_NO_DEVICE
    assert b"device" in lib.ea_last_error() and best.value == 7


def test_c99_caller_compiles(tmp_path):
    src = tmp_path / "starts.c"
    src.write_text(r'''#include "ea_hip.h"
int run(ea_batch *b, ea_problem *p) {
  double q[2 * 4] = {1, 0, 0, 0, 1, 0, 0, 0}, t[2 * 3] = {0, 0, 0, 0.01, 0, 0};
  ea_summary s[2];
  ea_options o;
  int best = -1, rc;
  ea_default_options(&o);
  rc = ea_batch_solve_starts(b, 2, &o, q, t, s, &best);
  if (rc != EA_OK) return rc;
  return ea_solve_starts(p, 2, 0, q, t, 0, 0);
}
''')
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-c", str(src), "-o", str(tmp_path / "starts.o")])
