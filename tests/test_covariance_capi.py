"""CPU side of the covariance entry points (include/ea_hip.h, ceres::Covariance): exported, argument checks before any
device is touched, EA_ERR_NO_DEVICE without one, and a Ceres-documentation-style program compiles against the facade."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["ea_default_covariance_options", "ea_problem_covariance", "ea_batch_covariance", "ea_tracker_set_covariance",
         "ea_tracker_last_covariance"]


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def test_covariance_symbols_exported(lib):
    from edge_alignment_amd import capi
    for name in NAMES:
        assert name in capi.EXPORTED and hasattr(lib, name), name


def test_struct_sizes_and_defaults(lib):
    from edge_alignment_amd import capi
    assert C.sizeof(capi.CovarianceOptions) == 24
    assert C.sizeof(capi.Covariance) == 3 * 4 + 4 + 8 + 8 + (6 + 36 + 16 + 12 + 9) * 8
    o = capi.covariance_options()
    assert (o.algorithm, o.min_reciprocal_condition_number, o.null_space_rank, o.apply_loss_function) == (capi.COV_SPARSE_QR, 1e-14, 0, 1)
    assert capi.covariance_options(algorithm="dense_svd", null_space_rank=-1).algorithm == capi.COV_DENSE_SVD


def test_argument_validation_needs_no_device(lib):
    from edge_alignment_amd import capi
    q = (C.c_double * 4)(1, 0, 0, 0)
    t = (C.c_double * 3)()
    out = capi.Covariance()
    dummy = C.create_string_buffer(64)  # never dereferenced: the arguments are rejected first
    good = capi.covariance_options()
    for fn in (lib.ea_problem_covariance, lib.ea_batch_covariance):
        assert fn(None, q, t, C.byref(good), C.byref(out)) == -1
        assert fn(dummy, None, t, C.byref(good), C.byref(out)) == -1
        assert fn(dummy, q, None, C.byref(good), C.byref(out)) == -1
        assert fn(dummy, q, t, None, C.byref(out)) == -1
        assert fn(dummy, q, t, C.byref(good), None) == -1
        for bad in (capi.covariance_options(algorithm=2), capi.covariance_options(algorithm=-1),
                    capi.covariance_options(null_space_rank=-2), capi.covariance_options(null_space_rank=7),
                    capi.covariance_options(min_reciprocal_condition_number=-1e-3)):
            assert fn(dummy, q, t, C.byref(bad), C.byref(out)) == -1
    nan = capi.covariance_options()
    nan.min_reciprocal_condition_number = float("nan")
    assert lib.ea_problem_covariance(dummy, q, t, C.byref(nan), C.byref(out)) == -1
    assert lib.ea_tracker_set_covariance(None, C.byref(good)) == -1
    assert lib.ea_tracker_set_covariance(None, None) == -1
    assert lib.ea_tracker_last_covariance(None, C.byref(out)) == -1
    lib.ea_default_covariance_options(None)  # like free(NULL)


def test_no_device_without_a_gpu(lib):
    from edge_alignment_amd import capi
    if capi.device_count() > 0:
        pytest.skip("a gfx950 device is visible; the no-device path is exercised on the CPU box")
    q = (C.c_double * 4)(1, 0, 0, 0)
    t = (C.c_double * 3)()
    out = capi.Covariance()
    dummy = C.create_string_buffer(64)
    o = capi.covariance_options()
    assert lib.ea_problem_covariance(dummy, q, t, C.byref(o), C.byref(out)) == -3
    assert lib.ea_batch_covariance(dummy, q, t, C.byref(o), C.byref(out)) == -3


def test_ceres_style_program_compiles(lib, tmp_path):
    """Solve, then Covariance::Options, Compute on (q,q), (q,t), (t,t) and both Get... forms: -std=c++14 -Wall -Werror"""
    from edge_alignment_amd import capi
    lib_dir = os.path.dirname(capi.LIB_PATH)
    exe = str(tmp_path / "covariance_example")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "edge_alignment_amd", "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "covariance_example.cpp"),
                           "-L", lib_dir, "-lea_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    assert os.path.exists(exe)


def test_covariance_header_stands_alone(tmp_path):
    """ceres/covariance.h included first (before ceres.h) compiles too"""
    src = tmp_path / "inc.cpp"
    src.write_text('#include "ceres/covariance.h"\nint main() { ceres::Covariance::Options o; ceres::Covariance c(o);\n'
                   '  return o.algorithm_type == ceres::SPARSE_QR && ceres::SUITE_SPARSE_QR == ceres::SPARSE_QR ? 0 : 1; }\n')
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "edge_alignment_amd", "include"),
                           "-c", str(src), "-o", str(tmp_path / "inc.o")])
