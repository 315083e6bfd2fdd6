"""CPU-side checks of the NormalPrior boundary: the new symbols are exported and bound by the stub, argument checks fail
with EA_ERR_INVALID_ARG before any device work, and the facade program compiles against edge_alignment_amd/include with
the facade's ceres::Matrix / Vector and with an Eigen-like stand-in."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ea_problem_set_normal_prior", "ea_tracker_set_motion_prior")


@pytest.fixture(scope="module")
def lib():
    from edge_alignment_amd import build_library, capi
    build_library()
    return capi.load()


def test_new_symbols_exported_and_bound(lib):
    from edge_alignment_amd import capi
    for name in NEW:
        assert name in capi.EXPORTED and hasattr(lib, name)
    for name in ("set_normal_prior", "clear_normal_prior"):
        assert callable(getattr(capi.Problem, name))
    assert callable(capi.Tracker.set_motion_prior)


def test_argument_checks_without_a_device(lib):
    """every argument check comes before the problem is looked at: each one is seen here by its message"""
    from edge_alignment_amd import capi
    A = (C.c_double * 16)(*([1.0] * 16))
    b = (C.c_double * 4)()
    bad_A = (C.c_double * 16)(*([1.0] * 15 + [float("nan")]))
    bad_b = (C.c_double * 4)(0.0, float("inf"), 0.0, 0.0)
    cases = [((2, A, 4, b), b"block"), ((-1, A, 4, b), b"block"), ((0, A, -1, b), b"k must be"),
             ((0, bad_A, 4, b), b"A must be finite"), ((1, A, 3, bad_b), b"b must be finite"),
             ((0, A, 4, None), b"b must not be NULL"), ((0, A, 4, b), b"NULL problem"), ((1, None, 0, None), b"NULL problem")]
    for args, msg in cases:
        assert lib.ea_problem_set_normal_prior(None, *args) == capi.EA_ERR_INVALID_ARG, args
        assert msg in lib.ea_last_error(), (args, lib.ea_last_error())
    assert lib.ea_tracker_set_motion_prior(None, 0.1, 0.1) == capi.EA_ERR_INVALID_ARG


def test_python_binding_checks_shapes():
    from edge_alignment_amd import capi
    P = capi.Problem.__new__(capi.Problem)  # (no device: the shape checks come before the library is called)
    P._h = C.c_void_p()
    for block, A, b in ((1, np.eye(2, 6), np.zeros(3)), (0, np.eye(4), np.zeros(3)), (1, np.zeros(3), np.zeros(3))):
        with pytest.raises(ValueError):
            P.set_normal_prior(block, A, b)


def test_facade_refuses_a_problem_of_priors_only(lib, tmp_path):
    """Problem::Evaluate and ceres::Solve on a problem that holds a NormalPrior and no EAResidue block: refused (false /
    FAILURE) before anything touches a device"""
    from edge_alignment_amd import capi
    src = tmp_path / "priors_only.cpp"
    src.write_text(r"""
#include <cstdio>
#include <vector>
#include "ceres/ceres.h"
int main() {
  double q[4] = {1, 0, 0, 0}, t[3] = {0, 0, 0};
  ceres::Problem problem;
  ceres::Matrix A(3, 3);
  A.setIdentity();
  ceres::Vector b(3);
  problem.AddResidualBlock(new ceres::NormalPrior(A, b), NULL, t);
  problem.SetParameterization(q, new ceres::QuaternionParameterization);
  double cost = -1.0;
  std::vector<double> r, g;
  ceres::CRSMatrix J;
  const bool ok = problem.Evaluate(ceres::Problem::EvaluateOptions(), &cost, &r, &g, &J);
  ceres::Solver::Options o;
  ceres::Solver::Summary s;
  ceres::Solve(o, &problem, &s);
  std::printf("%d %d %d %d\n", ok ? 1 : 0, s.termination_type == ceres::FAILURE ? 1 : 0, problem.NumResidualBlocks(), problem.NumResiduals());
  std::printf("%s\n", s.message.c_str());
  return 0;
}
""")
    lib_dir = os.path.dirname(capi.LIB_PATH)
    exe = str(tmp_path / "priors_only")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "edge_alignment_amd", "include"),
                           "-o", exe, str(src), "-L", lib_dir, "-lea_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    first, msg = out.stdout.splitlines()[:2]
    assert first.split() == ["0", "1", "1", "3"]
    assert "priors only" in msg


@pytest.mark.parametrize("eigen_like", [False, True])
def test_facade_example_compiles(eigen_like):
    cmd = ["g++", "-std=c++14", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "edge_alignment_amd", "include"),
           os.path.join(ROOT, "tests", "cpp", "normal_prior_example.cpp")]
    if eigen_like:
        cmd.insert(1, "-DEA_EIGEN_LIKE")
    subprocess.check_call(cmd)
