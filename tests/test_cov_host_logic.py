"""The SHIPPED covariance code (edge_alignment_amd/csrc/ea_cov.h, the code ea_cov_kernel runs on the device) compiled for
the host with g++ and checked against numpy: inverse, eigen-decomposition, Ceres' rank rules and the ambient lift."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim():
    from edge_alignment_amd import capi
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libea_cov_host.so")
    src = os.path.join(ROOT, "tests", "cov_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_cov.h"), os.path.join(csrc, "ea_types.h"), os.path.join(ROOT, "include", "ea_hip.h"),
            os.path.join(ROOT, "edge_alignment_amd", "include", "ceres", "ceres.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror",
                               "-I", csrc, "-I", os.path.join(ROOT, "edge_alignment_amd", "include"), "-o", so, src])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.ea_cov_host_eigh.argtypes = [dp, dp, dp]
    L.ea_cov_host_compute.argtypes = [dp, C.c_double, dp, C.POINTER(capi.CovarianceOptions), C.POINTER(capi.Covariance)]
    L.ea_cov_host_quat_plus.argtypes = [dp, dp, dp]
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _opts(algorithm=0, rcn=1e-14, nsr=0):
    from edge_alignment_amd import capi
    return capi.CovarianceOptions(algorithm, rcn, nsr, 1)


def _compute(shim, A, q=(1.0, 0, 0, 0), n_invalid=0, **kw):
    from edge_alignment_amd import capi
    A = np.ascontiguousarray(A, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    o = _opts(**kw)
    c = capi.Covariance()
    shim.ea_cov_host_compute(_dp(A), float(n_invalid), _dp(q), C.byref(o), C.byref(c))
    return capi.covariance_to_dict(c)


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _spectrum(rng, lams):
    Q, _ = np.linalg.qr(rng.standard_normal((6, 6)))
    return (Q * np.asarray(lams, dtype=np.float64)) @ Q.T, Q


def test_random_spd_inverse_matches_numpy(shim):
    rng = np.random.default_rng(7)
    for _ in range(200):
        J = rng.standard_normal((40, 6)) * rng.uniform(0.1, 10.0, 6)
        A = J.T @ J
        assert np.linalg.cond(A) < 1e6
        for alg in (0, 1):
            c = _compute(shim, A, algorithm=alg)
            assert c["ok"] and c["why"] == 0 and c["rank"] == 6
            assert _rel(c["tangent"], np.linalg.inv(A)) <= 1e-12
            assert _rel(c["eigenvalues"], np.linalg.eigvalsh(A)[::-1]) <= 1e-13


def test_eigh_vectors_reconstruct(shim):
    rng = np.random.default_rng(3)
    A, _ = _spectrum(rng, [5.0, 3.0, 2.0, 1.0, 0.5, 1e-3])
    lam, V = np.zeros(6), np.zeros((6, 6))
    shim.ea_cov_host_eigh(_dp(np.ascontiguousarray(A)), _dp(lam), _dp(V))
    assert np.all(np.diff(lam) <= 0)
    assert np.abs(V @ np.diag(lam) @ V.T - A).max() <= 1e-14 * np.abs(A).max() * 10
    assert np.abs(V.T @ V - np.eye(6)).max() <= 1e-14


def _pinv_eigh(A, keep):
    w, U = np.linalg.eigh(A)
    w, U = w[::-1], U[:, ::-1]
    return (U[:, :keep] / w[:keep]) @ U[:, :keep].T


@pytest.mark.parametrize("ratio,kept", [(1e-10, True), (1e-18, False)])
def test_rank_rules_on_constructed_spectra(shim, ratio, kept):
    rng = np.random.default_rng(11)
    lams = [4.0, 3.0, 2.0, 1.5, 1.0, 4.0 * ratio]
    A, _ = _spectrum(rng, lams)
    # SPARSE_QR and DENSE_SVD with null_space_rank = 0: full rank or "not computed"
    for alg in (0, 1):
        c = _compute(shim, A, algorithm=alg, nsr=0)
        if kept:
            assert c["ok"] and c["rank"] == 6 and _rel(c["tangent"], _pinv_eigh(A, 6)) <= 1e-6
        else:
            assert not c["ok"] and c["why"] == 1
    # null_space_rank = -1: automatic truncation
    c = _compute(shim, A, algorithm=1, nsr=-1)
    assert c["ok"] and c["rank"] == (6 if kept else 5)
    if not kept:
        assert _rel(c["tangent"], _pinv_eigh(A, 5)) <= 1e-12
    # null_space_rank = 1: the smallest direction dropped unconditionally, the rest tested
    c = _compute(shim, A, algorithm=1, nsr=1)
    assert c["ok"] and c["rank"] == 5 and _rel(c["tangent"], _pinv_eigh(A, 5)) <= 1e-12
    # two tiny directions: null_space_rank = 1 tests the 5th and fails, 2 drops both untested
    B, _ = _spectrum(rng, [4.0, 3.0, 2.0, 1.0, 4.0 * 1e-18, 4.0 * 1e-19])
    c = _compute(shim, B, algorithm=1, nsr=1)
    assert not c["ok"] and c["why"] == 1
    c = _compute(shim, B, algorithm=1, nsr=2)
    assert c["ok"] and c["rank"] == 4 and _rel(c["tangent"], _pinv_eigh(B, 4)) <= 1e-12
    c = _compute(shim, B, algorithm=1, nsr=-1)
    assert c["ok"] and c["rank"] == 4 and _rel(c["tangent"], _pinv_eigh(B, 4)) <= 1e-12


def test_rank_one_system(shim):
    """one edge point: J J^T of a single row"""
    j = np.array([0.3, -1.2, 0.7, 2.0, -0.5, 0.1])
    A = np.outer(j, j)
    for alg, nsr in ((0, 0), (1, 0)):
        c = _compute(shim, A, algorithm=alg, nsr=nsr)
        assert not c["ok"] and c["why"] == 1
    c = _compute(shim, A, algorithm=1, nsr=-1)
    assert c["ok"] and c["rank"] == 1
    assert _rel(c["tangent"], np.linalg.pinv(A)) <= 1e-12


def test_invalid_blocks_mean_not_computed(shim):
    A = np.eye(6)
    c = _compute(shim, A, n_invalid=3)
    assert not c["ok"] and c["why"] == 2 and c["n_invalid"] == 3


def test_ambient_lift_against_differences_of_plus(shim):
    rng = np.random.default_rng(5)
    for _ in range(10):
        q = rng.standard_normal(4)
        q *= rng.uniform(0.5, 1.5) / np.linalg.norm(q)  # not normalised: L is taken at q as given
        L = np.zeros((4, 3))
        h = 1e-6
        for k in range(3):
            dp, dm, op, om = np.zeros(3), np.zeros(3), np.zeros(4), np.zeros(4)
            dp[k], dm[k] = h, -h
            shim.ea_cov_host_quat_plus(_dp(q), _dp(dp), _dp(op))
            shim.ea_cov_host_quat_plus(_dp(q), _dp(dm), _dp(om))
            L[:, k] = (op - om) / (2 * h)
        J = rng.standard_normal((30, 6))
        A = J.T @ J
        c = _compute(shim, A, q=q)
        Cm = np.linalg.inv(A)
        assert c["ok"]
        assert _rel(c["qq"], L @ Cm[:3, :3] @ L.T) <= 1e-8
        assert _rel(c["qt"], L @ Cm[:3, 3:]) <= 1e-8
        assert _rel(c["tt"], Cm[3:, 3:]) <= 1e-12
