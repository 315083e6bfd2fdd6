"""ceres::NormalPrior folded into the 32 accumulator slots (edge_alignment_amd/csrc/ea_prior.h) on the CPU: packed JtJ, Jtr
and cost against numpy on random A (k = 1..6), b, q (unit and not) and t; the tangent gradient against central differences
of 1/2 |A (Plus(q, delta) - b)|^2."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def shim():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libea_prior_host.so")
    src = os.path.join(ROOT, "tests", "prior_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_prior.h"), os.path.join(csrc, "ea_types.h"),
            os.path.join(ROOT, "edge_alignment_amd", "include", "ceres", "ceres.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-Wall", "-Werror",
                               "-I", csrc, "-I", os.path.join(ROOT, "edge_alignment_amd", "include"), "-o", so, src])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.ea_prior_host_add.argtypes = [dp, dp, C.c_int, dp, dp, C.c_int, dp, dp]
    L.ea_prior_host_quat_plus.argtypes = [dp, dp, dp]
    return L


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _P(q):
    return np.array([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]])


def _add(shim, Aq, bq, At, bt, q, t):
    Hq = np.ascontiguousarray(Aq.T @ Aq) if Aq is not None else np.zeros((4, 4))
    Ht = np.ascontiguousarray(At.T @ At) if At is not None else np.zeros((3, 3))
    bq = np.ascontiguousarray(bq if bq is not None else np.zeros(4), dtype=np.float64)
    bt = np.ascontiguousarray(bt if bt is not None else np.zeros(3), dtype=np.float64)
    x = np.ascontiguousarray(np.concatenate([q, t]), dtype=np.float64)
    acc = np.zeros(32)
    shim.ea_prior_host_add(_dp(Hq), _dp(bq), int(Aq is not None), _dp(Ht), _dp(bt), int(At is not None), _dp(x), _dp(acc))
    return acc


def _unpack(acc):
    J = np.zeros((6, 6))
    k = 0
    for a in range(6):
        for c in range(a, 6):
            J[a, c] = J[c, a] = acc[k]
            k += 1
    return J, acc[21:27], acc[27]


def _numpy(Aq, bq, At, bt, q, t):
    JtJ, Jtr, cost = np.zeros((6, 6)), np.zeros(6), 0.0
    if Aq is not None:
        J = Aq @ _P(q)
        r = Aq @ (q - bq)
        JtJ[:3, :3] += J.T @ J
        Jtr[:3] += J.T @ r
        cost += 0.5 * r @ r
    if At is not None:
        r = At @ (t - bt)
        JtJ[3:, 3:] += At.T @ At
        Jtr[3:] += At.T @ r
        cost += 0.5 * r @ r
    return JtJ, Jtr, cost


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 6])
def test_terms_match_numpy(shim, k):
    rng = np.random.default_rng(100 + k)
    for trial in range(20):
        q = rng.normal(size=4)
        if trial % 2 == 0:
            q /= np.linalg.norm(q)
        t = rng.normal(size=3)
        Aq, At = rng.normal(size=(k, 4)), rng.normal(size=(k, 3))
        bq, bt = rng.normal(size=4), rng.normal(size=3)
        for use_q, use_t in ((1, 0), (0, 1), (1, 1)):
            args = (Aq if use_q else None, bq if use_q else None, At if use_t else None, bt if use_t else None, q, t)
            acc = _add(shim, *args)
            JtJ, Jtr, cost = _unpack(acc)
            rJ, rg, rc = _numpy(*args)
            assert _rel(JtJ, rJ) <= 1e-13 and _rel(Jtr, rg) <= 1e-13 and abs(cost - rc) <= 1e-13 * rc
            assert acc[28] == 0 and not acc[29:].any()
    assert not _add(shim, None, None, None, None, np.array([1.0, 0, 0, 0]), np.zeros(3)).any()  # no prior, no terms


def test_tangent_gradient_is_the_derivative_of_the_cost(shim):
    rng = np.random.default_rng(7)
    for trial in range(10):
        q = rng.normal(size=4)
        q /= np.linalg.norm(q)
        A, b = rng.normal(size=(3, 4)), q + 0.1 * rng.normal(size=4)
        _, Jtr, _ = _unpack(_add(shim, A, b, None, None, q, np.zeros(3)))

        def f(d):
            out = np.zeros(4)
            shim.ea_prior_host_quat_plus(_dp(np.ascontiguousarray(q)), _dp(np.ascontiguousarray(d, dtype=np.float64)), _dp(out))
            r = A @ (out - b)
            return 0.5 * r @ r

        h = 1e-6
        fd = np.array([(f(h * e) - f(-h * e)) / (2 * h) for e in np.eye(3)])
        assert np.abs(fd - Jtr[:3]).max() <= 1e-7 * max(1.0, np.abs(Jtr[:3]).max())
