"""The covariance ladder (tests/cov_ladder.py) on the CPU: the oracle's JtJ of every rung through two host builds of the
SHIPPED edge_alignment_amd/csrc/ea_cov.h -- g++ -ffp-contract=off, and -ffp-contract=fast -mfma, the contraction the device
build applies -- against the 60-digit reference.  It proves the inputs and the bounds satisfiable before a device sees them:
tests/test_gpu_covariance_ladder.py runs the same assertions through ea_problem_covariance and ea_batch_covariance.

The constant 32 of the bounds was set from 240 ladder matrices x 6 ranks through both builds: worst rank-k error 6.5 of the
32 (numpy.linalg.eigh: 8.0), full-rank inverse below 0.07 of kappa * 2^-53.  This module's nine draws, masks and the
non-unit pose included (printed at its end): rank-k 2.8 of 32, inverse 0.20 of kappa * 2^-53,
eigenvalues 17.4 of 32 with contraction, 14.5 without.

Mutations of a scratch copy of ea_cov.h (host builds only) and the tests of this module they turn red, of 47 with both
builds: kCovSweeps = 2: 20; the skip criterion 1e-17 -> 1e-8: 18; j <= rank in cov_pinv: 16; a sort that leaves the columns
of V where they were: 26."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import cov_ladder as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILDS = {"nofma": ["-ffp-contract=off"], "fma": ["-ffp-contract=fast", "-mfma"]}


def _host_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(ln.startswith("flags") and " fma " in ln + " " for ln in f)
    except OSError:
        return False


@pytest.fixture(scope="module", params=sorted(BUILDS))
def shim(request):
    from edge_alignment_amd import capi
    if request.param == "fma" and not _host_has_fma():
        pytest.skip("this host has no FMA instructions")
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, "libea_cov_host_%s.so" % request.param)
    src = os.path.join(ROOT, "tests", "cov_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_cov.h"), os.path.join(csrc, "ea_types.h"), os.path.join(ROOT, "include", "ea_hip.h"),
            os.path.join(ROOT, "edge_alignment_amd", "include", "ceres", "ceres.h")]
    if not os.path.exists(so) or any(os.path.getmtime(d) > os.path.getmtime(so) for d in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror"] + BUILDS[request.param] +
                              ["-I", csrc, "-I", os.path.join(ROOT, "edge_alignment_amd", "include"), "-o", so, src])
    L = C.CDLL(so)
    dp = C.POINTER(C.c_double)
    L.ea_cov_host_compute_held.argtypes = [dp, C.c_double, dp, C.POINTER(capi.CovarianceOptions), C.c_int, C.POINTER(capi.Covariance)]
    return L


@pytest.fixture(scope="module")
def worst(shim):
    w = cl.Worst()
    yield w
    print("\n" + w.line("host build of ea_cov.h"))


@pytest.fixture(scope="module")
def systems(oracle):
    """the oracle's evaluation of every rung at the ladder's pose, trivial loss"""
    O = oracle.OracleProblem(cl.grid(), *cl.K, loss=oracle.LOSS_TRIVIAL)
    return [O.eval(cl.rung_points(i), cl.Q, cl.T) for i in range(len(cl.RUNGS))]


def _computer(shim, A, q):
    from edge_alignment_amd import capi
    A = np.ascontiguousarray(A, dtype=np.float64)
    q = np.ascontiguousarray(q, dtype=np.float64)
    dp = C.POINTER(C.c_double)

    def compute(algorithm=cl.SPARSE_QR, min_rcn=1e-14, nsr=0, held=None):
        o = capi.CovarianceOptions(algorithm, min_rcn, nsr, 1)
        c = capi.Covariance()
        bits = sum(1 << i for i in range(6) if held is not None and held[i])
        shim.ea_cov_host_compute_held(A.ctypes.data_as(dp), 0.0, q.ctypes.data_as(dp), C.byref(o), bits, C.byref(c))
        return capi.covariance_to_dict(c)
    return compute


RUNG_IDS = ["s=%g" % s for s in cl.RUNGS]


def test_ladder_spans_the_conditioning(systems):
    kappas = [cl.ref_of(e["JtJ"]).kappa for e in systems]
    print("\nkappa_2 per rung: " + ", ".join("%g: %.2g" % (s, k) for s, k in zip(cl.RUNGS, kappas)))
    assert all(e["n_invalid"] == 0 for e in systems)
    assert kappas[0] <= 1e3 and kappas[-1] >= 1e15
    assert all(a < b for a, b in zip(kappas, kappas[1:])), kappas
    assert sum(k <= 1e8 for k in kappas) >= 4 and sum(k > 1e8 for k in kappas) >= 4


def test_defaults_and_1e12_on_every_rung(shim, systems, worst):
    decisions = [cl.check_defaults(_computer(shim, e["JtJ"], cl.Q), e["JtJ"], cl.Q, worst) for e in systems]
    cl.check_caps(decisions)
    # both ends of the ladder are decided, and differently
    assert decisions[0][1e-14] == 6 and decisions[-1][1e-14] == -1 and decisions[-1][1e-12] == -1


@pytest.mark.parametrize("i", range(len(cl.RUNGS)), ids=RUNG_IDS)
def test_truncation_at_every_rank(shim, systems, worst, i):
    A = systems[i]["JtJ"]
    if cl.ref_of(A).kappa > 1e8:
        return  # (the rungs above serve the decisions at the defaults only)
    cl.check_truncation(_computer(shim, A, cl.Q), A, cl.Q, worst)


@pytest.mark.parametrize("i", range(len(cl.RUNGS)), ids=RUNG_IDS)
def test_threshold_a_thousandth_either_side(shim, systems, worst, i):
    A = systems[i]["JtJ"]
    if cl.ref_of(A).kappa > 1e8:
        return
    cl.check_threshold(_computer(shim, A, cl.Q), A, cl.Q, worst)


@pytest.mark.parametrize("i", cl.MASK_RUNGS, ids=[RUNG_IDS[i] for i in cl.MASK_RUNGS])
def test_held_masks_against_the_reduced_reference(shim, systems, worst, i):
    A = systems[i]["JtJ"]
    cl.check_masks(_computer(shim, A, cl.Q), A, cl.Q, worst)


def test_non_unit_quaternion(shim, oracle, worst):
    q = 1.2 * cl.Q
    O = oracle.OracleProblem(cl.grid(), *cl.K, loss=oracle.LOSS_TRIVIAL)
    for i in (0, 3):
        A = O.eval(cl.rung_points(i), q, cl.T)["JtJ"]
        compute = _computer(shim, A, q)
        assert cl.check_result(compute(), A, q, worst, want=6) == 6
        assert cl.check_result(compute(algorithm=cl.DENSE_SVD, min_rcn=0.0, nsr=2), A, q, worst, cl.DENSE_SVD, 0.0, 2, want=4) == 4
