"""The SHIPPED trust-region state machine (edge_alignment_amd/csrc/ea_lm.h, compiled for the host by the lm_host_shim
fixture) driven by the oracle's evaluation plus a numpy NormalPrior -- the reference trajectory of a prior solve: a strong
prior pins the solution to b, a vanishing one reproduces the prior-free iterates, and a solve run to the gradient test ends
where the total gradient (edge points + prior) passes Ceres' gradient rule.  `_run_prior` is also the reference of
tests/test_gpu_prior_shim.py."""
import ctypes as C

import numpy as np
import pytest

from edge_alignment_amd import synth


class LMOptions(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int),
                ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double), ("parameter_tolerance", C.c_double),
                ("initial_trust_region_radius", C.c_double), ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
                ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double), ("max_lm_diagonal", C.c_double),
                ("max_num_consecutive_invalid_steps", C.c_int), ("jacobi_scaling", C.c_int), ("strategy", C.c_int)]


KT = 128


class ShimOut(C.Structure):
    _fields_ = [("x", C.c_double * 7), ("iteration", C.c_int), ("termination", C.c_int), ("why", C.c_int),
                ("num_successful", C.c_int), ("num_unsuccessful", C.c_int), ("num_evals", C.c_int),
                ("final_cost", C.c_double), ("it_cost", C.c_double * KT), ("it_radius", C.c_double * KT),
                ("it_successful", C.c_int * KT)]


CB = C.CFUNCTYPE(None, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)
WHY = ["none", "function_tolerance", "gradient_tolerance", "parameter_tolerance", "max_iterations", "min_radius",
       "initial_eval_failed", "too_many_invalid_steps", "eval_failed"]


def _opts(**kw):
    o = LMOptions(50, 1e-6, 1e-10, 1e-8, 1e4, 1e16, 1e-32, 1e-3, 1e-6, 1e32, 5, 1, 0)
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def _P(q):
    return np.array([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]])


def prior_terms(q, t, prior):
    """the NormalPriors' JtJ (6x6), Jtr (6), cost at (q, t); prior = dict(Aq, bq, At, bt), any pair may be missing"""
    JtJ, Jtr, cost = np.zeros((6, 6)), np.zeros(6), 0.0
    if prior.get("Aq") is not None:
        J, r = prior["Aq"] @ _P(q), prior["Aq"] @ (np.asarray(q) - prior["bq"])
        JtJ[:3, :3] += J.T @ J; Jtr[:3] += J.T @ r; cost += 0.5 * r @ r
    if prior.get("At") is not None:
        J, r = prior["At"], prior["At"] @ (np.asarray(t) - prior["bt"])
        JtJ[3:, 3:] += J.T @ J; Jtr[3:] += J.T @ r; cost += 0.5 * r @ r
    return JtJ, Jtr, cost


def total_eval(P, X, q, t, prior):
    e = P.eval(X, q, t)
    J, g, c = prior_terms(q, t, prior)
    return e["JtJ"] + J, e["Jtr"] + g, e["cost"] + c, e["n_invalid"]


def _run_prior(shim, P, X, q0, t0, prior, **kw):
    def cb(pose, acc, _):
        x = np.array([pose[i] for i in range(7)])
        JtJ, Jtr, cost, bad = total_eval(P, X, x[:4], x[4:], prior)
        k = 0
        for a in range(6):
            for b in range(a, 6):
                acc[k] = JtJ[a, b]; k += 1
        for a in range(6):
            acc[21 + a] = Jtr[a]
        acc[27] = cost
        acc[28] = float(bad)
        for i in range(29, 32):
            acc[i] = 0.0
    out = ShimOut()
    o = _opts(**kw)
    q0 = np.asarray(q0, dtype=np.float64); t0 = np.asarray(t0, dtype=np.float64)
    shim.ea_lm_host_solve.argtypes = [C.POINTER(LMOptions), C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_int, CB, C.c_void_p, C.POINTER(ShimOut)]
    rc = shim.ea_lm_host_solve(C.byref(o), q0.ctypes.data_as(C.POINTER(C.c_double)), t0.ctypes.data_as(C.POINTER(C.c_double)), 0, CB(cb), None, C.byref(out))
    assert rc == 0
    return out


def _quat_plus(x, d):
    n = np.linalg.norm(d)
    if n == 0:
        return np.array(x, dtype=np.float64)
    a = np.concatenate([[np.cos(n)], np.sin(n) / n * np.asarray(d)])
    w1, v1, w2, v2 = a[0], a[1:], x[0], np.asarray(x[1:])
    return np.concatenate([[w1 * w2 - v1 @ v2], w1 * v2 + w2 * v1 + np.cross(v1, v2)])


def _problem():
    pr = synth.make_problem(120, 160, 1500, 40, 21, 130.0, 130.0, 79.5, 59.5,
                            planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)), planted_t=(0.01, -0.005, 0.02),
                            normalize=True)
    return pr


@pytest.mark.parametrize("strategy", [0, 1])
def test_strong_prior_pins_the_solution(lm_host_shim, oracle, strategy):
    pr = _problem()
    P = oracle.OracleProblem(pr["grid"], *pr["K"])
    bq = synth.quat_from_axis_angle([0, 1, 1], np.deg2rad(0.5)); bt = np.array([0.02, 0.01, -0.01])
    prior = dict(Aq=1e6 * np.eye(4), bq=bq, At=1e6 * np.eye(3), bt=bt)
    out = _run_prior(lm_host_shim, P, pr["xyz"], [1, 0, 0, 0], [0, 0, 0], prior, strategy=strategy)
    x = np.array(out.x[:])
    assert out.termination == 0
    assert np.abs(x[:4] - bq).max() < 1e-6 and np.abs(x[4:] - bt).max() < 1e-6


@pytest.mark.parametrize("strategy", [0, 1])
def test_vanishing_prior_reproduces_the_prior_free_iterates(lm_host_shim, oracle, strategy):
    pr = _problem()
    P = oracle.OracleProblem(pr["grid"], *pr["K"])
    prior = dict(Aq=1e-12 * np.eye(4), bq=np.array([0.9, 0.1, 0.2, 0.3]), At=1e-12 * np.eye(3), bt=np.array([0.5, -0.5, 0.5]))
    a = _run_prior(lm_host_shim, P, pr["xyz"], [1, 0, 0, 0], [0, 0, 0], prior, strategy=strategy)
    b = _run_prior(lm_host_shim, P, pr["xyz"], [1, 0, 0, 0], [0, 0, 0], {}, strategy=strategy)
    assert a.iteration == b.iteration and a.why == b.why and a.num_successful == b.num_successful
    n = a.iteration + 1
    assert list(a.it_successful[:n]) == list(b.it_successful[:n])
    assert np.array(a.it_cost[:n]) == pytest.approx(np.array(b.it_cost[:n]), rel=1e-12)
    assert np.abs(np.array(a.x[:]) - np.array(b.x[:])).max() < 1e-12


def test_gradient_rule_holds_at_the_final_pose(lm_host_shim, oracle):
    """function and parameter tests off: the solve ends on the gradient test, and the TOTAL gradient at its pose -- edge
    points plus prior, evaluated independently here -- passes Ceres' rule |x - Plus(x, -g)|_inf <= gradient_tolerance"""
    pr = _problem()
    P = oracle.OracleProblem(pr["grid"], *pr["K"], loss=oracle.LOSS_TRIVIAL)
    rng = np.random.default_rng(5)
    prior = dict(Aq=rng.normal(size=(3, 4)) * 5.0, bq=np.array([0.999, 0.02, -0.01, 0.03]), At=rng.normal(size=(3, 3)) * 5.0,
                 bt=np.array([0.01, 0.0, 0.02]))
    tol = 1e-7
    out = _run_prior(lm_host_shim, P, pr["xyz"], [1, 0, 0, 0], [0, 0, 0], prior, gradient_tolerance=tol, function_tolerance=0.0,
                     parameter_tolerance=0.0, max_num_iterations=100)
    assert WHY[out.why] == "gradient_tolerance"
    x = np.array(out.x[:])
    _, g, _, bad = total_eval(P, pr["xyz"], x[:4], x[4:], prior)
    assert bad == 0
    step = np.concatenate([x[:4] - _quat_plus(x[:4], -g[:3]), g[3:]])
    assert np.abs(step).max() <= tol
    # the prior matters at this pose: the edge points' gradient alone fails the rule
    e = P.eval(pr["xyz"], x[:4], x[4:])
    assert np.abs(np.concatenate([x[:4] - _quat_plus(x[:4], -e["Jtr"][:3]), e["Jtr"][3:]])).max() > tol
