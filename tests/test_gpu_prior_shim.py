"""The device solve with NormalPriors on q and t follows an independent reference: the shipped state machine on the host
driven by the oracle's evaluation plus the numpy prior (tests/test_prior_lm_host.py::_run_prior) -- on the bundled pair at
strides 30 and 1, LM and dogleg, at the bars of test_bundled_pair_solve_fp64_follows_oracle: the same iterations, reason
and accepted steps, per-iteration cost to 1e-7, the pose to 1e-7."""
import numpy as np
import pytest

from test_prior_lm_host import _run_prior, WHY

pytestmark = pytest.mark.gpu
RNG = np.random.default_rng(77)
PRIOR = dict(Aq=RNG.normal(size=(3, 4)) * 30.0, bq=np.array([0.999, 0.01, -0.02, 0.015]),
             At=RNG.normal(size=(2, 3)) * 20.0, bt=np.array([0.01, -0.02, 0.03]))


@pytest.mark.parametrize("stride", [30, 1])
@pytest.mark.parametrize("strategy", [0, 1])
def test_prior_solve_follows_host_shim(hip, oracle, lm_host_shim, bundled_pair, stride, strategy):
    X = bundled_pair["aX"][:3, ::stride].T.copy()
    O = oracle.OracleProblem(bundled_pair["grids"][3], *bundled_pair["K"])
    ref = _run_prior(lm_host_shim, O, X, [1, 0, 0, 0], [0, 0, 0], PRIOR, strategy=strategy)
    P = hip.Problem(*bundled_pair["K"], dtype=hip.EA_F64)
    P.set_points(X)
    P.set_dt_grid(bundled_pair["grids"][3])
    P.set_normal_prior(0, PRIOR["Aq"], PRIOR["bq"])
    P.set_normal_prior(1, PRIOR["At"], PRIOR["bt"])
    q, t, s = P.solve([1, 0, 0, 0], [0, 0, 0], strategy=hip.STRATEGY_DOGLEG if strategy else hip.STRATEGY_LM)
    assert s["num_iterations"] == ref.iteration and s["why"] == WHY[ref.why] and s["termination"] == ref.termination
    n = ref.iteration + 1
    assert list(s["it_successful"]) == list(ref.it_successful[:n])
    assert s["it_cost"] == pytest.approx(np.array(ref.it_cost[:n]), rel=1e-7)
    x = np.array(ref.x[:])
    assert np.abs(q - x[:4]).max() < 1e-7 and np.abs(t - x[4:]).max() < 1e-7
    # and the prior is what moved it: the prior-free solve ends elsewhere
    P.clear_normal_prior(0); P.clear_normal_prior(1)
    q0, t0, _ = P.solve([1, 0, 0, 0], [0, 0, 0], strategy=hip.STRATEGY_DOGLEG if strategy else hip.STRATEGY_LM)
    assert max(np.abs(q0 - q).max(), np.abs(t0 - t).max()) > 1e-5
    P.close()
