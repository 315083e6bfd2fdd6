"""tests/weights_ref.py against the oracle itself (no GPU): for integer weights the weighted problem IS the problem with
point i repeated w_i times, so the numpy sums over the oracle's raw rows must equal OracleProblem.eval of
np.repeat(xyz, w) -- with and without failed blocks (|b_z| < 0.01), which the sums leave out and the oracle counts once per
copy.  Measured on the cases below: <= 6.9e-15 relative on cost, JtJ and Jtr; asserted 1e-13 (a factor of 15 for another
summation order, nothing for a wrong term)."""
import numpy as np
import pytest

import test_gpu_weights as tgw
import weights_ref as wr
from test_gpu_weights import cloud  # noqa: F401  (the fixture)

TOL = 1e-13


def _weights(n, idx):
    w = np.random.default_rng(200 + n).integers(0, 4, n)
    for i, v in zip(idx, wr.FAILED_W):
        w[i] = v
    return w


@pytest.mark.parametrize("f32", [False, True], ids=["as-given", "fp32-rounded"])
@pytest.mark.parametrize("failed", [False, True], ids=["all-valid", "failed-blocks"])
@pytest.mark.parametrize("n", [1, 511, 513, 1025])
def test_sums_equal_the_oracle_on_the_repeated_cloud(oracle, cloud, n, failed, f32):
    xyz, idx = cloud["xyz"][:n], []
    if failed:
        xyz, idx = wr.plant_failed(xyz, tgw.QE, tgw.TE)
    if f32:
        xyz = xyz.astype(np.float32).astype(np.float64)
    w = _weights(n, idx)
    for kind, a in tgw.LOSSES:
        O = oracle.OracleProblem(cloud["grid"], *cloud["K"], loss=kind, loss_a=a)
        e = O.eval(xyz, tgw.QE, tgw.TE, oracle.JAC_JET, materialize=True)
        assert np.flatnonzero(np.isnan(e["raw_r"])).tolist() == idx and wr.n_failed(e) == len(idx)
        rep = O.eval(np.repeat(xyz, w, axis=0), tgw.QE, tgw.TE, oracle.JAC_JET)
        assert rep["n_invalid"] == int(w[idx].sum())          # the oracle counts every copy of a failed block
        cost, JtJ, Jtr = wr.weighted_sums(e, w, kind, a)
        d = (abs(cost - rep["cost"]) / max(abs(rep["cost"]), 1e-300), wr.rel(JtJ, rep["JtJ"]), wr.rel(Jtr, rep["Jtr"]))
        print("WEIGHTS-REF n %d loss %d failed %d f32 %d: cost %.1e JtJ %.1e Jtr %.1e" % ((n, kind, failed, f32) + d))
        assert max(d) <= TOL, (n, kind, d)
        # the weightless reading: weights all 1 are the oracle's own sums of the cloud
        cost, JtJ, Jtr = wr.weighted_sums(e, np.ones(n), kind, a)
        d = (abs(cost - e["cost"]) / max(abs(e["cost"]), 1e-300), wr.rel(JtJ, e["JtJ"]), wr.rel(Jtr, e["Jtr"]))
        assert max(d) <= TOL, (n, kind, "unit weights", d)


def test_planted_blocks_sit_where_the_kernels_can_go_wrong():
    for n in (257, 513, 1025):
        idx = wr.failed_indices(n)
        assert len(idx) == 3 and idx[0] == 0 and idx[-1] == n - 1
        assert any(i % 512 >= 256 for i in idx)          # the k = 1 half of a two-point lane
    assert wr.failed_indices(1) == [0]
    assert all(0.003 <= abs(b) <= 0.008 for b in wr.FAILED_BZ) and 0 in wr.FAILED_W
