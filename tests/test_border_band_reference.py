"""The two CPU checkers (oracle/ea_oracle.c with Jet rows, oracle/ea_numpy.py) against the extended-precision restatement
of tests/border_band.py on every case of the border-band generator: all shapes, noise and distance-like texels, the
identity, a small unit pose and a non-unit quaternion, the three losses.  This pins the checkers where a 4x4 stencil
touches the border (per-tap clamping) and prints, per case, what plain fp64 and plain fp32 arithmetic lose against the
reference: the figures the GPU tolerances of test_gpu_border_band.py refer to.

Bounds: the checkers are plain fp64 arithmetic, so they are held to the rule the kernels are held to
(border_band.tolerances): the larger of the project's fp64 bound (r 1e-12 absolute, J 1e-12 of the largest entry, sums
1e-11) and 4x the deviation of the plain fp64 run of the reference's own formulas."""
import numpy as np
import pytest

import border_band as bb
from oracle import ea_numpy as en

N = 4000


def _cases():
    for i, (H, W) in enumerate(bb.SHAPES):
        for kind in bb.KINDS:
            yield pytest.param(H, W, kind, 100 + i, id="%dx%d-%s" % (H, W, kind))


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 1e-18


def test_reference_reproduces_hand_computed_clamped_taps():
    """a 2 x 3 image, one point per region: far outside (constant border texel), on a texel centre, and half-way
    between two columns on the first row, where Catmull-Rom through the clamped taps has a closed form"""
    img = np.array([[1.0, 2.0, 4.0], [8.0, 16.0, 32.0]])
    K = (1.0, 1.0, 0.0, 0.0)
    pts = np.array([[-9.0, -9.0, 1.0], [50.0, 50.0, 1.0], [1.0, 1.0, 1.0], [0.5, 0.0, 1.0], [60.0, -7.0, 1.0]])
    out = bb.functor(img, K, pts, bb.Q_ID, bb.T_ID)
    # u = 0.5, v = 0: rows clamp to (0, 0, 1, 1) -> weights at fraction 0 pick row 0; columns (-1, 0, 1, 2) -> (1, 1, 2, 4)
    mid = (-1.0 + 9.0 * 1.0 + 9.0 * 2.0 - 4.0) / 16.0
    assert np.allclose(out["r"].astype(np.float64), [1.0, 32.0, 16.0, mid, 4.0], rtol=0, atol=1e-18)
    assert np.abs(out["J"][[0, 1, 4]].astype(np.float64)).max() == 0.0   # constant border: zero gradient
    assert out["band"].all()


@pytest.mark.parametrize("H,W,kind,seed", _cases())
def test_cpu_checkers_match_the_extended_reference_on_the_band(oracle, H, W, kind, seed):
    pr = bb.band_problem(H, W, N, seed, kind)
    xyz32 = pr["xyz"].astype(np.float32).astype(np.float64)   # what an fp32 problem holds
    lines = []
    for pi, (q, t) in enumerate(bb.POSES):
        raw = bb.functor(pr["image"], pr["K"], pr["xyz"], q, t)
        assert raw["valid"].all() and not np.isnan(raw["J"].astype(np.float64)).any()
        share = float(raw["band"].mean())
        assert share >= 0.5, share                            # the workload is a border workload
        # d(u, v) / d pose stays of order fx: every row is compared, none is rounding noise of a zero gradient
        for loss in bb.LOSSES:
            ref = bb.with_loss(raw, *loss)
            tol = bb.tolerances(pr, pr["xyz"], q, t, loss, np.float64, ref_rows=ref)
            es = bb.sums(ref)
            O = oracle.OracleProblem(pr["grid"], *pr["K"], loss=loss[0], loss_a=loss[1])
            e = O.eval(pr["xyz"], q, t, oracle.JAC_JET, materialize=True)
            assert e["n_invalid"] == 0
            where = (pi, loss)
            assert bb.dev_r(e["raw_r"], raw["r"]) <= tol["r"] and bb.dev_J(e["raw_J"], raw["J"]) <= tol["J"], where
            assert bb.dev_r(e["r"], ref["r"]) <= tol["r"] and bb.dev_J(e["J"], ref["J"]) <= tol["J"], where
            assert bb.dev_sums(e, es) <= tol["sums"], where
            a = O.eval(pr["xyz"], q, t, oracle.JAC_ANALYTIC, materialize=True)
            assert bb.dev_r(a["r"], ref["r"]) <= tol["r"] and bb.dev_J(a["J"], ref["J"]) <= tol["J"], where
            if pi < 2:   # ea_numpy's Jacobian is the unit-quaternion identity
                g = en.evaluate(pr["grid"], pr["K"], pr["xyz"], q, t, loss_kind=loss[0], loss_a=loss[1])
                assert g["n_invalid"] == 0
                assert bb.dev_r(g["raw_r"], raw["r"]) <= tol["r"] and bb.dev_J(g["raw_J"], raw["J"]) <= tol["J"], where
                assert bb.dev_r(g["r"], ref["r"]) <= tol["r"] and bb.dev_J(g["J"], ref["J"]) <= tol["J"], where
                assert bb.dev_sums(g, es) <= tol["sums"], where
            if loss[0] == bb.LOSS_TRIVIAL:
                t32 = bb.tolerances(pr, xyz32, q, t, loss, np.float32)
                lines.append("BAND-CPU %dx%d %s pose %d share %.2f  plain fp64 r %.1e J %.1e sums %.1e | plain fp32 r %.1e J %.1e sums %.1e"
                             % (H, W, kind, pi, share, tol["plain_r"], tol["plain_J"], tol["plain_sums"],
                                t32["plain_r"], t32["plain_J"], t32["plain_sums"]))
    print("\n".join(lines))   # (shown with -s or -rP)


@pytest.mark.parametrize("H,W", bb.CORE_SHAPES, ids=["%dx%d" % s for s in bb.CORE_SHAPES])
def test_weighted_rows_and_sums_on_the_band(oracle, H, W):
    """per-point weights (ceres::ScaledLoss per block) through border_band: (a) integer weights in {0..3} are the cloud with
    point i repeated w_i times, in the reference's own extended arithmetic -- the two sums differ by the order of at most
    3 N additions, 3 N eps(longdouble) = 1.3e-15 for N = 4000, asserted 2e-15; (b) the oracle's raw rows scaled by
    sqrt(w rho') and the sums of tests/weights_ref.py, with real weights that have exact zeros, under the rule the kernels
    are held to: weighted plain-fp64 rows against weighted extended rows, 4x, or the project's bound"""
    import weights_ref as wr
    pr = bb.band_problem(H, W, N, 100 + bb.SHAPES.index((H, W)), "noise")
    wi = np.random.default_rng(H + W).integers(0, 4, N)
    wreal = wr.real_weights(N, H + W)
    assert (wreal == 0).sum() >= N // 6 and (wi == 0).any()
    for pi, (q, t) in enumerate(bb.POSES):
        raw = bb.functor(pr["image"], pr["K"], pr["xyz"], q, t)
        rep = bb.functor(pr["image"], pr["K"], np.repeat(pr["xyz"], wi, axis=0), q, t)
        assert raw["valid"].all() and raw["band"].mean() >= 0.5
        for loss in bb.LOSSES:
            a, b = bb.sums(bb.with_loss(raw, *loss, weights=wi)), bb.sums(bb.with_loss(rep, *loss))
            d = bb.dev_sums(a, b)
            assert d <= 2e-15, (pi, loss, "repeated cloud", d)
            ref = bb.with_loss(raw, *loss, weights=wreal)
            tol = bb.tolerances(pr, pr["xyz"], q, t, loss, np.float64, ref_rows=ref, weights=wreal)
            e = oracle.OracleProblem(pr["grid"], *pr["K"], loss=loss[0], loss_a=loss[1]).eval(pr["xyz"], q, t, oracle.JAC_JET, materialize=True)
            sc = np.sqrt(wreal * wr.loss_pair(loss[0], loss[1], e["raw_r"] ** 2)[1])
            assert bb.dev_r(sc * e["raw_r"], ref["r"]) <= tol["r"] and bb.dev_J(sc[:, None] * e["raw_J"], ref["J"]) <= tol["J"], (pi, loss)
            cost, JtJ, Jtr = wr.weighted_sums(e, wreal, *loss)
            ds = bb.dev_sums(dict(cost=cost, JtJ=JtJ, Jtr=Jtr), bb.sums(ref))
            assert ds <= tol["sums"], (pi, loss, ds, tol["sums"])
            if loss[0] == bb.LOSS_CAUCHY:
                print("BAND-CPU weighted %dx%d pose %d: repeated cloud %.1e | plain fp64 r %.1e J %.1e sums %.1e | oracle sums %.1e"
                      % (H, W, pi, d, tol["plain_r"], tol["plain_J"], tol["plain_sums"], ds))
