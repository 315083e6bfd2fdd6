"""Per-point weights (ceres::ScaledLoss per residual block) on the GPU: ea_problem_set_weights / _get_weights /
_set_depth_weighting through every evaluation and solve path, against the expected values of tests/weights_ref.py
(numpy sums over the oracle's raw rows; the oracle's solve of the cloud with point i repeated w_i times)."""
import os
import struct
import subprocess

import numpy as np
import pytest

from edge_alignment_amd import synth
import weights_ref as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "rgbd")
DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)
LOSSES = ((wr.LOSS_TRIVIAL, 1.0), (wr.LOSS_CAUCHY, 1.0), (wr.LOSS_HUBER, 0.05))
# a pose near, not at, the planted one
QE = synth.quat_mul(synth.quat_from_axis_angle([0.2, -1, 0.4], 0.003), wr.PLANTED_Q)
TE = np.array(wr.PLANTED_T) + 0.001


@pytest.fixture(scope="module")
def cloud():
    """96 x 128, 1025 points: the chunk tests take its first n points"""
    return synth.make_problem(96, 128, 1025, 24, 21, 130.0, 130.0, 63.5, 47.5, planted_q=wr.PLANTED_Q, planted_t=wr.PLANTED_T)


@pytest.fixture(scope="module")
def solves(oracle):
    """the three solve problems and the oracle's solve of each repeated cloud, computed once"""
    out = []
    for spec in wr.SOLVE_PROBLEMS:
        pb = wr.solve_problem(*spec)
        O = oracle.OracleProblem(pb["grid"], *pb["K"])
        pb["oracle"] = O.solve(pb["repeated"], wr.Q0, wr.T0)
        out.append(pb)
    return out


def _problem(hip, xyz, grid, K, dtype, loss=(wr.LOSS_CAUCHY, 1.0), w=None, order=None):
    P = hip.Problem(*K, dtype=dtype)
    if order is not None:
        P.set_point_order(order)
    P.set_points(xyz)
    P.set_dt_grid(grid)
    P.set_loss(*loss)
    if w is not None:
        P.set_weights(w)
    return P


def _check_sums(g, cost, JtJ, Jtr, tol, what):
    print(what, "cost", abs(g["cost"] - cost) / max(abs(cost), 1e-300), "JtJ", wr.rel(g["JtJ"], JtJ), "Jtr", wr.rel(g["Jtr"], Jtr))
    assert abs(g["cost"] - cost) <= tol * abs(cost), what
    assert wr.rel(g["JtJ"], JtJ) <= tol and wr.rel(g["Jtr"], Jtr) <= tol, what


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025])
def test_chunk_and_wavefront_edges(hip, oracle, cloud, n):
    xyz, w = cloud["xyz"][:n], wr.real_weights(n, 100 + n)
    for kind, a in LOSSES:
        e = oracle.OracleProblem(cloud["grid"], *cloud["K"], loss=kind, loss_a=a).eval(xyz, QE, TE, oracle.JAC_JET, materialize=True)
        cost, JtJ, Jtr = wr.weighted_sums(e, w, kind, a)
        for dtype, tol in ((hip.EA_F64, 1e-11), (hip.EA_F32, 2e-4)):
            P = _problem(hip, xyz, cloud["grid"], cloud["K"], dtype, (kind, a), w)
            g = P.eval(QE, TE)
            assert g["n_invalid"] == 0
            _check_sums(g, cost, JtJ, Jtr, tol, (n, kind, dtype))
            c, bad = P.cost(QE, TE)
            assert bad == 0 and abs(c - cost) <= tol * abs(cost)
            P.close()


def test_weights_with_distortion(hip, oracle, cloud):
    """bits 0 and 2 of the variant together"""
    n = 513
    xyz, w = cloud["xyz"][:n], wr.real_weights(n, 7)
    e = oracle.OracleProblem(cloud["grid"], *cloud["K"], distortion=DIST).eval(xyz, QE, TE, oracle.JAC_JET, materialize=True)
    cost, JtJ, Jtr = wr.weighted_sums(e, w)
    for dtype, tol in ((hip.EA_F64, 1e-11), (hip.EA_F32, 2e-4)):
        P = _problem(hip, xyz, cloud["grid"], cloud["K"], dtype, w=w)
        P.set_distortion(*DIST)
        _check_sums(P.eval(QE, TE), cost, JtJ, Jtr, tol, ("distortion", dtype))
        c, _ = P.cost(QE, TE)
        assert abs(c - cost) <= tol * abs(cost)
        P.close()


def test_two_terms_with_their_own_weights(hip, oracle, cloud):
    xa, xb = cloud["xyz"][:257], cloud["xyz"][300:900]
    wa, wb = wr.real_weights(257, 8), wr.real_weights(600, 9)
    O = oracle.OracleProblem(cloud["grid"], *cloud["K"])
    sa = wr.weighted_sums(O.eval(xa, QE, TE, oracle.JAC_JET, materialize=True), wa)
    sb = wr.weighted_sums(O.eval(xb, QE, TE, oracle.JAC_JET, materialize=True), wb)
    su = wr.weighted_sums(O.eval(xb, QE, TE, oracle.JAC_JET, materialize=True), np.ones(600))
    for dtype, tol in ((hip.EA_F64, 1e-11), (hip.EA_F32, 2e-4)):
        P = _problem(hip, xa, cloud["grid"], cloud["K"], dtype, w=wa)
        T = _problem(hip, xb, cloud["grid"], cloud["K"], dtype, w=wb)
        P.add_term(T)
        _check_sums(P.eval(QE, TE), *[x + y for x, y in zip(sa, sb)], tol, ("terms", dtype))
        T.set_weights(None)  # the term without weights: bit 2 set on the head only, nothing loaded for the term
        _check_sums(P.eval(QE, TE), *[x + y for x, y in zip(sa, su)], tol, ("head only", dtype))
        P.clear_terms()
        P.close(); T.close()


def test_tile_order_keeps_caller_order_outside(hip, oracle, cloud):
    n = 1025
    xyz, w = cloud["xyz"], wr.real_weights(n, 10)
    e = oracle.OracleProblem(cloud["grid"], *cloud["K"]).eval(xyz, QE, TE, oracle.JAC_JET, materialize=True)
    cost, JtJ, Jtr = wr.weighted_sums(e, w)
    _, rho1 = wr.loss_pair(wr.LOSS_CAUCHY, 1.0, e["raw_r"] ** 2)
    for dtype, tol, ptol in ((hip.EA_F64, 1e-11, 1e-12), (hip.EA_F32, 2e-4, 2e-5)):
        P = _problem(hip, xyz, cloud["grid"], cloud["K"], dtype, w=w, order=16)
        assert P.point_order == 16
        C = _problem(hip, xyz, cloud["grid"], cloud["K"], dtype, w=w, order=0)
        g, gc = P.eval(QE, TE), C.eval(QE, TE)
        _check_sums(g, cost, JtJ, Jtr, tol, ("tiled", dtype))
        _check_sums(g, gc["cost"], gc["JtJ"], gc["Jtr"], tol, ("tiled against caller order", dtype))
        stored = w if dtype == hip.EA_F64 else w.astype(np.float32).astype(np.float64)
        assert np.array_equal(P.get_weights(), stored) and np.array_equal(C.get_weights(), stored)
        r, J = P.eval_points(QE, TE, corrected=True)  # caller order
        sc = np.sqrt(stored * rho1)
        assert np.abs(r - sc * e["raw_r"]).max() <= ptol and wr.rel(J, sc[:, None] * e["raw_J"]) <= 10 * ptol
        P.close(); C.close()


def test_per_point_outputs(hip, oracle, cloud):
    n = 513
    xyz, w = cloud["xyz"][:n], wr.real_weights(n, 11)
    for kind, a in LOSSES:
        e = oracle.OracleProblem(cloud["grid"], *cloud["K"], loss=kind, loss_a=a).eval(xyz, QE, TE, oracle.JAC_JET, materialize=True)
        _, rho1 = wr.loss_pair(kind, a, e["raw_r"] ** 2)
        sc = np.sqrt(w * rho1)
        P = _problem(hip, xyz, cloud["grid"], cloud["K"], hip.EA_F64, (kind, a), w)
        g = P.eval(QE, TE)
        r, J = P.eval_points(QE, TE, corrected=True)
        assert np.abs(r - sc * e["raw_r"]).max() <= 1e-12 and wr.rel(J, sc[:, None] * e["raw_J"]) <= 1e-11
        assert wr.rel(J.T @ J, g["JtJ"]) <= 1e-12 and wr.rel(J.T @ r, g["Jtr"]) <= 1e-12
        r0, J0 = P.eval_points(QE, TE, corrected=False)  # raw and unweighted
        assert np.abs(r0 - e["raw_r"]).max() <= 1e-12 and wr.rel(J0, e["raw_J"]) <= 1e-11
        for layout in (0, 1):
            rr, JJ, bad = P.eval_rows(QE, TE, corrected=True, layout=layout)
            JJ = JJ if layout == 0 else JJ.T
            assert bad == 0 and np.abs(rr - sc * e["raw_r"]).max() <= 1e-12 and wr.rel(JJ, sc[:, None] * e["raw_J"]) <= 1e-11
            assert wr.rel(JJ.T @ JJ, g["JtJ"]) <= 1e-12
            rr, JJ, bad = P.eval_rows(QE, TE, corrected=False, layout=layout)
            JJ = JJ if layout == 0 else JJ.T
            assert bad == 0 and np.abs(rr - e["raw_r"]).max() <= 1e-12 and wr.rel(JJ, e["raw_J"]) <= 1e-11
        P.close()


def _check_solve(q, t, s, oracle_solve, rad=1e-4, m=1e-3, crel=1e-9):
    qo, to, so = oracle_solve
    print("pose", synth.rotation_angle_between(q, qo), np.linalg.norm(t - to), "costs", s["initial_cost"], so["initial_cost"],
          s["final_cost"], so["final_cost"], s["why"], so["why"], s["num_iterations"], so["num_iterations"])
    assert synth.rotation_angle_between(q, qo) < rad and np.linalg.norm(t - to) < m
    assert s["initial_cost"] == pytest.approx(so["initial_cost"], rel=crel)
    assert s["final_cost"] == pytest.approx(so["final_cost"], rel=crel)
    assert s["why"] == so["why"]


@pytest.mark.parametrize("k", [0, 1, 2])
def test_weighted_solve_is_the_solve_of_the_repeated_cloud(hip, solves, k):
    pb = solves[k]
    P = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64, w=pb["w"])
    q, t, s = P.solve(wr.Q0, wr.T0)
    _check_solve(q, t, s, pb["oracle"])
    # a library that ignores the weights ends somewhere else
    P.set_weights(None)
    qu, tu, _ = P.solve(wr.Q0, wr.T0)
    qo, to, _ = pb["oracle"]
    assert synth.rotation_angle_between(qu, qo) > 4e-4 or np.linalg.norm(tu - to) > 1e-3
    P.close()


def test_weighted_solve_dogleg_and_fp32(hip, oracle, solves):
    pb = solves[0]
    O = oracle.OracleProblem(pb["grid"], *pb["K"])
    od = O.solve(pb["repeated"], wr.Q0, wr.T0, strategy=oracle.STRATEGY_DOGLEG)
    P = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64, w=pb["w"])
    q, t, s = P.solve(wr.Q0, wr.T0, strategy=hip.STRATEGY_DOGLEG)
    _check_solve(q, t, s, od)
    P.close()
    P = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F32, w=pb["w"])
    q, t, s = P.solve(wr.Q0, wr.T0)
    qo, to, _ = pb["oracle"]
    assert synth.rotation_angle_between(q, qo) < 1e-4 and np.linalg.norm(t - to) < 1e-3  # (tests/test_gpu_fp32_pose.py)
    P.close()


def test_unit_weights_are_the_variant_path(hip, solves):
    """weights all 1: the bits of a variant-path solve of the unweighted problem (a batch beside a distorted problem puts
    a plain problem on the variant kernels), and within rounding of the plain solve"""
    pb, other = solves[0], solves[1]
    A1 = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64, w=np.ones(len(pb["w"])))
    A0 = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64)
    D = _problem(hip, other["xyz"], other["grid"], other["K"], hip.EA_F64)
    D.set_distortion(1e-3, 0, 0, 0, 0)
    q0, t0 = np.tile(wr.Q0, (2, 1)), np.tile(wr.T0, (2, 1))
    B1, B0 = hip.Batch([A1, D]), hip.Batch([A0, D])
    q1, t1, s1 = B1.solve(q0, t0)
    qv, tv, sv = B0.solve(q0, t0)
    assert B1.info("weighted") == 1 and B0.info("weighted") == 0
    assert np.array_equal(q1[0], qv[0]) and np.array_equal(t1[0], tv[0]) and s1[0]["final_cost"] == sv[0]["final_cost"]
    B1.close(); B0.close()
    qp, tp, sp = A0.solve(wr.Q0, wr.T0)  # the plain kernels
    qw, tw, sw = A1.solve(wr.Q0, wr.T0)
    assert synth.rotation_angle_between(qw, qp) < 1e-9 and np.linalg.norm(tw - tp) < 1e-9
    assert sw["final_cost"] == pytest.approx(sp["final_cost"], rel=1e-10) and sw["why"] == sp["why"]
    A1.close(); A0.close(); D.close()


@pytest.fixture()
def weighted_batch(hip, solves):
    """weighted fp64, unweighted, weighted with a prior on t and t_z held"""
    a, b, c = solves
    Ps = [_problem(hip, a["xyz"], a["grid"], a["K"], hip.EA_F64, w=a["w"]),
          _problem(hip, b["xyz"], b["grid"], b["K"], hip.EA_F64),
          _problem(hip, c["xyz"], c["grid"], c["K"], hip.EA_F64, w=c["w"])]
    Ps[2].set_normal_prior(1, np.eye(3) * 20.0, np.array([0.003, -0.002, 0.004]))
    Ps[2].set_constant_parameters([0, 0, 0, 0, 0, 1])
    B = hip.Batch(Ps)
    yield B, Ps
    B.close()
    for P in Ps:
        P.close()


def test_batch_equals_single(hip, weighted_batch):
    B, Ps = weighted_batch
    q0, t0 = np.tile(wr.Q0, (3, 1)), np.tile(wr.T0, (3, 1))
    qb, tb, sb = B.solve(q0, t0)
    assert B.info("weighted") == 2
    for i, P in enumerate(Ps):
        q, t, s = P.solve(wr.Q0, wr.T0)
        print(i, np.abs(qb[i] - q).max(), np.abs(tb[i] - t).max())
        assert np.abs(qb[i] - q).max() <= 1e-10 and np.abs(tb[i] - t).max() <= 1e-10, i
        assert sb[i]["why"] == s["why"] and sb[i]["final_cost"] == pytest.approx(s["final_cost"], rel=1e-10)
    assert tb[2][2] == 0.0  # held
    g = B.eval(qb, tb)
    for i, P in enumerate(Ps):
        e = P.eval(qb[i], tb[i])
        assert g["cost"][i] == pytest.approx(e["cost"], rel=1e-10) and wr.rel(g["JtJ"][i], e["JtJ"]) <= 1e-10


def test_pose_batched_calls_on_a_weighted_batch(hip, weighted_batch):
    B, Ps = weighted_batch
    rng = np.random.default_rng(5)
    K = 3
    q = np.tile(wr.Q0, (K, 3, 1)) + 0.003 * rng.standard_normal((K, 3, 4))
    q /= np.linalg.norm(q, axis=2)[:, :, None]
    t = 0.004 * rng.standard_normal((K, 3, 3))
    e = B.eval_poses(q, t)
    c = B.cost_poses(q, t)
    assert B.info("cost_form") == 0 and B.info("weighted") == 2
    for k in range(K):
        g = B.eval(q[k], t[k])
        for i in range(3):
            assert e["cost"][k, i] == pytest.approx(g["cost"][i], rel=1e-10)
            assert wr.rel(e["JtJ"][k, i], g["JtJ"][i]) <= 1e-10 and wr.rel(e["Jtr"][k, i], g["Jtr"][i]) <= 1e-10
            assert c["cost"][k, i] == pytest.approx(g["cost"][i], rel=1e-10)
    qs, ts, ss, best = B.solve_starts(q[:2], t[:2])
    assert B.info("starts_form") == 0
    for k in range(2):
        qb, tb, sb = B.solve(q[k], t[k])
        assert np.abs(qs[k] - qb).max() <= 1e-10 and np.abs(ts[k] - tb).max() <= 1e-10, k
        for i in range(3):
            assert ss[k][i]["final_cost"] == pytest.approx(sb[i]["final_cost"], rel=1e-10)


def test_covariance(hip, solves):
    pb = solves[2]
    P = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64, w=pb["w"])
    q, t, _ = P.solve(wr.Q0, wr.T0)
    g = P.eval(q, t)
    c = P.covariance(q, t)
    assert c["ok"] and wr.rel(c["tangent"], np.linalg.pinv(g["JtJ"])) <= 1e-12
    c0 = P.covariance(q, t, apply_loss_function=0)  # the weights go with the loss
    U = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64, loss=(wr.LOSS_TRIVIAL, 1.0))
    cu = U.covariance(q, t)
    assert c0["ok"] and cu["ok"] and wr.rel(c0["tangent"], cu["tangent"]) <= 1e-12
    assert wr.rel(c["tangent"], cu["tangent"]) > 1e-2
    after = P.eval(q, t)  # the problem keeps loss and weights
    assert np.array_equal(after["JtJ"], g["JtJ"])
    P.close(); U.close()


def _depth_weights(z, z_ref, power, f32):
    ratio = z_ref / z
    v = ratio.copy()
    for _ in range(power - 1):
        v = v * ratio
    v = np.minimum(1.0, v)
    return v.astype(np.float32).astype(np.float64) if f32 else v


def _frames(count):
    from oracle import preprocess_np as pp
    return [(pp.load_rgb_as_bgr(os.path.join(G, "rgb_%d.png" % i)), pp.load_depth_u16(os.path.join(G, "depth_%d.png" % i)))
            for i in range(1, count + 1)]


def test_producer_depth_weighting(hip):
    (bgr, depth), = _frames(1)
    K = (525.0, 525.0, 319.5, 239.5)
    for dtype in (hip.EA_F64, hip.EA_F32):
        P = hip.Problem(*K, dtype=dtype)
        P.set_ref_frame(bgr, depth)
        assert P.get_weights() is None and P.num_points > 5000
        for power in (2, 4):
            P.set_depth_weighting(1.0, power)
            P.set_ref_frame(bgr, depth)
            z = P.get_points()[:, 2]
            w = P.get_weights()
            assert w is not None and (w < 1.0).any() and (w > 0.0).all()
            assert np.array_equal(w, _depth_weights(z, 1.0, power, dtype == hip.EA_F32)), (dtype, power)
        P.set_depth_weighting(1.0, 0)  # off again: the weights a producer wrote are gone
        assert P.get_weights() is None
        P.set_ref_frame(bgr, depth)
        assert P.get_weights() is None
        with pytest.raises(hip.EAError):
            P.set_depth_weighting(0.0, 2)
        with pytest.raises(hip.EAError):
            P.set_depth_weighting(1.0, 9)
        P.close()


def test_tracker_with_depth_weighting(hip):
    """the comparison tests/test_gpu_covariance.py makes for the tracker: the same producers on a problem of its own"""
    K = (525.0, 525.0, 319.5, 239.5)
    T = hip.Tracker(*K, dtype=hip.EA_F64, loss=(hip.LOSS_CAUCHY, 1.0))
    T.set_depth_weighting(1.0, 2)
    P = hip.Problem(*K, dtype=hip.EA_F64)
    P.set_loss(hip.LOSS_CAUCHY, 1.0)
    P.set_depth_weighting(1.0, 2)
    U = hip.Problem(*K, dtype=hip.EA_F64)  # without depth weighting
    U.set_loss(hip.LOSS_CAUCHY, 1.0)
    qp, tp = wr.Q0, wr.T0
    for k, (bgr, depth) in enumerate(_frames(3)):
        q, t, s = T.push_frame(bgr, depth)
        if k > 0:
            P.set_now_frame(bgr); U.set_now_frame(bgr)
            q2, t2, s2 = P.solve(qp, tp)
            assert np.abs(q - q2).max() <= 1e-10 and np.abs(t - t2).max() <= 1e-10, k
            assert s["final_cost"] == pytest.approx(s2["final_cost"], rel=1e-10)
            qu, tu, su = U.solve(qp, tp)
            assert np.abs(qu - q2).max() > 1e-9  # the weights were in the tracker's solve
            qp, tp = q, t
        P.set_ref_frame(bgr, depth); U.set_ref_frame(bgr, depth)
        assert P.get_weights() is not None and U.get_weights() is None
    T.close(); P.close(); U.close()


def test_clearing_and_misuse(hip, oracle, cloud):
    n = 257
    xyz, w = cloud["xyz"][:n], wr.real_weights(n, 12)
    O = oracle.OracleProblem(cloud["grid"], *cloud["K"])
    e = O.eval(xyz, QE, TE, oracle.JAC_JET, materialize=True)
    weighted, plain = wr.weighted_sums(e, w), wr.weighted_sums(e, np.ones(n))
    P = _problem(hip, xyz, cloud["grid"], cloud["K"], hip.EA_F64, w=w)
    for bad in (w[:-1], np.concatenate([w, [1.0]])):
        with pytest.raises(hip.EAError) as ei:
            P.set_weights(bad)
        assert ei.value.code == hip.EA_ERR_INVALID_ARG
    for value in (-1e-300, np.nan, np.inf):
        wb = w.copy(); wb[5] = value
        with pytest.raises(hip.EAError) as ei:
            P.set_weights(wb)
        assert ei.value.code == hip.EA_ERR_INVALID_ARG
    assert np.array_equal(P.get_weights(), w)  # untouched
    _check_sums(P.eval(QE, TE), *weighted, 1e-11, "after refused calls")
    P.set_points(xyz)  # a new point set drops the weights
    assert P.get_weights() is None
    _check_sums(P.eval(QE, TE), *plain, 1e-11, "after set_points")
    P.set_weights(w)
    P.set_weights(None)
    assert P.get_weights() is None
    _check_sums(P.eval(QE, TE), *plain, 1e-11, "after clearing")
    P.close()


def test_weights_and_points_from_device_arrays(hip, oracle, cloud):
    """ea_problem_set_weights_device on borrowed points (ea_problem_set_points_device): both are copied"""
    import torch
    n = 513
    xyz, w = cloud["xyz"][:n], wr.real_weights(n, 13)
    e = oracle.OracleProblem(cloud["grid"], *cloud["K"]).eval(xyz, QE, TE, oracle.JAC_JET, materialize=True)
    for dtype, tdt, tol in ((hip.EA_F64, torch.float64, 1e-11), (hip.EA_F32, torch.float32, 2e-4)):
        dev = [torch.tensor(np.ascontiguousarray(a), dtype=tdt, device="cuda") for a in (xyz[:, 0], xyz[:, 1], xyz[:, 2], w)]
        torch.cuda.synchronize()
        P = hip.Problem(*cloud["K"], dtype=dtype)
        P.set_points_device(dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n)
        P.set_dt_grid(cloud["grid"])
        P.set_weights_device(dev[3].data_ptr(), n)
        stored = w if dtype == hip.EA_F64 else w.astype(np.float32).astype(np.float64)
        assert np.array_equal(P.get_weights(), stored)
        del dev  # copied, not borrowed
        _check_sums(P.eval(QE, TE), *wr.weighted_sums(e, w), tol, ("device arrays", dtype))
        P.close()


def test_sharded_single_rank(hip, solves):
    from edge_alignment_amd import dist as ead
    pb = solves[0]
    P = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64, w=pb["w"])
    q, t, s = P.solve(wr.Q0, wr.T0)
    q2, t2, s2 = P.solve_sharded(wr.Q0, wr.T0, ead.make_allreduce(1))
    assert s2["num_iterations"] == s["num_iterations"] and s2["why"] == s["why"]
    assert np.abs(q - q2).max() < 1e-10 and np.abs(t - t2).max() < 1e-10  # (tests/test_gpu_sharded.py)
    _check_solve(q2, t2, s2, pb["oracle"])
    P.close()


def _lcg_weights(count, seed):
    out, s = [], seed
    for _ in range(count):
        s = (s * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        out.append(2.0 * (s >> 40) / 16777216.0)
    return np.array(out)


def test_facade_scaled_loss_example(hip, bundled_pair, tmp_path):
    """examples/weighted_blocks.cpp: one ceres::ScaledLoss per block -> ONE GPU problem, the C-ABI's weighted solve"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples")])
    aX, grid, K = bundled_pair["aX"], bundled_pair["grids"][3], bundled_pair["K"]
    p = str(tmp_path / "pair13.bin")
    W, H = grid.shape
    with open(p, "wb") as f:
        f.write(struct.pack("<iii", aX.shape[1], H, W))
        f.write(struct.pack("<dddd", *K))
        f.write(np.ascontiguousarray(aX.T, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(grid, dtype=np.float64).tobytes())
    stride, seed = 30, 5
    out = subprocess.run([os.path.join(ROOT, "examples", "weighted_blocks"), p, str(stride), str(seed)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    v = [float(x) for x in out.stdout.split()]
    X = np.ascontiguousarray(aX[:3, ::stride].T)
    w = _lcg_weights(X.shape[0], seed)
    assert int(v[11]) == 1 and int(v[12]) == X.shape[0]  # ONE residual family = one GPU problem for N distinct weights
    P = _problem(hip, X, grid, K, hip.EA_F64, w=w)
    q, t, s = P.solve(wr.Q0, wr.T0)
    assert np.abs(np.array(v[:4]) - q).max() <= 1e-12 and np.abs(np.array(v[4:7]) - t).max() <= 1e-12
    assert v[9] == pytest.approx(s["initial_cost"], rel=1e-12) and v[10] == pytest.approx(s["final_cost"], rel=1e-12)
    assert v[13] == pytest.approx(s["initial_cost"], rel=1e-12)  # Problem::Evaluate at the start
    assert int(v[8]) == s["termination"]
    P.set_weights(None)
    qu, tu, _ = P.solve(wr.Q0, wr.T0)
    assert np.abs(qu - q).max() > 1e-9  # the weights mattered
    P.close()
