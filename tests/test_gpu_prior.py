"""ceres::NormalPrior on the device: ea_eval / batches / covariance include the prior's terms at the evaluated pose, every
solve driver (single, batch, sharded, pyramid, tracker, ceres:: facade) carries it, and a problem without a prior runs
exactly as before (set-then-clear is bit-identical to never set)."""
import os
import struct
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "rgbd")
K = (525.0, 525.0, 319.5, 239.5)
Q0, T0 = np.array([1.0, 0, 0, 0]), np.zeros(3)


def _P(q):
    return np.array([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]])


def _prior_terms(q, t, Aq=None, bq=None, At=None, bt=None):
    JtJ, Jtr, cost = np.zeros((6, 6)), np.zeros(6), 0.0
    if Aq is not None:
        H = Aq.T @ Aq
        d = np.asarray(q) - bq
        JtJ[:3, :3] += _P(q).T @ H @ _P(q)
        Jtr[:3] += _P(q).T @ H @ d
        cost += 0.5 * d @ H @ d
    if At is not None:
        H = At.T @ At
        d = np.asarray(t) - bt
        JtJ[3:, 3:] += H
        Jtr[3:] += H @ d
        cost += 0.5 * d @ H @ d
    return JtJ, Jtr, cost


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _bundled(hip, bundled_pair, stride, dtype=None):
    P = hip.Problem(*bundled_pair["K"], dtype=hip.EA_F64 if dtype is None else dtype)
    X = bundled_pair["aX"][:3, ::stride].T.copy()
    P.set_points(X)
    P.set_dt_grid(bundled_pair["grids"][3])
    return P, X


RNG = np.random.default_rng(2024)
AQ, BQ = RNG.normal(size=(3, 4)) * 30.0, np.array([0.999, 0.01, -0.02, 0.015])
AT, BT = RNG.normal(size=(2, 3)) * 20.0, np.array([0.01, -0.02, 0.03])


def _same_summary(s1, s2):
    for k in ("termination", "why", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost"):
        assert s1[k] == s2[k], k
    for k in ("it_cost", "it_cost_change", "it_gradient_max_norm", "it_step_norm", "it_relative_decrease", "it_radius",
              "it_successful"):
        assert np.array_equal(s1[k], s2[k]), k


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_eval_adds_the_prior_terms(hip, bundled_pair, dtype):
    P, _ = _bundled(hip, bundled_pair, 30, hip.EA_F64 if dtype == "f64" else hip.EA_F32)
    q = np.array([0.9995, 0.01, -0.02, 0.015]); q /= np.linalg.norm(q)
    t = np.array([0.02, -0.01, 0.03])
    g0 = P.eval(q, t)
    r0, J0 = P.eval_points(q, t)
    P.set_normal_prior(0, AQ, BQ)
    P.set_normal_prior(1, AT, BT)
    g1 = P.eval(q, t)
    J, r, c = _prior_terms(q, t, AQ, BQ, AT, BT)
    assert _rel(g1["JtJ"], g0["JtJ"] + J) <= 1e-12
    assert _rel(g1["Jtr"], g0["Jtr"] + r) <= 1e-12
    assert abs(g1["cost"] - (g0["cost"] + c)) <= 1e-12 * (g0["cost"] + c)
    cost, bad = P.cost(q, t)
    assert cost == g1["cost"] and bad == 0
    _, _, s = P.solve(q, t)
    assert abs(s["initial_cost"] - cost) <= 1e-14 * cost
    r1, J1 = P.eval_points(q, t)  # per-point outputs stay prior-free
    assert np.array_equal(r0, r1) and np.array_equal(J0, J1)
    P.clear_normal_prior(0)
    P.clear_normal_prior(1)
    g2 = P.eval(q, t)
    assert g2["cost"] == g0["cost"] and np.array_equal(g2["JtJ"], g0["JtJ"])
    P.close()


def test_argument_checks(hip, bundled_pair):
    P, _ = _bundled(hip, bundled_pair, 30)
    for args in ((2, AQ, BQ), (-1, AT, BT), (0, np.full((1, 4), np.nan), BQ), (1, AT, np.array([0.0, np.inf, 0.0]))):
        with pytest.raises(hip.EAError) as ei:
            P.set_normal_prior(*args)
        assert ei.value.code == hip.EA_ERR_INVALID_ARG
    import ctypes as C
    A = (C.c_double * 12)(*([1.0] * 12))
    assert hip.load().ea_problem_set_normal_prior(P.handle, 1, A, 4, None) == hip.EA_ERR_INVALID_ARG   # b missing
    assert hip.load().ea_problem_set_normal_prior(P.handle, 1, A, -1, A) == hip.EA_ERR_INVALID_ARG     # k < 0
    P.close()


@pytest.mark.parametrize("stride", [30, 1])
@pytest.mark.parametrize("strategy", ["lm", "dogleg"])
def test_prior_solve_and_strong_prior(hip, bundled_pair, stride, strategy):
    st = hip.STRATEGY_LM if strategy == "lm" else hip.STRATEGY_DOGLEG
    P, _ = _bundled(hip, bundled_pair, stride)
    q0, t0, s0 = P.solve(Q0, T0, strategy=st)
    # set then clear: bit-identical to never set
    P.set_normal_prior(0, AQ, BQ); P.set_normal_prior(1, AT, BT)
    qp, tp, sp = P.solve(Q0, T0, strategy=st)
    assert sp["termination"] != hip.FAILURE
    P.clear_normal_prior(0); P.clear_normal_prior(1)
    q1, t1, s1 = P.solve(Q0, T0, strategy=st)
    assert np.array_equal(q0, q1) and np.array_equal(t0, t1)
    _same_summary(s0, s1)
    # at the prior solve's end the total gradient (prior included) is small against the cost scale
    P.set_normal_prior(0, AQ, BQ); P.set_normal_prior(1, AT, BT)
    g = P.eval(qp, tp)
    g_start = P.eval(Q0, T0)
    assert np.abs(g["Jtr"]).max() <= 1e-2 * np.abs(g_start["Jtr"]).max()
    assert sp["initial_cost"] == pytest.approx(g_start["cost"], rel=1e-14)
    assert sp["final_cost"] == pytest.approx(g["cost"], rel=1e-9)
    # a strong prior pins the pose to b
    bq = np.array([0.9998, 0.01, -0.01, 0.012]); bq /= np.linalg.norm(bq)
    bt = np.array([0.03, -0.01, 0.02])
    P.set_normal_prior(0, 1e6 * np.eye(4), bq); P.set_normal_prior(1, 1e6 * np.eye(3), bt)
    qs, ts, ss = P.solve(Q0, T0, strategy=st)
    assert np.abs(qs - bq).max() < 1e-6 and np.abs(ts - bt).max() < 1e-6
    # a vanishing prior reproduces the prior-free solve
    P.set_normal_prior(0, 1e-12 * np.eye(4), bq); P.set_normal_prior(1, 1e-12 * np.eye(3), bt)
    qv, tv, sv = P.solve(Q0, T0, strategy=st)
    assert sv["num_iterations"] == s0["num_iterations"] and sv["why"] == s0["why"]
    assert np.abs(qv - q0).max() < 1e-7 and np.abs(tv - t0).max() < 1e-7
    P.close()


def test_batch_mixed_priors_equal_single_solves(hip, bundled_pair):
    probs, single = [], []
    for i in range(8):
        dt = hip.EA_F64 if i % 2 == 0 else hip.EA_F32
        P, _ = _bundled(hip, bundled_pair, 20 + i, dt)
        if i % 3 == 1:
            P.set_normal_prior(0, AQ * (1 + i), BQ)
        if i % 3 == 2:
            P.set_normal_prior(1, AT * (1 + 0.5 * i), BT)
            P.set_normal_prior(0, AQ, BQ)
        probs.append(P)
    for dt in (hip.EA_F64, hip.EA_F32):
        group = [P for P in probs if P.dtype == dt]
        B = hip.Batch(group)
        n = len(group)
        q = np.tile(Q0, (n, 1)); t = np.tile(T0, (n, 1))
        qb, tb, sb = B.solve(q, t)
        for k, P in enumerate(group):
            qs, ts, ss = P.solve(Q0, T0)
            assert np.array_equal(qb[k], qs) and np.array_equal(tb[k], ts), k
            _same_summary(sb[k], ss)
        # K poses per problem: each equals ea_eval at that pose (to rounding: the pose path cuts its own chunks)
        Kp = 3
        qk = np.tile(qb, (Kp, 1, 1)); tk = np.tile(tb, (Kp, 1, 1))
        tk[1] += 0.01; tk[2] -= 0.02
        e = B.eval_poses(qk.reshape(Kp, n, 4), tk.reshape(Kp, n, 3))
        tolk = 1e-10 if dt == hip.EA_F64 else 1e-4  # (fp32: the tolerance of test_gpu_eval_poses.py)
        for k in range(Kp):
            for j, P in enumerate(group):
                g = P.eval(qk[k, j], tk[k, j])
                assert _rel(e["JtJ"][k, j], g["JtJ"]) <= tolk and _rel(e["Jtr"][k, j], g["Jtr"]) <= tolk
                assert abs(e["cost"][k, j] - g["cost"]) <= tolk * g["cost"]
        B.close()
    for P in probs:
        P.close()


def test_covariance_includes_the_prior(hip, bundled_pair):
    P, X = _bundled(hip, bundled_pair, 30)
    P.set_normal_prior(0, AQ, BQ); P.set_normal_prior(1, AT, BT)
    q, t, s = P.solve(Q0, T0)
    for loss_on in (1, 0):
        c = P.covariance(q, t, apply_loss_function=loss_on)
        assert c["ok"] and c["rank"] == 6
        if loss_on:
            assert _rel(c["tangent"], np.linalg.inv(P.eval(q, t)["JtJ"])) <= 1e-10
    B = hip.Batch([P])
    cb = B.covariance(q[None], t[None])[0]
    assert _rel(cb["tangent"], P.covariance(q, t)["tangent"]) <= 1e-12
    B.close()
    # the one-point problem (rank 1) is full rank with priors on q and t
    P1 = hip.Problem(*bundled_pair["K"])
    P1.set_points(X[:1])
    P1.set_dt_grid(bundled_pair["grids"][3])
    assert not P1.covariance(Q0, T0)["ok"]
    P1.set_normal_prior(0, 10.0 * np.eye(4), Q0); P1.set_normal_prior(1, 10.0 * np.eye(3), T0)
    c = P1.covariance(Q0, T0)
    assert c["ok"] and c["rank"] == 6 and c["why"] == 0
    assert _rel(c["tangent"], np.linalg.inv(P1.eval(Q0, T0)["JtJ"])) <= 1e-10
    P.close(); P1.close()


def test_sharded_forms_add_the_prior_once(hip, bundled_pair):
    import torch
    from edge_alignment_amd import dist as ead
    P, _ = _bundled(hip, bundled_pair, 30)
    P.set_loss(hip.LOSS_CAUCHY, 1.0)
    P.set_normal_prior(0, AQ, BQ); P.set_normal_prior(1, AT, BT)
    q, t, s = P.solve(Q0, T0)
    q2, t2, s2 = P.solve_sharded(Q0, T0, ead.make_allreduce(1))
    assert s2["num_iterations"] == s["num_iterations"] and s2["why"] == s["why"]
    assert np.abs(q - q2).max() < 1e-10 and np.abs(t - t2).max() < 1e-10
    sums, enqueue = ead.make_device_allreduce(1, torch.device("cuda", 0))
    q3, t3, s3 = P.solve_sharded_device(Q0, T0, enqueue, sums.data_ptr())
    assert s3["num_iterations"] == s["num_iterations"] and s3["why"] == s["why"]
    assert np.abs(q - q3).max() < 1e-10 and np.abs(t - t3).max() < 1e-10
    P.close()


def test_second_camera_term_and_prior(hip, bundled_pair):
    P, X = _bundled(hip, bundled_pair, 30)
    P2, _ = _bundled(hip, bundled_pair, 40)
    T12 = np.eye(4); T12[0, 3] = 0.05
    P2.set_second_camera(T12, np.linalg.inv(T12))
    P.set_normal_prior(1, AT, BT)
    P.add_term(P2)
    q, t, s = P.solve(Q0, T0)
    assert s["termination"] != hip.FAILURE
    g = P.eval(q, t)
    P.clear_normal_prior(1)
    g0 = P.eval(q, t)
    J, r, c = _prior_terms(q, t, At=AT, bt=BT)
    assert _rel(g["JtJ"], g0["JtJ"] + J) <= 1e-12
    # a term cannot carry a prior, a problem with a prior cannot become a term
    with pytest.raises(hip.EAError) as ei:
        P2.set_normal_prior(1, AT, BT)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    P3, _ = _bundled(hip, bundled_pair, 50)
    P3.set_normal_prior(0, AQ, BQ)
    with pytest.raises(hip.EAError) as ei:
        P.add_term(P3)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    P.close(); P2.close(); P3.close()


def test_tracker_motion_prior(hip):
    from oracle import preprocess_np as pp
    seq = [(pp.load_rgb_as_bgr(os.path.join(G, "rgb_%d.png" % i)), pp.load_depth_u16(os.path.join(G, "depth_%d.png" % i)))
           for i in range(1, 6)]
    Toff = hip.Tracker(*K, dtype=hip.EA_F64)
    Tdef = hip.Tracker(*K, dtype=hip.EA_F64)
    Tdef.set_motion_prior(0.0, 0.0)
    Ton = hip.Tracker(*K, dtype=hip.EA_F64)
    sr, st_ = 0.02, 0.05
    Ton.set_motion_prior(sr, st_)
    Ton.set_covariance(True)
    Ttiny = hip.Tracker(*K, dtype=hip.EA_F64)
    Ttiny.set_motion_prior(1e-9, 1e-9)
    M = hip.Problem(*K, dtype=hip.EA_F64)
    pq, pt = Q0.copy(), T0.copy()
    for k, (bgr, depth) in enumerate(seq):
        a = Toff.push_frame(bgr, depth)
        b = Tdef.push_frame(bgr, depth)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        q, t, s = Ton.push_frame(bgr, depth)
        qt_, tt_, _ = Ttiny.push_frame(bgr, depth)
        if k > 0:
            # the manual sequence: this frame's DT image, priors at the start pose (the previous relative pose), ea_solve
            M.set_now_frame(bgr)
            M.set_normal_prior(0, np.eye(4) / sr, pq); M.set_normal_prior(1, np.eye(3) / st_, pt)
            qm, tm, sm = M.solve(pq, pt)
            assert np.array_equal(q, qm) and np.array_equal(t, tm), k
            _same_summary(s, sm)
            c, cm = Ton.last_covariance(), M.covariance(qm, tm)  # tracker covariance includes the motion prior
            assert c["ok"] and cm["ok"] and _rel(c["tangent"], cm["tangent"]) <= 1e-10
            assert _rel(c["tangent"], np.linalg.inv(M.eval(qm, tm)["JtJ"])) <= 1e-10
            assert np.abs(qt_ - Q0).max() < 1e-6 and np.abs(tt_ - T0).max() < 1e-6  # held at the prediction (identity)
        M.set_ref_frame(bgr, depth)
        pq, pt = q, t
    Toff.close(); Tdef.close(); Ton.close(); Ttiny.close(); M.close()


def test_ceres_facade_normal_prior(hip, bundled_pair, tmp_path):
    from edge_alignment_amd import capi
    lib_dir = os.path.dirname(capi.LIB_PATH)
    grid = bundled_pair["grids"][3]
    W, H = grid.shape
    aX = bundled_pair["aX"]
    path = str(tmp_path / "problem.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", aX.shape[1], H, W))
        f.write(struct.pack("<dddd", *bundled_pair["K"]))
        f.write(np.ascontiguousarray(aX.T, dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(grid, dtype=np.float64).tobytes())
    At, bt = 20.0 * np.eye(3), np.array([0.01, -0.02, 0.005])
    Aq, bq = 50.0 * np.eye(4), np.array([1.0, 0, 0, 0])
    for eigen_like in (False, True):
        exe = str(tmp_path / ("normal_prior_example%d" % eigen_like))
        cmd = ["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "edge_alignment_amd", "include"),
               "-o", exe, os.path.join(ROOT, "tests", "cpp", "normal_prior_example.cpp"),
               "-L", lib_dir, "-lea_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"]
        if eigen_like:
            cmd.insert(1, "-DEA_EIGEN_LIKE")
        subprocess.check_call(cmd)
        for on_q in (0, 1):
            out = subprocess.run([exe, path, "30", str(on_q)], capture_output=True, text=True, timeout=120)
            assert out.returncode == 0, out.stdout + out.stderr
            v = {ln.split()[0]: np.array([float(x) for x in ln.split()[1:]]) for ln in out.stdout.splitlines() if ln.strip()}
            P = hip.Problem(*bundled_pair["K"])
            P.set_points(aX[:3, ::30].T.copy()); P.set_dt_grid(grid); P.set_loss(hip.LOSS_CAUCHY, 1.0)
            P.set_normal_prior(1, At, bt)
            if on_q:
                P.set_normal_prior(0, Aq, bq)
            q, t, s = P.solve(Q0, T0)
            assert np.array_equal(v["q"], q) and np.array_equal(v["t"], t)
            nea, nres, nrows, nprob = v["counts"]
            assert nres == nea + 3 + 4 * on_q and nrows == nres and nprob == nres
            assert np.allclose(v["prior_rows"][:3], At @ (t - bt), rtol=1e-12, atol=1e-15)
            Jp = v["prior_jacobian"].reshape(-1, 6)
            assert not Jp[:3, :3].any() and np.array_equal(Jp[:3, 3:], At)
            if on_q:
                assert np.allclose(v["prior_rows"][3:], Aq @ (q - bq), rtol=1e-12, atol=1e-15)
                assert np.allclose(Jp[3:, :3], Aq @ _P(q), rtol=1e-12, atol=1e-15) and not Jp[3:, 3:].any()
            g = P.eval(q, t)
            assert _rel(v["gradient"], g["Jtr"]) <= 1e-12
            P.close()
