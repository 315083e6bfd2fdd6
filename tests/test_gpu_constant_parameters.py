"""Constant tangent coordinates on the device (ea_problem_set_constant_parameters): masked solves against the reduced
reference (tests/reduced_lm.py with the oracle's evaluations), the fused and the pair form, batches with a mask per
problem, the all-held case, reduced covariance, priors and terms under a mask, the sharded, pyramid and tracker drivers,
the ceres:: facade, misuse."""
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from edge_alignment_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduced_lm  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "rgbd")
K = (525.0, 525.0, 319.5, 239.5)
Q0, T0 = np.array([1.0, 0, 0, 0]), np.zeros(3)
FREE, Q_HELD, T_HELD, TYZ_HELD, TZ_HELD, D02_HELD = (0,) * 6, (1, 1, 1, 0, 0, 0), (0, 0, 0, 1, 1, 1), (0, 0, 0, 0, 1, 1), (0, 0, 0, 0, 0, 1), (1, 0, 1, 0, 0, 0)
ALL_HELD = (1,) * 6
# a start whose held coordinates are not round numbers
QS, TS = synth.quat_from_axis_angle([0, 1, 0], np.deg2rad(0.2)), np.array([0.001, -0.002, 0.003])


def _synth(seed):
    return synth.make_problem(120, 160, 1500, 40, seed, 130.0, 130.0, 79.5, 59.5,
                              planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)), planted_t=(0.01, -0.005, 0.02),
                              normalize=True, pixel_centres=False)


@pytest.fixture(scope="module")
def data():
    return {seed: _synth(seed) for seed in (21, 22, 23)}


def _problem(hip, pr, dtype=None, held=None):
    P = hip.Problem(*pr["K"], dtype=hip.EA_F64 if dtype is None else dtype)
    P.set_points(pr["xyz"]); P.set_dt_grid(pr["grid"]); P.set_loss(hip.LOSS_CAUCHY, 1.0)
    if held is not None:
        P.set_constant_parameters(held)
    return P


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _held_unchanged(q, t, q0, t0, held):
    for i in range(3):
        if held[3 + i]:
            assert np.float64(t[i]).tobytes() == np.float64(t0[i]).tobytes(), i
    if all(held[:3]):
        assert np.asarray(q).tobytes() == np.asarray(q0, dtype=np.float64).tobytes()


def _same_summary(s1, s2):
    for k in ("termination", "why", "num_iterations", "num_successful_steps", "num_unsuccessful_steps", "initial_cost", "final_cost"):
        assert s1[k] == s2[k], k
    for k in ("it_cost", "it_cost_change", "it_gradient_max_norm", "it_step_norm", "it_relative_decrease", "it_radius",
              "it_successful"):
        assert np.array_equal(s1[k], s2[k]), k


CASES = [(21, Q_HELD, {}), (22, T_HELD, {}), (23, TYZ_HELD, {}), (21, D02_HELD, {}), (22, TZ_HELD, {"min_relative_decrease": 0.75})]


@pytest.mark.parametrize("seed,held,kw", CASES, ids=["q", "t", "tyz", "d02", "tz-rejected"])
def test_masked_fp64_solve_follows_the_reduced_reference(hip, oracle, data, seed, held, kw):
    pr = data[seed]
    O = oracle.OracleProblem(pr["grid"], *pr["K"])
    qr, tr, sr = reduced_lm.solve(lambda q, t: O.eval(pr["xyz"], q, t), oracle.quat_plus, QS, TS, held, **kw)
    if kw:
        assert sr["num_unsuccessful_steps"] >= 1 and 0 in list(sr["it_successful"])  # the reference does reject steps
    P = _problem(hip, pr, held=held)
    assert P.get_constant_parameters() == list(held)
    q, t, s = P.solve(QS, TS, **kw)
    P.close()
    # (tolerances: tests/test_gpu_lm_random.py)
    assert s["why"] == sr["why"] and s["num_iterations"] == sr["num_iterations"] and s["termination"] == sr["termination"]
    assert list(s["it_successful"]) == list(sr["it_successful"])
    assert np.allclose(s["it_cost"], sr["it_cost"], rtol=1e-6, atol=0)
    assert synth.rotation_angle_between(q, qr) < 1e-6 and np.linalg.norm(t - tr) < 1e-6
    _held_unchanged(q, t, QS, TS, held)
    assert s["num_successful_steps"] >= 3 and s["final_cost"] < 0.5 * s["initial_cost"]


@pytest.mark.parametrize("held", [Q_HELD, T_HELD, TYZ_HELD, D02_HELD], ids=["q", "t", "tyz", "d02"])
@pytest.mark.parametrize("strategy", ["lm", "dogleg"])
def test_masked_fp32_solve_properties(hip, data, held, strategy):
    P = _problem(hip, data[21], dtype=hip.EA_F32, held=held)
    q, t, s = P.solve(QS, TS, strategy=hip.STRATEGY_LM if strategy == "lm" else hip.STRATEGY_DOGLEG)
    P.close()
    assert s["termination"] != hip.FAILURE and s["num_successful_steps"] >= 1 and s["final_cost"] < s["initial_cost"]
    _held_unchanged(q, t, QS, TS, held)
    assert not (np.array_equal(q, QS) and np.array_equal(t, TS))


@pytest.mark.parametrize("held", [Q_HELD, TYZ_HELD, FREE], ids=["q", "tyz", "free"])
def test_fused_and_pair_form_give_the_same_bits(hip, data, held):
    P = _problem(hip, data[22], held=held)
    B = hip.Batch([P])
    res = []
    for fused in (1, 0):
        B.set_tuning("fused_iterations", fused)
        q, t, s = B.solve(QS[None], TS[None], min_relative_decrease=0.75)
        assert B.info("fused_iterations") == fused
        res.append((q[0], t[0], s[0]))
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    _same_summary(res[0][2], res[1][2])
    _held_unchanged(res[0][0], res[0][1], QS, TS, held)
    B.close(); P.close()


@pytest.mark.parametrize("streams", [0, 2])
def test_batch_with_mixed_masks_equals_single_solves(hip, data, streams):
    masks = [TYZ_HELD, Q_HELD, FREE, D02_HELD]
    probs = [_problem(hip, data[21 + (i % 3)], held=m if any(m) else None) for i, m in enumerate(masks)]
    B = hip.Batch(probs)
    if streams:
        B.set_tuning("solve_streams", streams)
    n = len(probs)
    qb, tb, sb = B.solve(np.tile(QS, (n, 1)), np.tile(TS, (n, 1)))
    for k, P in enumerate(probs):
        qs, ts, ss = P.solve(QS, TS)
        assert np.array_equal(qb[k], qs) and np.array_equal(tb[k], ts), k
        _same_summary(sb[k], ss)
        _held_unchanged(qb[k], tb[k], QS, TS, masks[k])
    # the unmasked member: the bits of its own solve in an all-unmasked batch
    for P in probs:
        P.set_constant_parameters(None)
    qf, tf, sf = B.solve(np.tile(QS, (n, 1)), np.tile(TS, (n, 1)))
    assert np.array_equal(qf[2], qb[2]) and np.array_equal(tf[2], tb[2])
    _same_summary(sf[2], sb[2])
    assert not np.array_equal(tf[0], tb[0])  # (the others did change)
    B.close()
    for P in probs:
        P.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_all_six_held(hip, data, dtype):
    pr = data[21]
    P = _problem(hip, pr, dtype=hip.EA_F64 if dtype == "f64" else hip.EA_F32, held=ALL_HELD)
    cost, bad = P.cost(QS, TS)
    for strategy in (hip.STRATEGY_LM, hip.STRATEGY_DOGLEG):
        q, t, s = P.solve(QS, TS, strategy=strategy)
        assert s["termination"] == hip.CONVERGENCE and s["why"] == "function_tolerance"
        assert s["num_iterations"] == 0 and s["num_successful_steps"] == 0 and s["num_unsuccessful_steps"] == 0
        assert s["initial_cost"] == s["final_cost"]
        assert abs(s["initial_cost"] - cost) <= 1e-14 * cost if dtype == "f64" else abs(s["initial_cost"] - cost) <= 1e-6 * cost
        assert q.tobytes() == QS.tobytes() and t.tobytes() == TS.tobytes()
    c = P.covariance(QS, TS)
    assert c["ok"] == 1 and c["rank"] == 0 and c["why"] == 0
    for key in ("tangent", "eigenvalues", "qq", "qt", "tt"):
        assert not np.asarray(c[key]).any()
    g = P.eval(QS, TS)   # the evaluation entry points keep the full system
    assert np.all(np.diag(g["JtJ"]) > 0) and np.all(g["Jtr"] != 0)
    # a failed evaluation: FAILURE / initial evaluation failed, the pose untouched
    X = pr["xyz"].copy()
    X[5] = [0.0, 0.0, 0.001]
    P.set_points(X)
    assert P.get_constant_parameters() == list(ALL_HELD)   # survives set_points
    q, t, s = P.solve(QS, TS)
    assert s["termination"] == hip.FAILURE and s["why"] == "initial_eval_failed"
    assert q.tobytes() == QS.tobytes() and t.tobytes() == TS.tobytes()
    P.close()


def _lifted(Cm, q):
    L = np.array([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]])
    return L @ Cm[:3, :3] @ L.T, L @ Cm[:3, 3:], Cm[3:, 3:]


def test_reduced_covariance_against_the_oracle(hip, oracle, data):
    """tolerances of tests/test_gpu_covariance.py: 1e-8 against the oracle's JtJ, 1e-12 against the device's own, 1e-12 for
    the eigenvalues and the lift"""
    pr = data[21]
    O = oracle.OracleProblem(pr["grid"], *pr["K"])
    masks = [Q_HELD, T_HELD, TYZ_HELD, D02_HELD, (1, 1, 1, 1, 1, 0)]
    probs = [_problem(hip, pr, held=m) for m in masks]
    q, t, _ = probs[2].solve(QS, TS)
    eo = O.eval(pr["xyz"], q, t)
    B = hip.Batch(probs)
    cb = B.covariance(np.tile(q, (len(masks), 1)), np.tile(t, (len(masks), 1)))
    for k, (P, held) in enumerate(zip(probs, masks)):
        free = [i for i in range(6) if not held[i]]
        m = len(free)
        h = np.array(held, dtype=bool)
        g = P.eval(q, t)
        assert np.all(np.diag(g["JtJ"]) > 0)   # the evaluation still returns the full 6x6
        for alg in (hip.COV_SPARSE_QR, hip.COV_DENSE_SVD):
            c = P.covariance(q, t, algorithm=alg)
            assert c["ok"] and c["rank"] == m and c["why"] == 0
            want_o, want_g = np.zeros((6, 6)), np.zeros((6, 6))
            want_o[np.ix_(free, free)] = np.linalg.inv(eo["JtJ"][np.ix_(free, free)])
            want_g[np.ix_(free, free)] = np.linalg.inv(g["JtJ"][np.ix_(free, free)])
            assert _rel(c["tangent"], want_o) <= 1e-8
            assert _rel(c["tangent"], want_g) <= 1e-12
            assert not c["tangent"][h].any() and not c["tangent"][:, h].any()
            assert _rel(c["eigenvalues"][:m], np.linalg.eigvalsh(g["JtJ"][np.ix_(free, free)])[::-1]) <= 1e-12
            assert not c["eigenvalues"][m:].any()
            for key, ref in zip(("qq", "qt", "tt"), _lifted(c["tangent"], q)):
                if not ref.any():
                    assert not c[key].any()
                else:
                    assert _rel(c[key], ref) <= 1e-12
        c = P.covariance(q, t)
        assert np.array_equal(cb[k]["tangent"], c["tangent"]) and cb[k]["rank"] == m
        # DENSE_SVD, null_space_rank counts from m
        c1 = P.covariance(q, t, algorithm=hip.COV_DENSE_SVD, null_space_rank=1)
        assert c1["ok"] and c1["rank"] == m - 1
    B.close()
    for P in probs:
        P.close()


def test_prior_on_a_held_block_only_enters_the_cost(hip, data):
    pr = data[22]
    A, b = 30.0 * np.eye(3), np.array([0.02, -0.01, 0.01])
    P = _problem(hip, pr, held=T_HELD)
    q0, t0, s0 = P.solve(QS, TS)
    P.set_normal_prior(1, A, b)
    q1, t1, s1 = P.solve(QS, TS)
    d = A @ (TS - b)
    c = 0.5 * d @ d
    assert t1.tobytes() == TS.tobytes()
    assert s1["initial_cost"] == pytest.approx(s0["initial_cost"] + c, rel=1e-13)
    # a constant added to the cost: the same iterates (the function-tolerance test sees a larger cost and may end the solve
    # an iteration earlier, so compare the steps both took)
    n = min(s0["num_iterations"], s1["num_iterations"])
    assert n >= 3 and list(s0["it_successful"][:n]) == list(s1["it_successful"][:n])
    # (row n of the shorter solve is its terminating iteration, which records no new cost)
    assert np.allclose(np.asarray(s1["it_cost"][:n]) - c, s0["it_cost"][:n], rtol=1e-9, atol=0)
    cov = P.covariance(q1, t1)   # priors first, the mask afterwards: a zero block
    assert cov["ok"] and cov["rank"] == 3 and not cov["tt"].any() and not cov["qt"].any()
    P.close()


def test_second_camera_term_under_a_masked_head(hip, data):
    P = _problem(hip, data[21], held=TYZ_HELD)
    P2 = _problem(hip, data[23])
    T12 = np.eye(4); T12[0, 3] = 0.05
    P2.set_second_camera(T12, np.linalg.inv(T12))
    P.add_term(P2)
    q, t, s = P.solve(QS, TS)
    assert s["termination"] != hip.FAILURE and s["num_successful_steps"] >= 1 and s["final_cost"] < s["initial_cost"]
    _held_unchanged(q, t, QS, TS, TYZ_HELD)
    g = P.eval(q, t)
    # the free coordinates are at a minimum of the two-term problem, the held ones are not
    g0 = P.eval(QS, TS)
    assert np.abs(g["Jtr"][:4]).max() <= 1e-2 * np.abs(g0["Jtr"][:4]).max()
    c = P.covariance(q, t)
    want = np.zeros((6, 6))
    want[:4, :4] = np.linalg.inv(g["JtJ"][:4, :4])
    assert c["ok"] and c["rank"] == 4 and _rel(c["tangent"], want) <= 1e-12
    P.close(); P2.close()


def test_misuse(hip, data):
    import ctypes as C
    P = _problem(hip, data[21])
    P2 = _problem(hip, data[22])
    P3 = _problem(hip, data[23], held=TZ_HELD)
    with pytest.raises(hip.EAError) as ei:   # a problem with a mask cannot become a term
        P.add_term(P3)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    P.add_term(P2)
    with pytest.raises(hip.EAError) as ei:   # a term cannot carry a mask
        P2.set_constant_parameters(TZ_HELD)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    L = hip.load()
    m = (C.c_int * 6)(0, 0, 0, 0, 0, 1)
    assert L.ea_problem_set_constant_parameters(None, m) == hip.EA_ERR_INVALID_ARG
    assert L.ea_problem_get_constant_parameters(None, m) == hip.EA_ERR_INVALID_ARG
    assert L.ea_problem_get_constant_parameters(P.handle, None) == hip.EA_ERR_INVALID_ARG
    # NULL = all variable; any non-zero value holds
    P.set_constant_parameters([0, 0, 7, 0, -1, 0])
    assert P.get_constant_parameters() == [0, 0, 1, 0, 1, 0]
    P.set_constant_parameters(None)
    assert P.get_constant_parameters() == [0] * 6
    P.close(); P2.close(); P3.close()


def test_sharded_forms_apply_the_mask(hip, data):
    import torch
    from edge_alignment_amd import dist as ead
    P = _problem(hip, data[23], held=TYZ_HELD)
    q, t, s = P.solve(QS, TS)
    q2, t2, s2 = P.solve_sharded(QS, TS, ead.make_allreduce(1))
    assert s2["num_iterations"] == s["num_iterations"] and s2["why"] == s["why"]
    assert np.abs(q - q2).max() < 1e-10 and np.abs(t - t2).max() < 1e-10
    _held_unchanged(q2, t2, QS, TS, TYZ_HELD)
    sums, enqueue = ead.make_device_allreduce(1, torch.device("cuda", 0))
    q3, t3, s3 = P.solve_sharded_device(QS, TS, enqueue, sums.data_ptr())
    assert s3["num_iterations"] == s["num_iterations"] and s3["why"] == s["why"]
    assert np.abs(q - q3).max() < 1e-10 and np.abs(t - t3).max() < 1e-10
    _held_unchanged(q3, t3, QS, TS, TYZ_HELD)
    P.close()


def test_pyramid_keeps_held_coordinates_through_every_level(hip, data):
    levels = [_problem(hip, data[21], held=TZ_HELD), _problem(hip, data[22], held=TZ_HELD), _problem(hip, data[23], held=TZ_HELD)]
    q, t, ss = hip.solve_pyramid(levels, QS, TS)
    assert len(ss) == 3 and all(s["termination"] != hip.FAILURE for s in ss)
    assert np.float64(t[2]).tobytes() == np.float64(TS[2]).tobytes()
    assert not np.array_equal(t[:2], TS[:2]) and not np.array_equal(q, QS)
    # each level's own mask: the coarsest level holds q as well
    levels[2].set_constant_parameters((1, 1, 1, 0, 0, 1))
    levels[0].set_constant_parameters((1, 1, 1, 0, 0, 1))
    levels[1].set_constant_parameters((1, 1, 1, 0, 0, 1))
    q2, t2, _ = hip.solve_pyramid(levels, QS, TS)
    assert q2.tobytes() == QS.tobytes() and np.float64(t2[2]).tobytes() == np.float64(TS[2]).tobytes()
    for P in levels:
        P.close()


def test_tracker_with_t_held(hip):
    from oracle import preprocess_np as pp
    seq = [(pp.load_rgb_as_bgr(os.path.join(G, "rgb_%d.png" % i)), pp.load_depth_u16(os.path.join(G, "depth_%d.png" % i)))
           for i in range(1, 5)]
    T = hip.Tracker(*K, dtype=hip.EA_F64, loss=(hip.LOSS_CAUCHY, 1.0))
    T.set_constant_parameters(T_HELD)
    T.set_covariance(True)
    moved = 0
    for k, (bgr, depth) in enumerate(seq):
        q, t, s = T.push_frame(bgr, depth)
        assert t.tobytes() == np.zeros(3).tobytes(), k     # t_rel == 0 exactly, on every push
        if k > 0:
            assert s is not None and s["termination"] != hip.FAILURE
            moved += int(not np.array_equal(q, Q0))
            c = T.last_covariance()
            assert c["ok"] and c["rank"] == 3 and not c["tt"].any() and not c["qt"].any() and c["qq"].any()
    assert moved >= 1
    T.close()


def test_ceres_facade_constant_blocks(hip, bundled_pair, tmp_path):
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
    exe = str(tmp_path / "constant_block_example")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-Wall", "-Werror", "-I", os.path.join(ROOT, "edge_alignment_amd", "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "constant_block_example.cpp"),
                           "-L", lib_dir, "-lea_hip", "-Wl,-rpath," + lib_dir, "-Wl,-rpath,/opt/rocm/lib"])
    start = ["%.17g" % v for v in np.concatenate([QS, TS])]
    want = {0: (FREE, (2, 7, 6)), 1: (T_HELD, (1, 4, 3)), 2: (Q_HELD, (1, 3, 3)), 3: (TYZ_HELD, (2, 7, 4)), 4: (ALL_HELD, (0, 0, 0))}
    for mode, (held, reduced) in want.items():
        out = subprocess.run([exe, path, "30", str(mode)] + start, capture_output=True, text=True, timeout=120)
        assert out.returncode == 0, out.stdout + out.stderr
        v = {ln.split()[0]: np.array([float(x) for x in ln.split()[1:]]) for ln in out.stdout.splitlines() if ln.strip()}
        P = hip.Problem(*bundled_pair["K"])
        P.set_points(aX[:3, ::30].T.copy()); P.set_dt_grid(grid); P.set_loss(hip.LOSS_CAUCHY, 1.0)
        P.set_constant_parameters(held)
        q, t, s = P.solve(QS, TS)
        assert np.array_equal(v["q"], q) and np.array_equal(v["t"], t), mode
        _held_unchanged(v["q"], v["t"], QS, TS, held)
        assert list(v["constant"]) == [float(mode in (2, 4)), float(mode in (1, 4))]
        assert tuple(v["counts"][:3]) == (2, 7, 6) and tuple(v["counts"][3:6]) == reduced
        assert v["counts"][6] == s["num_successful_steps"] + s["num_unsuccessful_steps"] and v["costs"][1] == s["final_cost"]
        assert v["reduced_in_report"][0] == 1 and v["t_variable_again"][0] == 1
        c = P.covariance(q, t, algorithm=hip.COV_DENSE_SVD)
        assert np.array_equal(v["cov_qq"].reshape(4, 4), c["qq"]) and np.array_equal(v["cov_tt"].reshape(3, 3), c["tt"])
        assert np.array_equal(v["cov_qt"].reshape(4, 3), c["qt"])
        if all(held[:3]):
            assert not v["cov_qq"].any() and not v["cov_qt"].any()
        if all(held[3:]):
            assert not v["cov_tt"].any() and not v["cov_qt"].any()
        P.close()
    out = subprocess.run([exe, path, "30", "5"] + start, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and out.stdout.startswith("failed") and "SubsetParameterization" in out.stdout
