"""Exact residual quantiles on the device and auto-scaled losses (ea_*_residual_quantiles, ea_problem_set_loss_auto_scale,
ea_selftest_select): the select kernels alone against numpy's sort, bit for bit; the residual path against the order
statistics of the oracle's raw residuals; batch == single; the auto-scaled solve == the sequence a caller runs by hand
(quantile, set_loss, solve), bit for bit, through ea_solve, ea_batch_solve and ea_solve_pyramid; scale invariance under a DT
image multiplied by 255; the tracker.

The definition the tests restate: m = number of blocks whose functor succeeds, k = floor(prob * (double)(m - 1)) (one IEEE
multiplication), value = the k-th smallest |r|, 0-based."""
import os

import numpy as np
import pytest

from edge_alignment_amd import synth
import weights_ref as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "rgbd")
DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)
QE = synth.quat_mul(synth.quat_from_axis_angle([0.2, -1, 0.4], 0.003), wr.PLANTED_Q)
TE = np.array(wr.PLANTED_T) + 0.001
PROBS = (0.0, 0.1, 0.5, 0.9, 1.0)
# the project's per-point tolerances (tests/test_gpu_parity.py::test_per_point_residuals_and_rows): the k-th order statistic
# of two vectors differs by at most their largest per-element difference
PTOL = {0: 1e-12, 1: 2e-5}  # EA_F64, EA_F32


def rank(prob, m):
    return int(np.floor(np.float64(prob) * np.float64(m - 1)))


def order_stats(absr, probs):
    """the definition on a vector of |r| that may hold NaN (failed blocks) -> (values, m)"""
    a = np.sort(absr[~np.isnan(absr)])
    if a.size == 0:
        return np.full(len(probs), np.nan), 0
    return np.array([a[rank(p, a.size)] for p in probs]), a.size


@pytest.fixture(scope="module")
def cloud():
    """96 x 128, 1025 points (the cloud of tests/test_gpu_weights.py): the tests take its first n points"""
    return synth.make_problem(96, 128, 1025, 24, 21, 130.0, 130.0, 63.5, 47.5, planted_q=wr.PLANTED_Q, planted_t=wr.PLANTED_T)


@pytest.fixture(scope="module")
def raw(oracle, cloud):
    """the oracle's raw residuals of the whole cloud at (QE, TE), plain and distorted: computed once"""
    plain = oracle.OracleProblem(cloud["grid"], *cloud["K"]).eval(cloud["xyz"], QE, TE, oracle.JAC_JET, materialize=True)["raw_r"]
    dist = oracle.OracleProblem(cloud["grid"], *cloud["K"], distortion=DIST).eval(cloud["xyz"], QE, TE, oracle.JAC_JET, materialize=True)["raw_r"]
    assert np.isfinite(plain).all() and np.isfinite(dist).all()
    return dict(plain=plain, dist=dist)


def _problem(hip, xyz, grid, K, dtype, loss=(wr.LOSS_CAUCHY, 1.0)):
    P = hip.Problem(*K, dtype=dtype)
    P.set_points(xyz)
    P.set_dt_grid(grid)
    P.set_loss(*loss)
    return P


# ---- the select kernels alone ---------------------------------------------------------------------------------------------

def _segment(kind, n, rng):
    x = (rng.random(n) - 0.5) * np.exp(20.0 * (rng.random(n) - 0.5))
    if kind == 1:
        x[:] = -0.37
    elif kind == 2:
        x = np.where(rng.random(n) < 0.5, 1.0, np.nextafter(1.0, 2.0))   # differ in the last mantissa bit: every pass decides
    elif kind == 3:
        x = np.where(rng.random(n) < 0.5, 0.0, -0.0)
    elif kind == 4:
        x = rng.integers(0, 1000, n) * 5e-324 * np.where(rng.random(n) < 0.5, 1.0, -1.0)  # denormals
    elif kind == 5:
        x[0::3] = 1e300
        x[1::3] = np.inf
    elif kind == 6:
        x[rng.random(n) < 0.3] = np.nan
    return x


def test_selection_alone_is_bit_exact(hip):
    """every size in ONE call, with an empty and an all-NaN segment; 2049 and 4099: past the 256 keys a workgroup of the key
    pass covers and past the 2048 a workgroup of the histogram pass covers"""
    rng = np.random.default_rng(5)
    probs = np.array([0.0, 0.25, 0.5, 1.0 - 2.0 ** -53, 1.0])
    segs = []
    for n in (1, 2, 63, 64, 65, 255, 256, 257, 1025, 2049, 4099):
        for kind in range(7):
            segs.append(_segment(kind, n, rng))
    segs.insert(3, np.zeros(0))
    segs.insert(11, np.full(300, np.nan))
    segs.append(np.zeros(0))
    values = np.concatenate(segs)
    offsets = np.concatenate([[0], np.cumsum([s.size for s in segs])])
    out, m = hip.selftest_select(values, offsets, probs)
    exp = np.zeros_like(out)
    for i, s in enumerate(segs):
        exp[i], mi = order_stats(np.abs(s), probs)
        assert m[i] == mi, i
    assert m[3] == 0 and m[11] == 0 and np.isnan(out[3]).all() and np.isnan(out[11]).all() and np.isnan(out[-1]).all()
    ok = ~np.isnan(exp)
    assert np.array_equal(np.isnan(out), ~ok)
    assert np.array_equal(out[ok].view(np.uint64), exp[ok].view(np.uint64))
    out2, m2 = hip.selftest_select(values, offsets, probs)
    assert np.array_equal(out2.view(np.uint64), out.view(np.uint64)) and np.array_equal(m2, m)
    # sixteen quantiles that share prefixes pass after pass (equal probabilities included)
    p16 = np.array([0.5, 0.5, 0.0, 1.0, 0.5000001, 0.25, 0.75, 0.1, 0.9, 0.33, 0.66, 0.5, 0.01, 0.99, 0.2, 0.8])
    o16, m16 = hip.selftest_select(segs[-2], [0, segs[-2].size], p16)
    e16, me = order_stats(np.abs(segs[-2]), p16)
    assert m16[0] == me and np.array_equal(o16[0].view(np.uint64), e16.view(np.uint64))


# ---- the residual path against the oracle -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1, 64, 65, 257, 1025])
def test_residual_quantiles_against_the_oracle(hip, cloud, raw, n):
    xyz = cloud["xyz"][:n]
    for dtype in (hip.EA_F64, hip.EA_F32):
        for variant in ("plain", "dist"):
            exp, m = order_stats(np.abs(raw[variant][:n]), PROBS)
            P = _problem(hip, xyz, cloud["grid"], cloud["K"], dtype)
            if variant == "dist":
                P.set_distortion(*DIST)
            v, nv = P.residual_quantiles(QE, TE, PROBS)
            print(n, dtype, variant, "max |device - oracle|", np.abs(v - exp).max())
            assert nv == n == m
            assert np.abs(v - exp).max() <= PTOL[dtype], (n, dtype, variant)
            # every value is an element of the multiset the device itself reports (raw per-point residuals)
            r, _ = P.eval_points(QE, TE, corrected=False)
            assert np.isin(v, np.abs(r)).all()
            dv, _ = order_stats(np.abs(r), PROBS)
            assert np.array_equal(v.view(np.uint64), dv.view(np.uint64))
            # weights do not enter: the same bits with them, with another loss and with a prior
            P.set_weights(wr.real_weights(n, 40 + n))
            P.set_loss(wr.LOSS_HUBER, 0.05)
            P.set_normal_prior(1, np.eye(3), np.zeros(3))
            vw, nw = P.residual_quantiles(QE, TE, PROBS)
            assert nw == n and np.array_equal(vw.view(np.uint64), v.view(np.uint64)), (n, dtype, variant)
            P.close()


def test_failed_blocks_are_left_out(hip, oracle, cloud):
    n = 513
    xyz, idx = wr.plant_failed(cloud["xyz"][:n], QE, TE)
    assert len(idx) == 3
    rr = oracle.OracleProblem(cloud["grid"], *cloud["K"]).eval(xyz, QE, TE, oracle.JAC_JET, materialize=True)["raw_r"]
    exp, m = order_stats(np.abs(rr), PROBS)
    assert m == n - 3 == int(np.isfinite(rr).sum())
    for dtype in (hip.EA_F64, hip.EA_F32):
        P = _problem(hip, xyz, cloud["grid"], cloud["K"], dtype)
        v, nv = P.residual_quantiles(QE, TE, PROBS)
        assert nv == n - 3 and P.eval(QE, TE)["n_invalid"] == 3
        assert np.abs(v - exp).max() <= PTOL[dtype]
        P.close()
    # every block failed: NaN and 0, a result
    P = _problem(hip, xyz[idx], cloud["grid"], cloud["K"], hip.EA_F64)
    v, nv = P.residual_quantiles(QE, TE, PROBS)
    assert nv == 0 and np.isnan(v).all()
    P.close()


def test_second_camera_and_terms(hip, oracle, cloud):
    """the second-camera functor, and a head with a term: the head family only, the term through a call on the term"""
    T12 = np.eye(4)
    T12[:3, :3] = synth.quat_to_R(synth.quat_from_axis_angle([0, 1, 0], 0.02))
    T12[:3, 3] = (0.01, 0.0, -0.005)
    xa, xb = cloud["xyz"][:257], cloud["xyz"][300:900]
    ea = oracle.OracleProblem(cloud["grid"], *cloud["K"]).eval(xa, QE, TE, oracle.JAC_JET, materialize=True)["raw_r"]
    eb = oracle.OracleProblem(cloud["grid"], *cloud["K"], T12=T12).eval(xb, QE, TE, oracle.JAC_JET, materialize=True)["raw_r"]
    for dtype in (hip.EA_F64, hip.EA_F32):
        P = _problem(hip, xa, cloud["grid"], cloud["K"], dtype)
        T = _problem(hip, xb, cloud["grid"], cloud["K"], dtype)
        T.set_second_camera(T12)
        P.add_term(T)
        v, nv = P.residual_quantiles(QE, TE, PROBS)
        exp, m = order_stats(np.abs(ea), PROBS)
        assert nv == m == 257 and np.abs(v - exp).max() <= PTOL[dtype]
        vt, nt = T.residual_quantiles(QE, TE, PROBS)
        expt, mt = order_stats(np.abs(eb), PROBS)
        assert nt == mt and np.abs(vt - expt).max() <= PTOL[dtype]
        with pytest.raises(hip.EAError):
            P.set_loss_auto_scale(2.385)      # a head with terms
        with pytest.raises(hip.EAError):
            T.set_loss_auto_scale(2.385)      # a term
        P.clear_terms()
        P.set_loss_auto_scale(2.385)
        with pytest.raises(hip.EAError):
            P.add_term(T)                     # an auto-scaled head takes no terms
        P.set_loss_auto_scale(0.0)
        T.set_loss_auto_scale(2.385)
        with pytest.raises(hip.EAError):
            P.add_term(T)
        P.close(); T.close()


def test_misuse_and_round_trip(hip, cloud):
    P = hip.Problem(*cloud["K"], dtype=hip.EA_F64)
    assert P.get_loss() == (hip.LOSS_CAUCHY, 1.0) and P.get_loss_auto_scale() == (0.0, 0.5, 1e-6)
    with pytest.raises(hip.EAError) as ei:
        P.residual_quantiles(QE, TE, PROBS)   # no DT image, no points
    assert ei.value.code == hip.EA_ERR_STATE
    P.set_dt_grid(cloud["grid"])
    with pytest.raises(hip.EAError) as ei:
        P.residual_quantiles(QE, TE, PROBS)   # no points
    assert ei.value.code == hip.EA_ERR_STATE
    P.set_loss_auto_scale(1.994, 0.25, 1e-3)
    assert P.get_loss_auto_scale() == (1.994, 0.25, 1e-3)
    P.set_points(cloud["xyz"][:65])           # the setting belongs to the problem, not to its points or image
    P.set_dt_grid(cloud["grid"])
    assert P.get_loss_auto_scale() == (1.994, 0.25, 1e-3)
    for bad in ((-1.0, 0.5, 1e-6), (2.0, 1.5, 1e-6), (2.0, 0.5, 0.0)):
        with pytest.raises(hip.EAError):
            P.set_loss_auto_scale(*bad)
    assert P.get_loss_auto_scale() == (1.994, 0.25, 1e-3)
    with pytest.raises(hip.EAError):
        P.residual_quantiles(QE, TE, np.full(17, 0.5))
    P.close()


# ---- batch == single --------------------------------------------------------------------------------------------------------

def test_batch_equals_single_and_resident_poses_survive(hip, cloud):
    rng = np.random.default_rng(9)
    ns = (1025, 1, 257, 64)
    q = np.array([synth.quat_mul(synth.quat_from_axis_angle(rng.standard_normal(3), 0.004 * (i + 1)), wr.PLANTED_Q) for i in range(4)])
    t = np.array(wr.PLANTED_T) + 0.002 * rng.standard_normal((4, 3))
    for dtype in (hip.EA_F64, hip.EA_F32):
        Ps = [_problem(hip, cloud["xyz"][17 * i:17 * i + n], cloud["grid"], cloud["K"], dtype) for i, n in enumerate(ns)]
        Ps[2].set_distortion(*DIST)
        Ps[3].set_weights(wr.real_weights(64, 3))
        B = hip.Batch(Ps)
        B.set_poses(np.stack([q, q[::-1]]), np.stack([t, t[::-1]]))
        before = B.eval_resident_poses()
        v, m = B.residual_quantiles(q, t, PROBS)
        after = B.eval_resident_poses()
        for key in ("cost", "JtJ", "Jtr"):
            assert np.array_equal(before[key].view(np.uint64), after[key].view(np.uint64)), key
        assert np.array_equal(before["n_invalid"], after["n_invalid"])
        for i, P in enumerate(Ps):
            vi, mi = P.residual_quantiles(q[i], t[i], PROBS)
            assert m[i] == mi == ns[i]
            assert np.array_equal(v[i].view(np.uint64), vi.view(np.uint64)), (dtype, i)
        B.close()
        for P in Ps:
            P.close()


# ---- auto scale == the by-hand sequence -------------------------------------------------------------------------------------

FACTOR, A_MIN = 2.385, 1e-6


def _same_solve(a, b):
    (qa, ta, sa), (qb, tb, sb) = a, b
    assert np.array_equal(qa, qb) and np.array_equal(ta, tb)
    assert sa["num_iterations"] == sb["num_iterations"] and sa["why"] == sb["why"]
    assert np.array_equal(sa["it_cost"].view(np.uint64), sb["it_cost"].view(np.uint64))


def _by_hand(P, q0, t0, prob=0.5):
    v, m = P.residual_quantiles(q0, t0, [prob])
    assert m > 0
    a = max(A_MIN, FACTOR * v[0])
    P.set_loss(P.get_loss()[0], a)
    return a


@pytest.fixture(scope="module")
def solve_clouds():
    return [wr.solve_problem(*spec) for spec in wr.SOLVE_PROBLEMS]


@pytest.mark.parametrize("kind", [wr.LOSS_CAUCHY, wr.LOSS_HUBER])
def test_auto_scale_is_the_by_hand_sequence(hip, solve_clouds, kind):
    for dtype in (hip.EA_F64, hip.EA_F32):
        As = [_problem(hip, pb["xyz"], pb["grid"], pb["K"], dtype, (kind, 1.0)) for pb in solve_clouds]
        Bs = [_problem(hip, pb["xyz"], pb["grid"], pb["K"], dtype, (kind, 1.0)) for pb in solve_clouds]
        for A in As:
            A.set_loss_auto_scale(FACTOR, 0.5, A_MIN)
        # one problem through ea_solve
        a = _by_hand(Bs[0], wr.Q0, wr.T0)
        assert a > A_MIN and a != 1.0
        _same_solve(As[0].solve(wr.Q0, wr.T0), Bs[0].solve(wr.Q0, wr.T0))
        assert As[0].get_loss() == (kind, a)
        # solve_starts does not re-estimate: the problem's current a, as on a problem with that a set by hand
        starts_q = np.stack([wr.Q0, QE])
        starts_t = np.stack([wr.T0, TE])
        qa, ta, sa, ba = As[0].solve_starts(starts_q, starts_t)
        qb, tb, sb, bb = Bs[0].solve_starts(starts_q, starts_t)
        assert np.array_equal(qa, qb) and np.array_equal(ta, tb) and ba == bb and As[0].get_loss() == (kind, a)
        for x, y in zip(sa, sb):
            assert np.array_equal(x["it_cost"].view(np.uint64), y["it_cost"].view(np.uint64))
        # switched off: the loss stays where it was and the next solve does not move it
        As[0].set_loss_auto_scale(0.0)
        As[0].solve(QE, TE)
        assert As[0].get_loss() == (kind, a)
        As[0].set_loss(kind, 1.0)
        As[0].set_loss_auto_scale(FACTOR, 0.5, A_MIN)
        # three problems through ea_batch_solve: one quantile call, each problem its own scale
        q0 = np.stack([wr.Q0] * 3)
        t0 = np.stack([wr.T0] * 3)
        Bs[0].set_loss(kind, 1.0)
        hand = [_by_hand(B, wr.Q0, wr.T0) for B in Bs]
        BA, BB = hip.Batch(As), hip.Batch(Bs)
        qa, ta, sa = BA.solve(q0, t0)
        qb, tb, sb = BB.solve(q0, t0)
        for i in range(3):
            _same_solve((qa[i], ta[i], sa[i]), (qb[i], tb[i], sb[i]))
            assert As[i].get_loss() == (kind, hand[i])
        assert len(set(hand)) == 3
        BA.close(); BB.close()
        for P in As + Bs:
            P.close()


def test_auto_scale_through_the_pyramid(hip, solve_clouds):
    """two levels, each with its own estimate at the pose it starts from"""
    for dtype in (hip.EA_F64, hip.EA_F32):
        lv = [solve_clouds[0], solve_clouds[1]]  # (levels[0] = finest; any two complete problems serve)
        As = [_problem(hip, pb["xyz"], pb["grid"], pb["K"], dtype, (wr.LOSS_CAUCHY, 1.0)) for pb in lv]
        Bs = [_problem(hip, pb["xyz"], pb["grid"], pb["K"], dtype, (wr.LOSS_CAUCHY, 1.0)) for pb in lv]
        for A in As:
            A.set_loss_auto_scale(FACTOR, 0.5, A_MIN)
        qa, ta, sa = hip.solve_pyramid(As, wr.Q0, wr.T0)
        q, t, hand = wr.Q0, wr.T0, {}
        for l in (1, 0):
            hand[l] = _by_hand(Bs[l], q, t)
            q, t, s = Bs[l].solve(q, t)
            assert np.array_equal(s["it_cost"].view(np.uint64), sa[l]["it_cost"].view(np.uint64))
        assert np.array_equal(q, qa) and np.array_equal(t, ta)
        assert As[0].get_loss()[1] == hand[0] and As[1].get_loss()[1] == hand[1] and hand[0] != hand[1]
        for P in As + Bs:
            P.close()


def test_auto_scale_edges(hip, solve_clouds):
    pb = solve_clouds[1]
    # a DT grid of zeros: every residual 0, the clamp
    P = _problem(hip, pb["xyz"], np.zeros_like(pb["grid"]), pb["K"], hip.EA_F64)
    P.set_loss_auto_scale(FACTOR, 0.5, 1e-3)
    P.solve(wr.Q0, wr.T0)
    assert P.get_loss() == (wr.LOSS_CAUCHY, 1e-3)
    P.close()
    # the trivial loss is left alone
    P = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64, (wr.LOSS_TRIVIAL, 1.0))
    U = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64, (wr.LOSS_TRIVIAL, 1.0))
    P.set_loss_auto_scale(FACTOR)
    _same_solve(P.solve(wr.Q0, wr.T0), U.solve(wr.Q0, wr.T0))
    assert P.get_loss() == (wr.LOSS_TRIVIAL, 1.0)
    P.close(); U.close()
    # another probability and factor: the upper quartile
    P = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64, (wr.LOSS_HUBER, 1.0))
    P.set_loss_auto_scale(1.5, 0.75, 1e-6)
    v, _ = P.residual_quantiles(QE, TE, [0.75])
    P.solve(QE, TE)
    assert P.get_loss() == (wr.LOSS_HUBER, max(1e-6, 1.5 * v[0]))
    P.close()


def test_scale_invariance(hip, solve_clouds):
    """the point of the feature: the DT image times 255 gives a times 255 and the same pose"""
    pb = solve_clouds[0]
    P1 = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64)
    P255 = _problem(hip, pb["xyz"], pb["grid"] * 255.0, pb["K"], hip.EA_F64)
    for P in (P1, P255):
        P.set_loss_auto_scale(FACTOR, 0.5, A_MIN)
    q1, t1, s1 = P1.solve(wr.Q0, wr.T0)
    q2, t2, s2 = P255.solve(wr.Q0, wr.T0)
    a1, a2 = P1.get_loss()[1], P255.get_loss()[1]
    print("a", a1, a2, "rel", abs(a2 - 255.0 * a1) / (255.0 * a1), "angle", synth.rotation_angle_between(q1, q2), "dt", np.linalg.norm(t1 - t2))
    assert abs(a2 - 255.0 * a1) <= 1e-12 * 255.0 * a1
    # (the tolerance tests/test_gpu_lm_random.py holds device and oracle poses to)
    assert synth.rotation_angle_between(q1, q2) < 1e-6 and np.linalg.norm(t1 - t2) < 1e-6
    # with CauchyLoss(1.) fixed the two images are different problems: the iterates part
    F1 = _problem(hip, pb["xyz"], pb["grid"], pb["K"], hip.EA_F64)
    F255 = _problem(hip, pb["xyz"], pb["grid"] * 255.0, pb["K"], hip.EA_F64)
    qf1, tf1, _ = F1.solve(wr.Q0, wr.T0, max_num_iterations=3)
    qf2, tf2, _ = F255.solve(wr.Q0, wr.T0, max_num_iterations=3)
    assert synth.rotation_angle_between(qf1, qf2) > 1e-6 or np.linalg.norm(tf1 - tf2) > 1e-6
    for P in (P1, P255, F1, F255):
        P.close()


def test_tracker_estimates_per_push(hip):
    from oracle import preprocess_np as pp
    K = (525.0, 525.0, 319.5, 239.5)
    T = hip.Tracker(*K, dtype=hip.EA_F64, loss=(hip.LOSS_CAUCHY, 1.0))
    T.set_loss_auto_scale(FACTOR, 0.5, A_MIN)
    assert T.get_loss() == (hip.LOSS_CAUCHY, 1.0)
    for i in (1, 2):
        bgr = pp.load_rgb_as_bgr(os.path.join(G, "rgb_%d.png" % i))
        depth = pp.load_depth_u16(os.path.join(G, "depth_%d.png" % i))
        q, t, s = T.push_frame(bgr, depth)
    assert s is not None
    kind, a = T.get_loss()
    assert kind == hip.LOSS_CAUCHY and a != 1.0 and a >= A_MIN
    T.close()
