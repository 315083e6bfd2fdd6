"""Cost-only pose-batched evaluation (ea_batch_cost_poses / ea_batch_cost_resident_poses: ea_cost_poses_kernel + ea_cost_fold_kernel)
and the ranked search in front of the multi-start solve (ea_batch_search_starts), on the 120 x 160 synthetic problem of
test_gpu_poses_flat.py (9000 points, Cauchy 0.7) and on one odd image (37 x 53, 300 points) for the border pad.

Bars, all from the project: against the oracle's cost 1e-11 (fp64) / 1e-4 (fp32) relative (test_gpu_eval_poses.py); against
ea_batch_eval_poses' cost at the same pose 1e-12 / 1e-5, the bar between launch shapes -- the same points summed in another
order; n_invalid exactly.  The same pose alone, in any split over launches, twice, in other company and in either item order:
the same bits.  Batches the cost kernel does not cover run the full evaluation (cost_form 0): 1e-13, the same kernel.
The search: `picked` is a stable numpy ranking of what cost_poses returns, and everything behind it is bit for bit what
solve_starts returns from the picked poses."""
import numpy as np
import pytest

import border_band as bb
from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

DTYPES = [("EA_F64", 1e-11, 1e-12), ("EA_F32", 1e-4, 1e-5)]


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _poses(rng, K, n, scale=1.0):
    q = np.zeros((K, n, 4)); t = np.zeros((K, n, 3))
    for k in range(K):
        for i in range(n):
            q[k, i] = synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(scale * rng.uniform(0.0, 1.5)))
            t[k, i] = scale * rng.uniform(-0.03, 0.03, size=3)
    return q, t


@pytest.fixture(scope="module")
def base():
    return synth.make_problem(120, 160, 9000, 40, 1, 130.0, 130.0, 79.5, 59.5,
                              planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)),
                              planted_t=(0.01, -0.005, 0.02), normalize=True)


def _problem(hip, base, dtype, n, rng=None, loss=None, grid=None):
    X = base["xyz"][:n] if rng is None else base["xyz"][rng.choice(9000, n, replace=False)]
    P = hip.Problem(*base["K"], dtype=dtype)
    P.set_points(X.reshape(-1, 3)); P.set_dt_grid(base["grid"] if grid is None else grid)
    P.set_loss(*(loss or (hip.LOSS_CAUCHY, 0.7)))
    return P


def _against_eval_poses(B, q, t, got, tol, where=()):
    """cost_poses' result against ea_batch_eval_poses at the same poses; leaves (q, t) resident"""
    ref = B.eval_poses(q, t)
    for k in range(q.shape[0]):
        for i in range(q.shape[1]):
            d = abs(got["cost"][k, i] - ref["cost"][k, i])
            assert d <= tol * abs(ref["cost"][k, i]), where + (k, i, d, ref["cost"][k, i])
    assert np.array_equal(got["n_invalid"], ref["n_invalid"]), where
    return ref


@pytest.mark.parametrize("dtype_name,tol,ppt", [("EA_F64", 1e-12, 0), ("EA_F32", 1e-5, 0), ("EA_F32", 1e-5, 4)])
def test_chunk_edges(hip, base, dtype_name, tol, ppt):
    dtype = getattr(hip, dtype_name)
    rng = np.random.default_rng(41)
    sizes = (1, 511, 512, 513, 3585, 4097, 6145)
    probs = [_problem(hip, base, dtype, n, rng) for n in sizes]
    empty = _problem(hip, base, dtype, 0)
    batches = [hip.Batch([P]) for P in probs] + [hip.Batch(probs[:3] + [empty] + probs[3:])]
    try:
        for B in batches:
            n = len(B)
            if ppt:
                B.set_tuning("points_per_thread", ppt)
            for K in (1, 3, 8, 11):
                q, t = _poses(rng, K, n)
                got = None
                for order in (0, 1):
                    B.set_tuning("poses_order", order)
                    out = B.cost_poses(q, t)
                    assert B.info("cost_form") == 1 and B.info("poses_threads") == 256
                    assert B.info("poses_points_per_thread") == (ppt or 2)
                    assert out["cost"].shape == (K, n) and out["n_invalid"].shape == (K, n)
                    if got is None:
                        got = out
                        _against_eval_poses(B, q, t, got, tol, (n, K))
                    assert np.array_equal(out["cost"], got["cost"]) and np.array_equal(out["n_invalid"], got["n_invalid"]), (n, K, order)
                for k in range(K):   # the pose alone in a call of its own: the same bits
                    one = B.cost_poses(q[k:k + 1], t[k:k + 1])
                    assert np.array_equal(one["cost"][0], got["cost"][k]) and np.array_equal(one["n_invalid"][0], got["n_invalid"][k]), (n, K, k)
                if n > 1:
                    assert not got["cost"][:, 3].any() and not got["n_invalid"][:, 3].any()
                    assert (got["cost"][:, 4:] > 0).all()
    finally:
        for B in batches:
            B.close()
        for P in probs + [empty]:
            P.close()


@pytest.mark.parametrize("dtype_name,tol,tol_eval", DTYPES)
def test_against_the_oracle(hip, oracle, base, dtype_name, tol, tol_eval):
    dtype = getattr(hip, dtype_name)
    rng = np.random.default_rng(23)
    clouds = [base["xyz"][rng.choice(9000, n, replace=False)] for n in (9000, 257, 4097)]
    probs = []
    for X in clouds:
        P = hip.Problem(*base["K"], dtype=dtype)
        P.set_points(X); P.set_dt_grid(base["grid"]); P.set_loss(hip.LOSS_CAUCHY, 0.7)
        probs.append(P)
    O = oracle.OracleProblem(base["grid"], *base["K"], loss=hip.LOSS_CAUCHY, loss_a=0.7)
    B = hip.Batch(probs)
    try:
        q, t = _poses(rng, 3, 3)
        q[0, 0] = [1.0, 0, 0, 0]; t[0, 0] = 0.0
        got = B.cost_poses(q, t)
        assert B.info("cost_form") == 1
        for k in range(3):
            for i in range(3):
                e = O.eval(clouds[i], q[k, i], t[k, i])
                d = abs(got["cost"][k, i] - e["cost"])
                print(dtype_name, k, i, "cost", got["cost"][k, i], "oracle", e["cost"], "rel", d / abs(e["cost"]))
                assert d <= tol * abs(e["cost"]), (k, i)
                assert got["n_invalid"][k, i] == e["n_invalid"] == 0
        _against_eval_poses(B, q, t, got, tol_eval)
    finally:
        B.close()
        for P in probs:
            P.close()


@pytest.mark.parametrize("dtype_name,tol,tol_eval", DTYPES)
def test_same_bits_in_any_split_order_and_company(hip, base, dtype_name, tol, tol_eval):
    dtype = getattr(hip, dtype_name)
    rng = np.random.default_rng(43)
    probs = [_problem(hip, base, dtype, n, rng) for n in (4097, 700)]
    B = hip.Batch(probs)

    def same(a, b):
        return np.array_equal(a["cost"], b["cost"]) and np.array_equal(a["n_invalid"], b["n_invalid"])

    try:
        for K in (5, 20):
            q, t = _poses(rng, K, 2)
            first = None
            for g in (1, 2, 3, 0):
                B.set_tuning("poses_per_launch", g)
                B.set_poses(q, t)
                before = B.eval_resident_poses()
                out = B.cost_resident_poses()
                assert B.info("cost_form") == 1
                out["cost"][...] = np.nan; out["n_invalid"][...] = -1   # filled again: every result of every launch is unpacked
                B.cost_resident_poses(out=out)
                assert not np.isnan(out["cost"]).any() and (out["n_invalid"] >= 0).all(), (K, g)
                first = first or dict(cost=out["cost"].copy(), n_invalid=out["n_invalid"].copy())
                assert same(out, first), (K, g)
                assert same(B.cost_resident_poses(), first), (K, g)           # twice
                B.cost_resident_poses(fetch=False)                            # nothing fetched, then fetched
                assert same(B.cost_resident_poses(), first), (K, g)
                for order in (1, 0):                                          # the other item order: the same rows, the same fold
                    B.set_tuning("poses_order", order)
                    assert same(B.cost_resident_poses(), first), (K, g, order)
                # the full evaluation of the same resident poses is what it was before the cost calls
                after = B.eval_resident_poses()
                assert all(np.array_equal(after[f], before[f]) for f in ("cost", "JtJ", "Jtr", "n_invalid")), (K, g)
                for f in ("cost",):
                    assert _rel(first[f], before[f]) <= tol_eval, (K, g)
                assert np.array_equal(first["n_invalid"], before["n_invalid"])
            # other company: a few of the poses, reversed, among fresh ones
            q2, t2 = _poses(rng, 7, 2)
            pick = [K - 1, 2, 0]
            q2[[1, 4, 6]] = q[pick]; t2[[1, 4, 6]] = t[pick]
            mixed = B.cost_poses(q2, t2)
            assert np.array_equal(mixed["cost"][[1, 4, 6]], first["cost"][pick]), K
            assert np.array_equal(mixed["n_invalid"][[1, 4, 6]], first["n_invalid"][pick]), K
    finally:
        B.close()
        for P in probs:
            P.close()


def test_image_forms(hip, base):
    """an fp64 problem over an exact fp32 mirror, an fp64 problem whose grid is not float-representable (fp64 image path),
    an fp32 problem"""
    rng = np.random.default_rng(61)
    exact = base["grid"]                       # (the generator normalises in float32: every texel is float-representable)
    assert np.array_equal(exact.astype(np.float32).astype(np.float64), exact)
    inexact = base["grid"] * 0.7 + 1.0 / 3000.0
    assert not np.array_equal(inexact.astype(np.float32).astype(np.float64), inexact)
    for name, dtype, grid, mirror, tol in (("mirror", hip.EA_F64, exact, 1, 1e-12), ("fp64 image", hip.EA_F64, inexact, 0, 1e-12),
                                           ("fp32", hip.EA_F32, inexact, 0, 1e-5)):
        P = _problem(hip, base, dtype, 5000, rng, grid=grid)
        B = hip.Batch([P])
        try:
            for buf in (1, 0):   # raw-buffer and flat addressing of image and points
                B.set_tuning("buffer_loads", buf)
                q, t = _poses(rng, 5, 1)
                got = B.cost_poses(q, t)
                assert B.info("cost_form") == 1 and B.info("dt_f32") == mirror and B.info("buffer_loads") == buf, name
                _against_eval_poses(B, q, t, got, tol, (name, buf))
        finally:
            B.close(); P.close()


def test_losses_and_failed_functors(hip, base):
    rng = np.random.default_rng(67)
    for dtype, tol in ((hip.EA_F64, 1e-12), (hip.EA_F32, 1e-5)):
        for loss in ((hip.LOSS_TRIVIAL, 1.0), (hip.LOSS_CAUCHY, 0.7), (hip.LOSS_HUBER, 0.05)):
            P = _problem(hip, base, dtype, 3000, loss=loss)
            B = hip.Batch([P])
            try:
                q, t = _poses(rng, 4, 1, scale=2.0)
                _against_eval_poses(B, q, t, B.cost_poses(q, t), tol, (dtype, loss))
                assert B.info("cost_form") == 1
            finally:
                B.close(); P.close()
    P = _problem(hip, base, hip.EA_F64, 3000)
    B = hip.Batch([P])
    try:
        zmean = float(np.mean(base["xyz"][:3000, 2]))
        K = 6
        q = np.tile([1.0, 0, 0, 0], (K, 1, 1)); t = 0.002 * np.arange(K * 3, dtype=np.float64).reshape(K, 1, 3)
        t[3, 0] = [0.0, 0.0, -zmean]   # pose 3 = the second pose of the middle launch: points inside the z guard
        B.set_tuning("poses_per_launch", 2)
        got = B.cost_poses(q, t)
        ref = _against_eval_poses(B, q, t, got, 1e-12)
        assert got["n_invalid"][3, 0] > 0 and not got["n_invalid"][[0, 1, 2, 4, 5], 0].any()
        assert np.array_equal(got["n_invalid"], ref["n_invalid"])
    finally:
        B.close(); P.close()


@pytest.mark.parametrize("dtype_name,tol,tol_eval", DTYPES)
@pytest.mark.parametrize("kind", bb.KINDS)
def test_odd_image_border_band_and_off_the_image(hip, oracle, dtype_name, tol, tol_eval, kind):
    """37 x 53: the pitch is no multiple of anything convenient; most points sit in the border band, POSE_FAR swings most of the
    cloud off the image (every tap the same replicated texel)"""
    dtype = getattr(hip, dtype_name)
    pr = bb.band_problem(37, 53, 300, 7, kind)
    P = hip.Problem(*pr["K"], dtype=dtype)
    P.set_points(pr["xyz"]); P.set_dt_grid(pr["grid"]); P.set_loss(hip.LOSS_CAUCHY, 0.7)
    B = hip.Batch([P])
    O = oracle.OracleProblem(pr["grid"], *pr["K"], loss=hip.LOSS_CAUCHY, loss_a=0.7)
    try:
        poses = list(bb.POSES) + [bb.POSE_FAR]
        q = np.array([p[0] for p in poses])[:, None, :]; t = np.array([p[1] for p in poses])[:, None, :]
        got = B.cost_poses(q, t)
        assert B.info("cost_form") == 1
        _against_eval_poses(B, q, t, got, tol_eval, (kind,))
        for k in range(len(poses)):
            e = O.eval(pr["xyz"], q[k, 0], t[k, 0])
            d = abs(got["cost"][k, 0] - e["cost"])
            print(dtype_name, kind, k, "cost", got["cost"][k, 0], "oracle", e["cost"], "rel", d / abs(e["cost"]), "bad", got["n_invalid"][k, 0])
            assert d <= tol * abs(e["cost"]), k
            assert got["n_invalid"][k, 0] == e["n_invalid"], k
    finally:
        B.close(); P.close()


def test_normal_priors_across_three_launches(hip, base):
    rng = np.random.default_rng(53)
    P = _problem(hip, base, hip.EA_F64, 4097)
    S = _problem(hip, base, hip.EA_F64, 900, rng)
    P.set_normal_prior(0, 3.0 * np.eye(4), np.array([1.0, 0.002, -0.001, 0.003]))
    P.set_normal_prior(1, np.diag([5.0, 7.0, 9.0]), np.array([0.01, -0.02, 0.005]))
    B = hip.Batch([P, S])
    try:
        q, t = _poses(rng, 8, 2)
        B.set_tuning("poses_per_launch", 3)   # launches of 3, 3, 2 poses
        got = B.cost_poses(q, t)
        assert B.info("cost_form") == 1
        _against_eval_poses(B, q, t, got, 1e-12)
        assert len({float(c) for c in got["cost"][:, 0]}) == 8   # (each result carries the prior at its own pose)
        assert np.array_equal(B.cost_resident_poses()["cost"], got["cost"])   # (the prior is not added twice)
    finally:
        B.close(); P.close(); S.close()


def test_fall_back_to_the_full_evaluation(hip, base):
    rng = np.random.default_rng(71)
    q, t = _poses(rng, 5, 1)

    def check(B, what):
        got = B.cost_poses(q, t)
        assert B.info("cost_form") == 0, what
        ref = B.eval_poses(q, t)
        assert _rel(got["cost"], ref["cost"]) <= 1e-13 and np.array_equal(got["n_invalid"], ref["n_invalid"]), what
        assert np.array_equal(B.cost_resident_poses()["cost"], got["cost"]), what

    P = _problem(hip, base, hip.EA_F64, 5000)
    T = _problem(hip, base, hip.EA_F64, 1500)
    B = hip.Batch([P])
    try:
        assert B.cost_poses(q, t) is not None and B.info("cost_form") == 1
        P.add_term(T)
        check(B, "two terms")
        P.clear_terms()
        P.set_distortion(0.01, -0.002, 0.0005, -0.0003, 0.0)
        check(B, "variant functor")
    finally:
        B.close(); P.close(); T.close()
    P = _problem(hip, base, hip.EA_F64, 5000)
    B = hip.Batch([P])
    try:
        B.set_tuning("threads", 1024)
        check(B, "threads 1024")
        B.set_tuning("threads", 256)
        B.set_tuning("cost_form", 0)
        check(B, "cost_form 0")
        B.set_tuning("cost_form", 1)
        assert B.cost_poses(q, t) is not None and B.info("cost_form") == 1
    finally:
        B.close(); P.close()
    F = _problem(hip, base, hip.EA_F32, 5000)
    B = hip.Batch([F])
    try:
        B.set_tuning("wide_accumulate", 1)
        check(B, "wide_accumulate")
    finally:
        B.close(); F.close()


def test_state_and_empty_batch(hip, base):
    P = _problem(hip, base, hip.EA_F64, 600)
    E = _problem(hip, base, hip.EA_F64, 0)
    B, Be = hip.Batch([P]), hip.Batch([E, E])
    try:
        with pytest.raises(hip.EAError) as ei:
            B.cost_resident_poses(fetch=False)    # nothing resident yet
        assert ei.value.code == hip.EA_ERR_STATE
        q, t = _poses(np.random.default_rng(3), 4, 2)
        B.cost_poses(q[:, :1], t[:, :1])
        P.set_loss(hip.LOSS_HUBER, 0.2)           # the problem changed: resident poses are gone
        with pytest.raises(hip.EAError) as ei:
            B.cost_resident_poses()
        assert ei.value.code == hip.EA_ERR_STATE
        Bf = hip.Batch([P, P])                     # (dirty the pinned result block a batch of the same size gets next)
        Bf.eval_poses(q, t); Bf.close()
        got = Be.cost_poses(q, t)                  # not a single point: K x count zeros, no evaluation launch
        assert Be.info("cost_form") == 1 and not got["cost"].any() and not got["n_invalid"].any()
    finally:
        B.close(); Be.close(); P.close(); E.close()


def _summary_same(a, b):
    return (a["num_iterations"] == b["num_iterations"] and a["why"] == b["why"] and a["termination"] == b["termination"] and
            a["initial_cost"] == b["initial_cost"] and a["final_cost"] == b["final_cost"] and np.array_equal(a["it_cost"], b["it_cost"]))


def _rank(cost, bad, M):
    """the rule restated: eligible (finite cost, no failed functor) by (cost, index), then the ineligible by index"""
    K, n = cost.shape
    out = np.zeros((M, n), dtype=np.int64)
    for i in range(n):
        inel = ~(np.isfinite(cost[:, i]) & (bad[:, i] == 0))
        key = np.where(inel, 0.0, cost[:, i])
        order = np.lexsort((np.arange(K), key, inel))   # (last key first: ineligible, then cost, then index; lexsort is stable)
        out[:, i] = order[:M]
    return out


def test_search_ranks_then_solves_the_picked_starts(hip, oracle, base):
    other = synth.make_problem(120, 160, 3000, 40, 2, 130.0, 130.0, 79.5, 59.5,
                               planted_q=synth.quat_from_axis_angle([-2, 1, 0.5], np.deg2rad(0.8)),
                               planted_t=(-0.008, 0.012, 0.01), normalize=True)
    clouds = [base["xyz"][:2500], other["xyz"]]
    probs = [_problem(hip, base, hip.EA_F64, 2500), _problem(hip, other, hip.EA_F64, 3000)]
    B = hip.Batch(probs)
    try:
        K, M = 27, 4
        q = np.zeros((K, 2, 4)); t = np.zeros((K, 2, 3))
        for i, pr in enumerate((base, other)):
            q0 = synth.quat_plus(pr["q_true"], [0.004, -0.003, 0.002])
            t0 = np.asarray(pr["t_true"], dtype=np.float64) + [0.006, -0.004, 0.005]
            q[:, i], t[:, i] = synth.pose_lattice(q0, t0, [0.02, 0.0, 0.02, 0.0, 0.03, 0.0], [3, 1, 3, 1, 3, 1])
        for k, i in ((0, 0), (5, 0), (13, 0), (2, 1)):      # a few candidates with the cloud's first point on the camera plane
            q[k, i] = [1.0, 0, 0, 0]; t[k, i] = [0.0, 0.0, -clouds[i][0, 2]]
        costs = B.cost_poses(q, t)
        assert B.info("cost_form") == 1
        assert (costs["n_invalid"][[0, 5, 13], 0] > 0).all() and costs["n_invalid"][2, 1] > 0
        assert int((costs["n_invalid"] > 0).sum()) == 4
        qo, to, picked, s, best = B.search_starts(q, t, M)
        assert np.array_equal(picked, _rank(costs["cost"], costs["n_invalid"], M))
        assert not set(picked[:, 0]) & {0, 5, 13} and 2 not in picked[:, 1]
        # the K candidates are the resident poses now
        assert np.array_equal(B.cost_resident_poses()["cost"], costs["cost"])
        qp = np.stack([q[picked[:, i], i] for i in range(2)], axis=1); tp = np.stack([t[picked[:, i], i] for i in range(2)], axis=1)
        q1, t1, s1, best1 = B.solve_starts(qp, tp)
        assert np.array_equal(qo, q1) and np.array_equal(to, t1) and np.array_equal(best, best1)
        for m in range(M):
            for i in range(2):
                assert _summary_same(s[m][i], s1[m][i]), (m, i)
                assert s[m][i]["initial_cost"] == costs["cost"][picked[m, i], i] or \
                    abs(s[m][i]["initial_cost"] - costs["cost"][picked[m, i], i]) <= 1e-12 * costs["cost"][picked[m, i], i]
        # the best start lands on the oracle's solve from that start (the bars of test_gpu_solve_starts.py)
        for i, pr in enumerate((base, other)):
            O = oracle.OracleProblem(pr["grid"], *pr["K"], loss=hip.LOSS_CAUCHY, loss_a=0.7)
            b = int(best[i])
            assert 0 <= b < M and s[b][i]["termination"] == hip.CONVERGENCE
            q_or, t_or, so = O.solve(clouds[i], qp[b, i], tp[b, i])
            assert so["termination"] == 0
            ang, dt = synth.rotation_angle_between(qo[b, i], q_or), np.linalg.norm(to[b, i] - t_or)
            print("problem", i, "best rank", b, "candidate", picked[b, i], "angle", ang, "dt", dt)
            assert ang < 1e-7 and dt < 1e-7
        # without summaries and through the single-problem entry point: the same poses
        q2, t2, p2, none, best2 = B.search_starts(q, t, M, summaries=False)
        assert none is None and np.array_equal(q2, qo) and np.array_equal(t2, to) and np.array_equal(p2, picked) and np.array_equal(best2, best)
        qs, ts, ps, ss, bs = probs[0].search_starts(q[:, 0], t[:, 0], M)
        assert np.array_equal(ps, picked[:, 0]) and np.array_equal(qs, qo[:, 0]) and np.array_equal(ts, to[:, 0]) and bs == best[0]
        # M = K: every candidate is solved, the ineligible ones last (by index) and each ends on its failed first evaluation
        qa, ta, pa, sa, ba = B.search_starts(q, t, K)
        assert np.array_equal(pa, _rank(costs["cost"], costs["n_invalid"], K))
        assert sorted(pa[:, 0]) == list(range(K)) and list(pa[-3:, 0]) == [0, 5, 13] and pa[-1, 1] == 2
        for m in range(K):
            for i in range(2):
                failed = costs["n_invalid"][pa[m, i], i] > 0
                assert (sa[m][i]["why"] == "initial_eval_failed") == failed, (m, i)
        assert np.array_equal(qa[:M], qo) and np.array_equal(ta[:M], to)   # (a start does not depend on its company)
        for i in range(2):
            assert sa[ba[i]][i]["final_cost"] <= s[best[i]][i]["final_cost"]
        # M larger than the number of eligible candidates
        few = [0, 5, 13, 7, 20]
        qf, tf, pf, sf, bf = probs[0].search_starts(q[few, 0], t[few, 0], 4)
        assert pf[0] in (3, 4) and pf[1] in (3, 4) and list(pf[2:]) == [0, 1]
        assert [x["why"] == "initial_eval_failed" for x in sf] == [False, False, True, True] and bf in (0, 1)
        with pytest.raises(hip.EAError) as ei:
            B.search_starts(q, t, K + 1)
        assert ei.value.code == hip.EA_ERR_INVALID_ARG
    finally:
        B.close()
        for P in probs:
            P.close()
