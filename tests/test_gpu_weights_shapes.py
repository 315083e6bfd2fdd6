"""The weighted kernels (ea_eval_fused_w_kernel, ea_eval_poses_grid_w_kernel: {fp64, fp32} x {1, 2 points per lane} x
{raw-buffer, flat addressing}, 16 instantiations) and the weighted branch of the rows kernel in EVERY launch shape, against
tests/weights_ref.py (numpy sums over the oracle's raw rows), and failed residual blocks (|b_z| < 0.01: the functor returns
false) through the weighted and the plain kernels.

One hip.Batch([P]) per case, so that the tuning keys reach the launch; every case asserts through Batch.info that the launch
ran in the shape it asked for before it compares anything.  Clouds are the first n points of test_gpu_weights.cloud at the
pose QE, TE; n sits on both sides of the 256- and 512-point chunks and of the wavefront, with more than one workgroup.
Weights are weights_ref.real_weights (distinct per point, exact zeros).

Bounds (relative, on cost, JtJ and Jtr): 1e-11 (fp64) and 2e-4 (fp32), those of test_gpu_weights.py; rows 1e-12 absolute on r
and 1e-11 on J (fp64), 2e-5 / 2e-4 (fp32); the mixed batch 1e-10 / 2e-4 as test_gpu_variants.py holds variant functors to.

Failed blocks are planted by weights_ref.plant_failed at point 0, point n - 1 (the last lane of a partial chunk, whose
copies in the lanes past the end must not be counted) and in the k = 1 half of a two-point lane, with weights 2, 3 and 0:
n_invalid is the NUMBER of failed blocks (3), the sums leave them out, per-point outputs have NaN exactly there.  The
reference of these cases is evaluated at the points the device holds (Problem.get_points).

Every test prints one SHAPES-GPU line: the largest deviation it saw next to the bound (profiles/LOG.md has the figures of
an MI355X)."""
import itertools

import numpy as np
import pytest

from edge_alignment_amd import synth
import test_gpu_variants as tgv
import test_gpu_weights as tgw
import weights_ref as wr
from test_gpu_weights import cloud  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu
QE, TE, LOSSES = tgw.QE, tgw.TE, tgw.LOSSES
DTYPES = ("EA_F64", "EA_F32")
TOL = {"EA_F64": 1e-11, "EA_F32": 2e-4}
ROW_TOL = {"EA_F64": (1e-12, 1e-11), "EA_F32": (2e-5, 2e-4)}
# dtype, points per lane, raw-buffer (1) / flat (0) addressing, point order (0 = the caller's, 16 = tiles of 16 pixels)
SHAPES = list(itertools.product(DTYPES, (1, 2), (1, 0), (0, 16)))
NS = (1, 255, 257, 511, 512, 513, 1023, 1025)
NS_POSES = (257, 513, 1025)
FIELDS = ("cost", "JtJ", "Jtr", "n_invalid")


def _poses(tz_scale):
    """QE, TE and two perturbations (|dq| ~ 0.003, |dt| ~ 0.004 as in test_pose_batched_calls_on_a_weighted_batch);
    tz_scale < 1 keeps the planted |b_z| of the failed-block clouds inside the guard at every pose"""
    rng = np.random.default_rng(5)
    q, t = [QE], [TE]
    for _ in range(2):
        qq = QE + 0.003 * rng.standard_normal(4)
        d = 0.004 * rng.standard_normal(3)
        d[2] *= tz_scale
        q.append(qq / np.linalg.norm(qq)); t.append(TE + d)
    return np.stack(q), np.stack(t)


POSES, POSES_FAILED = _poses(1.0), _poses(0.1)


class Refs:
    """oracle evaluations (materialised raw rows), each computed once per module and left unchanged"""

    def __init__(self, oracle, cloud):
        self.oracle, self.cloud, self.cache = oracle, cloud, {}

    def points(self, n, failed=None, f32=False):
        """-> (cloud of n points, indices of the failed blocks).  failed: None, "three" (failed_indices) or "last" (n - 1)"""
        def make():
            xyz, idx = self.cloud["xyz"][:n], []
            if failed is not None:
                xyz, idx = wr.plant_failed(xyz, QE, TE, None if failed == "three" else [n - 1])
            xyz = np.array(xyz.astype(np.float32).astype(np.float64) if f32 else xyz)
            xyz.setflags(write=False)
            return xyz, idx
        return self._get(("points", n, failed, f32), make)

    def eval(self, n, loss, pose=0, failed=None, f32=False):
        """the oracle at pose `pose` of POSES (POSES_FAILED for the failed-block clouds)"""
        def make():
            q, t = POSES_FAILED if failed is not None else POSES
            O = self.oracle.OracleProblem(self.cloud["grid"], *self.cloud["K"], loss=loss[0], loss_a=loss[1])
            e = O.eval(self.points(n, failed, f32)[0], q[pose], t[pose], self.oracle.JAC_JET, materialize=True)
            for v in e.values():
                if isinstance(v, np.ndarray):
                    v.setflags(write=False)
            return e
        return self._get(("eval", n, tuple(loss), pose, failed, f32), make)

    def _get(self, key, make):
        if key not in self.cache:
            self.cache[key] = make()
        return self.cache[key]


@pytest.fixture(scope="module")
def refs(oracle, cloud):
    return Refs(oracle, cloud)


def _weights(n, idx=()):
    w = wr.real_weights(n, 100 + n)
    for i, v in zip(idx, wr.FAILED_W):
        w[i] = v
    return w


def _one(g, k=None):
    """one problem's evaluation out of Batch.eval (k None) or pose k of Batch.eval_poses / cost_poses"""
    pick = (lambda a: np.asarray(a)[0]) if k is None else (lambda a: np.asarray(a)[k, 0])
    return {f: pick(g[f]) for f in g if f in FIELDS}


def _dev(g, ref):
    cost, JtJ, Jtr = ref
    d = abs(float(g["cost"]) - cost) / max(abs(cost), 1e-300)
    if "JtJ" in g:
        d = max(d, wr.rel(g["JtJ"], JtJ), wr.rel(g["Jtr"], Jtr))
    return d


class Worst:
    def __init__(self, what, bound):
        self.what, self.bound, self.d, self.cases = what, bound, 0.0, 0

    def check(self, g, ref, where, bad=0):
        d = _dev(g, ref)
        self.d, self.cases = max(self.d, d), self.cases + 1
        assert int(g["n_invalid"]) == bad, (self.what, where, int(g["n_invalid"]), bad)
        assert d <= self.bound, (self.what, where, d, self.bound)

    def report(self):
        print("SHAPES-GPU %-60s cases %4d  largest deviation %.1e  bound %.0e" % (self.what, self.cases, self.d, self.bound))


def _same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in a if f in FIELDS)


def _ran_as_asked(B, ppt, buf, weighted=1):
    assert B.info("weighted") == weighted
    assert B.info("points_per_thread") == ppt and B.info("chunk") == 256 * ppt and B.info("threads") == 256
    assert B.info("buffer_loads") == buf


def _tile_order(xyz, K, tile):
    """the storage order of ea_problem_set_point_order(tile): stable by (tile row, tile column) of the identity-pose
    projection (Batch.eval_rows hands rows back in storage order) -> caller's index of stored point i"""
    if tile == 0:
        return np.arange(len(xyz))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = K[0] * xyz[:, 0] / xyz[:, 2] + K[2]
        v = K[1] * xyz[:, 1] / xyz[:, 2] + K[3]
    u, v = np.where(u >= 0, u, 0.0), np.where(v >= 0, v, 0.0)
    tx, ty = np.minimum(u / tile, 4095.0).astype(np.int64), np.minimum(v / tile, 4095.0).astype(np.int64)
    return np.argsort((ty << 12) | tx, kind="stable")


class OneProblem:
    """the first n cloud points (with planted failed blocks) in a Problem of its own Batch, tuned to (ppt, buf)"""

    def __init__(self, hip, refs, n, dtype_name, ppt=None, buf=None, order=0, failed=None, weighted=True, threads=None):
        self.dtype = getattr(hip, dtype_name)
        self.f32 = dtype_name == "EA_F32"
        c = refs.cloud
        xyz, self.idx = refs.points(n, failed)
        self.w = _weights(n, self.idx) if weighted else None
        self.P = tgw._problem(hip, xyz, c["grid"], c["K"], self.dtype, w=self.w, order=order)
        self.B = hip.Batch([self.P])
        assert self.P.point_order == order
        # the reference of the failed-block cases stands on the points the device holds
        assert np.array_equal(self.P.get_points(), refs.points(n, failed, self.f32)[0])
        for key, v in (("points_per_thread", ppt), ("buffer_loads", buf), ("threads", threads)):
            if v is not None:
                self.B.set_tuning(key, v)

    def close(self):
        self.B.close(); self.P.close()


# ---- part 2: every weighted instantiation against the reference -------------------------------------------------------

@pytest.mark.parametrize("dtype_name,ppt,buf,order", SHAPES)
def test_weighted_sums_in_every_launch_shape(hip, refs, dtype_name, ppt, buf, order):
    worst = Worst("ea_eval_fused_w_kernel %s ppt %d buf %d order %d" % (dtype_name, ppt, buf, order), TOL[dtype_name])
    for n in NS:
        c = OneProblem(hip, refs, n, dtype_name, ppt, buf, order)
        try:
            for loss in LOSSES:
                c.P.set_loss(*loss)
                g = c.B.eval(QE, TE)
                _ran_as_asked(c.B, ppt, buf)
                worst.check(_one(g), wr.weighted_sums(refs.eval(n, loss), c.w, *loss), (n, loss))
        finally:
            c.close()
    worst.report()


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_weighted_batch_clamps_the_launch_shape(hip, refs, dtype_name):
    """the weighted kernels exist at 256 lanes and one or two points per lane: a request beyond that runs 256 x 2, and gives
    the bits of asking for 256 x 2"""
    n = 1025
    c = OneProblem(hip, refs, n, dtype_name, 2, 1, threads=256)
    try:
        q, t = POSES
        want = c.B.eval(QE, TE)
        _ran_as_asked(c.B, 2, 1)
        want_k = c.B.eval_poses(q[:, None], t[:, None])
        Worst("clamp", TOL[dtype_name]).check(_one(want), wr.weighted_sums(refs.eval(n, LOSSES[1]), c.w), "direct")
        for ppt, nt in ((4, 256), (2, 1024), (4, 1024)):
            c.B.set_tuning("points_per_thread", ppt); c.B.set_tuning("threads", nt)
            got = c.B.eval(QE, TE)
            _ran_as_asked(c.B, 2, 1)
            assert _same(got, want), (ppt, nt)
            got_k = c.B.eval_poses(q[:, None], t[:, None])
            assert c.B.info("poses_points_per_thread") == 2 and c.B.info("poses_threads") == 256, (ppt, nt)
            assert _same(got_k, want_k), (ppt, nt)
    finally:
        c.close()


def _check_poses(c, refs, n, loss, ppt, buf, worst, failed=None, bad=0):
    """eval_poses and cost_poses at the three poses, each against the reference; every split over launches the same bits"""
    q, t = POSES_FAILED if failed is not None else POSES
    q, t = q[:, None], t[:, None]
    c.B.set_tuning("poses_per_launch", 0)
    e = c.B.eval_poses(q, t)
    assert c.B.info("poses_points_per_thread") == ppt and c.B.info("poses_threads") == 256
    assert c.B.info("buffer_loads") == buf and c.B.info("weighted") == 1
    k = c.B.cost_poses(q, t)
    assert c.B.info("cost_form") == 0   # (a weighted batch runs the full evaluation for a cost-only call)
    for p in range(len(q)):
        ev = refs.eval(n, loss, p, failed, c.f32 if failed is not None else False)
        assert wr.n_failed(ev) == bad   # (the workload: the planted blocks fail at every pose, no other does)
        ref = wr.weighted_sums(ev, c.w, *loss)
        worst.check(_one(e, p), ref, (n, loss, "eval_poses", p), bad)
        worst.check(_one(k, p), ref, (n, loss, "cost_poses", p), bad)
    for per in (1, 2):
        c.B.set_tuning("poses_per_launch", per)
        assert _same(c.B.eval_poses(q, t), e) and _same(c.B.cost_poses(q, t), k), (n, loss, "poses_per_launch", per)
    c.B.set_tuning("poses_per_launch", 0)


@pytest.mark.parametrize("dtype_name,ppt,buf,order", SHAPES)
def test_weighted_pose_batched_in_every_launch_shape(hip, refs, dtype_name, ppt, buf, order):
    worst = Worst("ea_eval_poses_grid_w_kernel %s ppt %d buf %d order %d" % (dtype_name, ppt, buf, order), TOL[dtype_name])
    for n in NS_POSES:
        c = OneProblem(hip, refs, n, dtype_name, ppt, buf, order)
        try:
            for loss in LOSSES:
                c.P.set_loss(*loss)
                _check_poses(c, refs, n, loss, ppt, buf, worst)
        finally:
            c.close()
    worst.report()


def _check_rows(c, refs, n, loss, order, dtype_name, e, bad_rows=()):
    """Batch.eval_rows in every store form and addressing form: corrected rows against sqrt(w rho') raw, raw rows against the
    unweighted reference, NaN exactly on the failed rows; layouts and store forms bit-identical among themselves
    -> (largest deviation of r, of J)"""
    rtol, jtol = ROW_TOL[dtype_name]
    perm = _tile_order(refs.points(n, "three" if len(bad_rows) else None)[0], refs.cloud["K"], order)
    w = c.P.get_weights()
    ok = np.ones(n, bool)
    ok[list(bad_rows)] = False
    assert np.array_equal(~ok, np.isnan(e["raw_r"]))
    with np.errstate(invalid="ignore"):
        sc = np.sqrt(w * wr.loss_pair(loss[0], loss[1], e["raw_r"] ** 2)[1])
    dr = dJ = 0.0
    for corrected in (True, False):
        want_r = (sc * e["raw_r"] if corrected else e["raw_r"])[perm]
        want_J = (sc[:, None] * e["raw_J"] if corrected else e["raw_J"])[perm]
        okp = ok[perm]
        for buf in (1, 0):
            c.B.set_tuning("buffer_loads", buf)
            first = None
            for staged, layout in itertools.product((1, 0), (0, 1)):
                c.B.set_tuning("rows_staged", staged)
                r, J, bad = c.B.eval_rows(QE, TE, corrected=corrected, layout=layout)
                J = J if layout == 0 else J.T
                where = (n, loss, corrected, buf, staged, layout)
                assert c.B.info("buffer_loads") == buf and c.B.info("weighted") == 1, where
                assert bad == len(bad_rows) and r.shape == (n,) and J.shape == (n, 6), where
                if first is None:
                    assert np.array_equal(np.isnan(r), ~okp) and np.array_equal(np.isnan(J).any(axis=1), ~okp), where
                    a, b = float(np.abs(r[okp] - want_r[okp]).max()), float(wr.rel(J[okp], want_J[okp]))
                    dr, dJ = max(dr, a), max(dJ, b)
                    assert a <= rtol and b <= jtol, (where, a, b)
                    first = (r.copy(), J.copy())
                assert np.array_equal(r, first[0], equal_nan=True) and np.array_equal(J, first[1], equal_nan=True), where
    c.B.set_tuning("buffer_loads", -1); c.B.set_tuning("rows_staged", -1)
    return dr, dJ


@pytest.mark.parametrize("order", [0, 16])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_weighted_rows_in_every_store_and_addressing_form(hip, refs, dtype_name, order):
    """for fp32 the reference takes what the device holds: Problem.get_points and Problem.get_weights"""
    n = 513
    c = OneProblem(hip, refs, n, dtype_name, order=order)
    try:
        dr = dJ = 0.0
        for loss in LOSSES:
            c.P.set_loss(*loss)
            O = refs.oracle.OracleProblem(refs.cloud["grid"], *refs.cloud["K"], loss=loss[0], loss_a=loss[1])
            e = O.eval(c.P.get_points(), QE, TE, refs.oracle.JAC_JET, materialize=True)
            a, b = _check_rows(c, refs, n, loss, order, dtype_name, e)
            dr, dJ = max(dr, a), max(dJ, b)
        print("SHAPES-GPU ea_eval_rows_kernel weighted %s order %d: largest deviation r %.1e (bound %.0e) J %.1e (bound %.0e)"
              % ((dtype_name, order, dr, ROW_TOL[dtype_name][0], dJ, ROW_TOL[dtype_name][1])))
    finally:
        c.close()


@pytest.fixture(scope="module")
def mixed(oracle):
    """four problems of different sizes and kinds (a list of terms each: cloud, grid, intrinsics, distortion, rig, weights)
    and the oracle's materialised rows of every term at the poses of the batch"""
    D, T12 = tgv.DIST, tgv.T12
    plain = synth.make_stereo_problem(120, 160, 1025, 600, 31, tgv.K1, tgv.K2, T12, tgv.Q, tgv.T)
    dist = synth.make_stereo_problem(120, 160, 513, 300, 32, tgv.K1, tgv.K2, T12, tgv.Q, tgv.T, distortion=D)

    def term(fam, n, K, d, t12, seed):
        return dict(xyz=fam["xyz"][:n], grid=fam["grid"], K=K, dist=d, T12=t12, w=None if seed is None else wr.real_weights(n, seed))

    problems = [[term(plain[0], 257, tgv.K1, None, None, None)],                 # 1. unweighted plain
                [term(plain[0], 1025, tgv.K1, None, None, 61)],                  # 2. weighted plain
                [term(dist[0], 513, tgv.K1, D, None, 62)],                       # 3. weighted + distortion (bits 0 + 2)
                [term(plain[1], 600, tgv.K2, None, T12, 63),                     # 4. weighted + second camera (bits 1 + 2)
                 term(dist[1], 300, tgv.K2, D, T12, 64)]]                        #    + a weighted distorted second-camera term (0 + 1 + 2)
    q = synth.quat_mul(synth.quat_from_axis_angle([0.2, -1, 0.4], 0.004), tgv.Q)
    t = tgv.T + 0.002
    for terms in problems:
        for tm in terms:
            O = oracle.OracleProblem(tm["grid"], *tm["K"], distortion=tm["dist"], T12=tm["T12"])
            tm["e"] = O.eval(tm["xyz"], q, t, oracle.JAC_JET, materialize=True)
    return problems, q, t


@pytest.mark.parametrize("reverse", [False, True], ids=["unweighted-head", "weighted-head"])
@pytest.mark.parametrize("dtype_name", DTYPES)
def test_mixed_batch_of_weighted_and_unweighted_variants(hip, mixed, dtype_name, reverse):
    """a head term without weights beside weighted ones (NULL weights inside the weighted kernel), the early point load of
    term 0 against the late one, workgroups past the end of the shorter problems, weights with the second camera and with all
    three variant bits; each problem against the sums over its terms' materialised rows and weights"""
    problems, q, t = mixed
    problems = problems[::-1] if reverse else problems
    dtype, tol = getattr(hip, dtype_name), {"EA_F64": 1e-10, "EA_F32": 2e-4}[dtype_name]
    keep, Ps = [], []
    for terms in problems:
        made = []
        for tm in terms:
            P = tgv._gpu(hip, tm, dtype, tm["K"], tm["dist"], tm["T12"])
            if tm["w"] is not None:
                P.set_weights(tm["w"])
            made.append(P)
        for T in made[1:]:
            made[0].add_term(T)
        keep += made; Ps.append(made[0])
    B = hip.Batch(Ps)
    worst = Worst("mixed batch %s reverse %d" % (dtype_name, reverse), tol)
    try:
        for ppt, buf in itertools.product((1, 2), (1, 0)):
            B.set_tuning("points_per_thread", ppt); B.set_tuning("buffer_loads", buf)
            g = B.eval(np.tile(q, (4, 1)), np.tile(t, (4, 1)))
            _ran_as_asked(B, ppt, buf, weighted=4)
            for i, terms in enumerate(problems):
                parts = [wr.weighted_sums(tm["e"], tm["w"] if tm["w"] is not None else np.ones(len(tm["xyz"]))) for tm in terms]
                ref = [sum(x) for x in zip(*parts)]
                worst.check({f: g[f][i] for f in FIELDS}, ref, (i, ppt, buf), sum(wr.n_failed(tm["e"]) for tm in terms))
        worst.report()
    finally:
        B.close()
        for P, terms in zip(Ps, problems):
            if len(terms) > 1:
                P.clear_terms()
        for P in keep:
            P.close()


# ---- part 3: failed blocks ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name,ppt,buf,order", SHAPES)
def test_failed_blocks_through_the_weighted_kernels(hip, refs, dtype_name, ppt, buf, order):
    worst = Worst("failed blocks, weighted %s ppt %d buf %d order %d" % (dtype_name, ppt, buf, order), TOL[dtype_name])
    f32 = dtype_name == "EA_F32"
    rtol, jtol = ROW_TOL[dtype_name]
    for n in NS_POSES:
        c = OneProblem(hip, refs, n, dtype_name, ppt, buf, order, failed="three")
        try:
            assert len(c.idx) == 3 and [c.w[i] for i in c.idx] == list(wr.FAILED_W)
            for loss in LOSSES:
                c.P.set_loss(*loss)
                e = refs.eval(n, loss, 0, "three", f32)
                assert wr.n_failed(e) == 3 and np.flatnonzero(np.isnan(e["raw_r"])).tolist() == c.idx
                g = c.B.eval(QE, TE)
                _ran_as_asked(c.B, ppt, buf)
                worst.check(_one(g), wr.weighted_sums(e, c.w, *loss), (n, loss), bad=3)   # 3, not the sum of the weights (5)
                _check_poses(c, refs, n, loss, ppt, buf, worst, failed="three", bad=3)
                # per-point outputs (caller's order): NaN exactly on the failed rows, the others as without failed blocks
                ok = ~np.isnan(e["raw_r"])
                with np.errstate(invalid="ignore"):
                    sc = np.sqrt(c.P.get_weights() * wr.loss_pair(loss[0], loss[1], e["raw_r"] ** 2)[1])
                r, J = c.P.eval_points(QE, TE, corrected=True)
                assert np.array_equal(np.isnan(r), ~ok) and np.array_equal(np.isnan(J).any(axis=1), ~ok), (n, loss)
                assert np.abs(r[ok] - (sc * e["raw_r"])[ok]).max() <= rtol and wr.rel(J[ok], (sc[:, None] * e["raw_J"])[ok]) <= jtol
            if ppt == 1 and buf == 1:   # (the rows kernel has no points-per-lane knob and _check_rows runs both addressing forms)
                c.P.set_loss(*LOSSES[1])
                _check_rows(c, refs, n, LOSSES[1], order, dtype_name, refs.eval(n, LOSSES[1], 0, "three", f32), bad_rows=c.idx)
        finally:
            c.close()
    worst.report()


# the launch shapes of the plain kernels: fp32 takes 1, 2 or 4 points per lane at either workgroup size; fp64 has no four
# points per lane and runs 1024 lanes at one point per lane only
PLAIN_SHAPES = list(itertools.product((1, 2, 4), (256, 1024)))
NOT_BUILT = {"EA_F64": {(2, 1024), (4, 256), (4, 1024)}, "EA_F32": set()}


def _plain_ref(e):
    return e["cost"], e["JtJ"], e["Jtr"]


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_failed_blocks_through_the_plain_kernels(hip, refs, dtype_name):
    """the same clouds without weights: Batch.eval in every launch shape the library builds, the pose-batched kernel (fp64:
    with and without the wave-exchange reduction), the cost-only kernel and Problem.cost, against the oracle's own sums
    and count.  A shape the library does not build is reported under another shape by Batch.info: skipped by name, and the
    names skipped are exactly the ones known not to exist."""
    worst = Worst("failed blocks, plain kernels %s" % dtype_name, TOL[dtype_name])
    f32 = dtype_name == "EA_F32"
    skipped = set()
    loss = LOSSES[1]
    q, t = POSES_FAILED
    for n in NS_POSES:
        refs_n = [refs.eval(n, loss, p, "three", f32) for p in range(3)]
        assert all(e["n_invalid"] == 3 == wr.n_failed(e) for e in refs_n)
        for ppt, nt in PLAIN_SHAPES:
            c = OneProblem(hip, refs, n, dtype_name, ppt, failed="three", weighted=False, threads=nt)
            try:
                g = c.B.eval(QE, TE)
                assert c.B.info("weighted") == 0
                if (c.B.info("points_per_thread"), c.B.info("threads")) != (ppt, nt):
                    skipped.add((ppt, nt))
                    continue
                assert c.B.info("chunk") == ppt * nt
                worst.check(_one(g), _plain_ref(refs_n[0]), (n, ppt, nt, "eval"), bad=3)
                cost, bad = c.P.cost(QE, TE)
                assert bad == 3 and abs(cost - refs_n[0]["cost"]) <= worst.bound * abs(refs_n[0]["cost"]), (n, ppt, nt)
                for xchg in ((1, 0) if not f32 else (0,)):
                    c.B.set_tuning("poses_wave_exchange", xchg)
                    e = c.B.eval_poses(q[:, None], t[:, None])
                    assert (c.B.info("poses_points_per_thread"), c.B.info("poses_threads")) == (ppt, nt), (n, ppt, nt)
                    if not f32 and nt == 256:
                        assert c.B.info("poses_wave_exchange") == xchg
                    k = c.B.cost_poses(q[:, None], t[:, None])
                    for p in range(3):
                        worst.check(_one(e, p), _plain_ref(refs_n[p]), (n, ppt, nt, xchg, "eval_poses", p), bad=3)
                        worst.check(_one(k, p), _plain_ref(refs_n[p]), (n, ppt, nt, xchg, "cost_poses", p), bad=3)
            finally:
                c.close()
    print("SHAPES-GPU plain shapes not built for %s (skipped): %s" % (dtype_name, sorted(skipped)))
    assert skipped == NOT_BUILT[dtype_name]
    worst.report()


@pytest.mark.parametrize("dtype_name", DTYPES)
def test_last_point_of_a_one_point_chunk_is_the_only_failed_block(hip, refs, dtype_name):
    """n = chunk + 1 and point n - 1 fails: the last workgroup has one valid lane, which fails, and chunk - 1 lanes past the
    end that carry a copy of it.  Counting the copies makes n_invalid 256, 512 or 1024 instead of 1."""
    worst = Worst("last point the only failed block %s" % dtype_name, TOL[dtype_name])
    f32 = dtype_name == "EA_F32"
    loss = LOSSES[1]
    q, t = POSES_FAILED
    cases = [(True, ppt, 256, buf) for ppt in (1, 2) for buf in (1, 0)]
    cases += [(False, ppt, nt, 1) for ppt, nt in PLAIN_SHAPES if ppt * nt <= 1024 and (ppt, nt) not in NOT_BUILT[dtype_name]]
    for weighted, ppt, nt, buf in cases:
        n = ppt * nt + 1
        refs_n = [refs.eval(n, loss, p, "last", f32) for p in range(3)]
        assert all(wr.n_failed(e) == 1 and np.isnan(e["raw_r"][n - 1]) for e in refs_n)
        c = OneProblem(hip, refs, n, dtype_name, ppt, buf, failed="last", weighted=weighted, threads=nt)
        try:
            w = c.w if weighted else np.ones(n)
            where = (weighted, ppt, nt, buf)
            g = c.B.eval(QE, TE)
            assert (c.B.info("points_per_thread"), c.B.info("threads"), c.B.info("chunk")) == (ppt, nt, n - 1), where
            assert c.B.info("weighted") == int(weighted) and c.B.info("buffer_loads") == buf, where
            worst.check(_one(g), wr.weighted_sums(refs_n[0], w, *loss), where + ("eval",), bad=1)
            e = c.B.eval_poses(q[:, None], t[:, None])
            assert (c.B.info("poses_points_per_thread"), c.B.info("poses_threads")) == (ppt, nt), where
            k = c.B.cost_poses(q[:, None], t[:, None])
            for p in range(3):
                ref = wr.weighted_sums(refs_n[p], w, *loss)
                worst.check(_one(e, p), ref, where + ("eval_poses", p), bad=1)
                worst.check(_one(k, p), ref, where + ("cost_poses", p), bad=1)
            cost, bad = c.P.cost(QE, TE)
            assert bad == 1, where
            r, J, bad = c.B.eval_rows(QE, TE, corrected=True)
            assert bad == 1 and np.flatnonzero(np.isnan(r)).tolist() == [n - 1], where
        finally:
            c.close()
    worst.report()
