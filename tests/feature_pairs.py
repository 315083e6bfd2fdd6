"""A pairwise covering array over the switches of a problem, with one reference composed from the references tests/ already
holds (test helper, no GPU, not a fixture).

A problem of this library is a product of independent switches (DIMENSIONS).  Which kernel a call runs is decided by host
predicates over them, and the per-feature test files let the features meet mostly by accident.  `cases()` is a deterministic,
seeded, generated array in which every pair of values of two different dimensions occurs in at least one case, except the
pairs include/ea_hip.h documents as refused or as having no effect (REFUSED_OR_IGNORED); those get one dedicated case each in
tests/test_gpu_feature_pairs.py.  A new problem feature adds its dimension here.

`reference(case, q, t)` is composed only of: border_band.functor / with_loss / sums (the long-double functor, the losses with
Ceres' corrector and per-point weights, the sums), the NormalPrior's contribution as tests/test_gpu_prior.py forms it, and
reduced_lm.solve (the trust-region loop over the free coordinates: the constant mask comes after the prior).  It works on the
inputs as a device holds them (`inputs`: what Problem.get_points / get_dt / get_weights return), or on the host's own statement
of them (`host_inputs`), which tests/test_gpu_feature_pairs.py holds to the same numbers.

Geometry: a 60 x 80 frame pair.  Term 0 has 321 points (one full 256-lane chunk and a partial one at one point per lane, one
partial chunk at two), term 1 has 130; every cloud is what get_aX makes of a synthetic frame (segments drawn white on black,
a depth image that is zero off the chosen edge pixels), so that the same cloud can be uploaded (set_points) or produced on
the device (set_ref_frame, which is what writes depth weights).  The distance transform is that of the pixels the cloud
projects to at the planted pose through the case's own functor.  A failed block is a point at depth 1 / 5000 m: the pose's
translation keeps |t_z| <= 0.005, so it sits inside the z guard at every pose a test uses.

Shards: SHARD_CUTS names the ways a case's points are cut over the ranks of a point-sharded solve, `shard_inputs` /
`shard_reference` are a rank's part of the inputs and the reference over it (no prior: that belongs to the reduced system), and
`sharded_runs()` lists what tests/test_gpu_feature_pairs_sharded.py runs."""
import functools
import itertools
import os
import sys

import numpy as np

from edge_alignment_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import border_band as bb  # noqa: E402
import reduced_lm  # noqa: E402
import weights_ref  # noqa: E402

DIMENSIONS = (
    ("dtype", ("f64", "f32")),
    ("loss", ("trivial", "cauchy", "huber", "auto")),
    ("weights", ("none", "real", "depth")),
    ("functor", ("plain", "Ex", "SecondCam", "SecondCamEx")),
    ("terms", ("one", "two")),
    ("flavour", ("default", "ros")),
    ("prior", ("none", "full", "t2")),
    ("held", ("none", "tz", "rot")),
    ("quat", ("unit", "scaled")),
    ("failed", ("none", "one")),
    ("shape", ("default", "ppt2", "nt1024")),
)
# (`shape` does not reach the point-sharded solves: they run on the problem's own batch, which has no tuning call, so the sharded
# forms of tests/test_gpu_feature_pairs_sharded.py run every case at the automatic shape)
NAMES = tuple(n for n, _ in DIMENSIONS)
VARIANT_FUNCTORS = ("Ex", "SecondCam", "SecondCamEx")

# Value pairs include/ea_hip.h documents as refused or as having no effect: kept out of the array, one dedicated case each
# (tests/test_gpu_feature_pairs.py::test_refused_or_ignored).  `pairs`: the pairs of dimension values the entry takes out of the
# array (none where the entry is about what a TERM may carry: the head of a two-term problem carries priors and masks, and that
# pair stays in the array).  `header`: the words of include/ea_hip.h that say so.
REFUSED_OR_IGNORED = (
    dict(name="term with a prior", kind="refused", pairs=(),
         header="ea_problem_set_normal_prior: EA_ERR_INVALID_ARG ... a problem that is a term of another (ea_problem_add_term, "
                "which in turn refuses a term that carries a prior)"),
    dict(name="term with a mask", kind="refused", pairs=(),
         header="constant parameters: Stored on the head problem only: EA_ERR_INVALID_ARG for a problem that is a term of "
                "another, and ea_problem_add_term refuses a term that carries a mask"),
    dict(name="terms of two dtypes", kind="refused", pairs=(),
         header="ea_problem_add_term: several residual families on ONE pose (terms must share device and dtype)"),
    dict(name="terms that disagree on rot_transposed", kind="refused", pairs=(),
         header="ea_problem_set_flavour / ea_problem_add_term: terms of one problem must agree on rot_transposed"),
    dict(name="auto-scaled loss with terms", kind="refused", pairs=((("loss", "auto"), ("terms", "two")),),
         header="ea_problem_set_loss_auto_scale: Refused (EA_ERR_INVALID_ARG) on a problem that has terms or is a term, and "
                "ea_problem_add_term refuses an auto-scaled problem on either side"),
    dict(name="threads = 1024 on the variant kernels", kind="ignored",
         pairs=tuple((("functor", f), ("shape", "nt1024")) for f in VARIANT_FUNCTORS)
         + tuple((("weights", w), ("shape", "nt1024")) for w in ("real", "depth"))
         # (the second term of this array's two-term problems always carries another functor, i.e. a variant one)
         + ((("terms", "two"), ("shape", "nt1024")),),
         header="per-point weights: A weighted problem runs the kernels of the residual variants (as a problem with distortion "
                "does); ea_batch_solve_starts: every other batch (variant functors, shared-pose terms, ..., \"threads\" = 1024): "
                "the variant kernels have the 256-thread shape only (ea_batch_get_info \"threads\" reports what is in effect)"),
    dict(name="z_guard = 0 has no failed block", kind="ignored", pairs=((("flavour", "ros"), ("failed", "one")),),
         header="ea_problem_set_flavour: ROS flavour = {z_guard 0, z_eps 0.001, rot_transposed 1}; n_invalid = blocks whose "
                "functor returned false (|b_z| < z_guard)"),
)

H, W = 60, 80                       # the image of scale_cases.lanes_base()
N_TERM = (321, 130)
K_TERM = ((65.0, 66.0, 39.5, 29.5), (64.0, 64.5, 40.5, 29.0))
# distortion and rig transform of tests/test_gpu_variants.py
DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)
T12 = synth.rigid_4x4(synth.quat_from_axis_angle([0.1, 1.0, 0.2], 0.04), [0.11, 0.004, -0.012])
OTHER_FUNCTOR = {"plain": "SecondCam", "Ex": "SecondCamEx", "SecondCam": "plain", "SecondCamEx": "Ex"}
PLANTED_Q = synth.quat_from_axis_angle([1, 2, 3], 0.01)
PLANTED_T = np.array([0.004, -0.002, 0.003])
Z_SCALING, Z_REF, DEPTH_POWER = 5000.0, 1.5, 2
DT_MAX = 4.0                        # texels in [0, 4]: residuals on both sides of Cauchy(0.3) and Huber(0.2)
LOSS = {"trivial": (bb.LOSS_TRIVIAL, 1.0), "cauchy": (bb.LOSS_CAUCHY, 0.3), "huber": (bb.LOSS_HUBER, 0.2), "auto": (bb.LOSS_CAUCHY, 0.3)}
AUTO_SCALE = (3.536, 0.5, 1e-6)     # Cauchy at 2.385 sigma, sigma = 1.4826 median |r| (include/ea_hip.h)
HELD = {"none": (0,) * 6, "tz": (0, 0, 0, 0, 0, 1), "rot": (1, 1, 1, 0, 0, 0)}
QUAT_SCALE = 1.2
K_POSES = 3
ARRAY_SEED = 20261
# the geometry / start-pose seed of every case of the array, in array order.  tests/test_feature_pairs_reference.py holds every
# solved case to the same iteration count, the same `why` and poses within 1e-9 between the float64 and the long-double
# evaluator; a case that does not is moved to the next seed here, never dropped.
DEFAULT_SEED = 1
SEEDS = (1,) * 22                   # (seed 1 is stable for every case of this array)


class Case(dict):
    __getattr__ = dict.__getitem__

    def name(self):
        return "#%d[%s]" % (self["index"], " ".join(str(self[n]) for n in NAMES))

    def with_(self, **kw):
        c = Case(self)
        c.update(kw)
        return c


# ---- the array -------------------------------------------------------------------------------------------------------------
def all_pairs():
    out = []
    for (na, va), (nb, vb) in itertools.combinations(DIMENSIONS, 2):
        out += [((na, a), (nb, b)) for a in va for b in vb]
    return out


def excluded_pairs():
    return {frozenset(p) for e in REFUSED_OR_IGNORED for p in e["pairs"]}


FAMILY = ("functor", "weights", "terms")   # the dimensions whose first values together mean: the plain kernels
PLAIN = ("family", "plain")


def family_pairs():
    """The kernel family is a switch of its own to the host (`any_variant`): a plain functor without weights and without a
    second term runs the plain kernels, the fused iteration, the lock-step multi-start, the cost kernel and the lane-per-pose
    evaluation; anything else runs the variant kernels.  Pairwise coverage alone leaves that triple to chance (the greedy array
    has it only where "threads" = 1024 forces it), so every value of every other dimension must also meet the plain family."""
    return [(PLAIN, (n, v)) for n, vs in DIMENSIONS if n not in FAMILY for v in vs]


def pairs_of(case):
    """the pairs a case covers (a partial assignment: those of the dimensions it has)"""
    items = [(n, case[n]) for n in NAMES if n in case]
    out = {frozenset(p) for p in itertools.combinations(items, 2)}
    if all(case.get(n) == dict(DIMENSIONS)[n][0] for n in FAMILY):
        out |= {frozenset((PLAIN, it)) for it in items if it[0] not in FAMILY}
    return out


def _allowed(assign, excl):
    items = list(assign.items())
    return not any(frozenset(p) in excl for p in itertools.combinations(items, 2))


@functools.lru_cache(maxsize=None)
def cases(seed=ARRAY_SEED, candidates=40):
    """The covering array: greedy, each new case the best of `candidates` seeded random completions of an uncovered pair.  The
    cases of the plain family come first, so that in a batch of three neighbours (tests/test_gpu_feature_pairs.py) plain
    problems sit beside plain ones in the middle of that block and beside variant ones at its ends."""
    rng = np.random.default_rng(seed)
    excl = excluded_pairs()
    uncovered_set = {p for p in map(frozenset, all_pairs() + family_pairs()) if p not in excl}
    values = dict(DIMENSIONS)
    out = []
    while uncovered_set:
        best, best_gain = None, -1
        todo = sorted(tuple(sorted(p)) for p in uncovered_set)
        for _ in range(candidates):
            first = todo[int(rng.integers(0, len(todo)))]
            assign = {n: v for n, v in first if n != "family"}
            if PLAIN in first:
                assign.update({n: values[n][0] for n in FAMILY})
            for n in [NAMES[i] for i in rng.permutation(len(NAMES))]:
                if n in assign:
                    continue
                scored = []
                for v in values[n]:
                    trial = dict(assign)
                    trial[n] = v
                    if not _allowed(trial, excl):
                        continue
                    scored.append((len(pairs_of(trial) & uncovered_set), float(rng.random()), v))
                assert scored, ("no allowed value", n, assign)
                assign[n] = max(scored)[2]
            gain = len(pairs_of(assign) & uncovered_set)
            if gain > best_gain:
                best, best_gain = assign, gain
        assert best_gain > 0
        uncovered_set -= pairs_of(best)
        out.append(best)
    out.sort(key=lambda c: is_variant(c))   # (stable: the plain family first, each block in the order it was generated)
    seeds = SEEDS if seed == ARRAY_SEED else (DEFAULT_SEED,) * len(out)
    assert len(seeds) == len(out), "SEEDS has %d entries, the array %d cases" % (len(seeds), len(out))
    return tuple(Case(c, index=i, seed=seeds[i]) for i, c in enumerate(out))


def solve_case(case):
    """the case as the solve forms run it to a numeric comparison: solves start from a unit quaternion, and a failed block ends
    every solve at its first evaluation (the GPU tests check that ending on the case itself, then solve this one)"""
    return case.with_(quat="unit", failed="none")


def first_values(**kw):
    """the case with every dimension at its first value but those given"""
    c = Case({n: v[0] for n, v in DIMENSIONS}, index=-1, seed=DEFAULT_SEED)
    c.update(kw)
    return c


# ---- what a case is made of ----------------------------------------------------------------------------------------------
def np_dtype(case):
    return np.float32 if case["dtype"] == "f32" else np.float64


def is_variant(case):
    """the case alone puts a batch on the variant kernels"""
    return case["functor"] != "plain" or case["weights"] != "none" or case["terms"] == "two"


def functor_args(functor, flavour):
    """keyword arguments of border_band.functor"""
    d = {}
    if functor in ("Ex", "SecondCamEx"):
        d["distortion"] = DIST
    if functor in ("SecondCam", "SecondCamEx"):
        d["T12"] = T12
    if flavour == "ros":
        d.update(z_guard=0.0, z_eps=0.001, rot_transposed=True)
    return d


def planted_q(flavour):
    """the functor of the ROS flavour warps by R(q)^T: the quaternion that aligns is the conjugate"""
    return PLANTED_Q * np.array([1.0, -1.0, -1.0, -1.0]) if flavour == "ros" else PLANTED_Q.copy()


def failed_index(case, n):
    """point 0, or the last point of the partial chunk (weights_ref.failed_indices), by the parity of the case's seed + index"""
    idx = weights_ref.failed_indices(n)
    return (idx[0], idx[-1])[(case["seed"] + max(case["index"], 0)) % 2]


@functools.lru_cache(maxsize=None)
def _frame(term, seed, failed):
    """(bgr (H, W, 3) uint8, depth (H, W) uint16, xyz (n, 3) = get_aX of them) of one term: n edge pixels keep a depth"""
    from oracle import preprocess_np as pp
    n, K = N_TERM[term], K_TERM[term]
    rng = np.random.default_rng(1000 * seed + term)
    p0, p1 = synth.random_segments(H, W, 14, rng, min_len=12.0)
    mask = synth.rasterize(H, W, p0, p1)
    bgr = np.ascontiguousarray(np.repeat((mask * 255).astype(np.uint8)[:, :, None], 3, axis=2))
    vv, uu = np.nonzero(pp.edge_strength(bgr) > 35)
    assert vv.size >= n, (vv.size, n)
    pick = np.sort(rng.choice(vv.size, n, replace=False))
    depth = np.zeros((H, W), np.uint16)
    depth[vv[pick], uu[pick]] = np.rint(rng.uniform(0.6, 3.0, n) * Z_SCALING).astype(np.uint16)
    if failed is not None:
        depth[vv[pick[failed]], uu[pick[failed]]] = 1
    aX, _ = pp.get_aX(bgr, depth, *K, z_scaling=Z_SCALING)
    xyz = np.ascontiguousarray(aX[:3].T)
    assert xyz.shape == (n, 3)
    return bgr, depth, xyz


@functools.lru_cache(maxsize=None)
def _image(term, seed, failed, functor, flavour):
    """the distance transform (H, W), float32 values in [0, DT_MAX], of the pixels the cloud projects to at the planted pose"""
    xyz = _frame(term, seed, failed)[2]
    p = bb.functor(np.zeros((H, W)), K_TERM[term], xyz, planted_q(flavour), PLANTED_T, np.float64, **functor_args(functor, flavour))
    ok = p["valid"] if failed is None else p["valid"] & (np.arange(len(xyz)) != failed)
    u, v = np.rint(p["u"][ok]).astype(int), np.rint(p["v"][ok]).astype(int)
    inside = (u >= 0) & (u < W) & (v >= 0) & (v < H)
    assert inside.sum() >= 0.6 * len(xyz), (term, seed, functor, flavour, int(inside.sum()))
    mask = np.zeros((H, W), bool)
    mask[v[inside], u[inside]] = True
    dt = synth.exact_edt(mask)
    return (dt * np.float32(DT_MAX / dt.max())).astype(np.float32).astype(np.float64)


def depth_weights(z, f32):
    """w = min(1, (z_ref / z)^2) from the stored z widened to double, rounded once to the problem dtype (include/ea_hip.h,
    ea_problem_set_depth_weighting; tests/test_gpu_depth_weights.py holds the device to it bit for bit)"""
    ratio = Z_REF / np.asarray(z, dtype=np.float64)
    v = ratio.copy()
    for _ in range(DEPTH_POWER - 1):
        v = v * ratio
    w = np.fmax(0.0, np.fmin(1.0, v))
    return w.astype(np.float32).astype(np.float64) if f32 else w


def term_specs(case):
    """what each term of the case is: dict(term, functor, weights)"""
    out = [dict(term=0, functor=case["functor"], weights=case["weights"])]
    if case["terms"] == "two":   # the second term takes another functor and its own weights
        out.append(dict(term=1, functor=OTHER_FUNCTOR[case["functor"]], weights="real" if case["weights"] != "none" else "none"))
    return out


def host_inputs(case):
    """per term: dict(bgr, depth, xyz, image, grid, K, weights, args, produced) with xyz and weights as a problem of the
    case's dtype holds them"""
    f32 = case["dtype"] == "f32"
    out = []
    for s in term_specs(case):
        k = s["term"]
        failed = failed_index(case, N_TERM[k]) if (case["failed"] == "one" and k == 0) else None
        bgr, depth, xyz = _frame(k, case["seed"], failed)
        image = _image(k, case["seed"], failed, s["functor"], case["flavour"])
        if f32:
            xyz = xyz.astype(np.float32).astype(np.float64)
        w = None
        if s["weights"] == "real":
            w = weights_ref.real_weights(len(xyz), 100 * case["seed"] + k)
            w = w.astype(np.float32).astype(np.float64) if f32 else w
        elif s["weights"] == "depth":
            w = depth_weights(xyz[:, 2], f32)
        out.append(dict(term=k, bgr=bgr, depth=depth, xyz=xyz, image=image, grid=np.ascontiguousarray(image.T), K=K_TERM[k],
                        weights=w, args=functor_args(s["functor"], case["flavour"]), functor=s["functor"],
                        produced=s["weights"] == "depth", failed=failed))
    return out


def prior(case):
    """dict(Aq, bq, At, bt) (None where the block has no prior)"""
    rng = np.random.default_rng(77)
    Aq, At3, At2 = rng.normal(size=(4, 4)) * 10.0, rng.normal(size=(3, 3)) * 10.0, rng.normal(size=(2, 3)) * 10.0
    bq = planted_q(case["flavour"]) + np.array([0.002, -0.001, 0.0015, 0.001])
    bt = PLANTED_T + np.array([0.003, -0.002, 0.001])
    if case["prior"] == "full":
        return dict(Aq=Aq, bq=bq, At=At3, bt=bt)
    if case["prior"] == "t2":
        return dict(Aq=None, bq=None, At=At2, bt=bt)
    return dict(Aq=None, bq=None, At=None, bt=None)


def poses(case, scaled=None):
    """K_POSES poses about 1 degree / 1 cm from the planted one (|t_z| stays at or below 0.005: a failed block fails at all of them)
    -> q (K, 4), t (K, 3).  scaled: None = as the case's `quat` says (the evaluation forms), False = unit (the solves)"""
    rng = np.random.default_rng(5000 + case["seed"])
    qp = planted_q(case["flavour"])
    q, t = np.zeros((K_POSES, 4)), np.zeros((K_POSES, 3))
    for k in range(K_POSES):
        q[k] = synth.quat_mul(synth.quat_from_axis_angle(rng.normal(size=3), np.deg2rad(rng.uniform(0.7, 1.2))), qp)
        d = rng.normal(size=2)
        t[k] = PLANTED_T + np.concatenate([0.01 * d / np.linalg.norm(d), [rng.uniform(-0.002, 0.002)]])
    if (case["quat"] == "scaled") if scaled is None else scaled:
        q = q * QUAT_SCALE
    return q, t


# ---- the reference ---------------------------------------------------------------------------------------------------------
def _plus_jacobian(q):
    return np.array([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]])


def prior_terms(q, t, Aq=None, bq=None, At=None, bt=None):
    """JtJ, Jtr, cost of the NormalPriors, as tests/test_gpu_prior.py forms them"""
    JtJ, Jtr, cost = np.zeros((6, 6)), np.zeros(6), 0.0
    if Aq is not None:
        Hq = Aq.T @ Aq
        d = np.asarray(q) - bq
        JtJ[:3, :3] += _plus_jacobian(q).T @ Hq @ _plus_jacobian(q)
        Jtr[:3] += _plus_jacobian(q).T @ Hq @ d
        cost += 0.5 * d @ Hq @ d
    if At is not None:
        Ht = At.T @ At
        d = np.asarray(t) - bt
        JtJ[3:, 3:] += Ht
        Jtr[3:] += Ht @ d
        cost += 0.5 * d @ Ht @ d
    return JtJ, Jtr, cost


_REF = {}


def reference(case, q, t, dtype=np.longdouble, inputs=None, loss=None, key=None):
    """cost, JtJ, Jtr, n_invalid of the whole problem (terms and prior included, the full 6 x 6 system: the mask belongs to
    the solve and the covariance) and the raw and corrected rows of every term in term order, in arithmetic `dtype`.
    inputs: per term what the device holds (default: host_inputs); loss: (kind, a) where it is not the case's own (an
    auto-scaled solve).  key: cache the result under (key, pose, dtype) -- references are pure functions of their inputs."""
    q, t = np.asarray(q, dtype=np.float64), np.asarray(t, dtype=np.float64)
    ck = None if key is None else (key, q.tobytes(), t.tobytes(), np.dtype(dtype).name, loss)
    if ck is not None and ck in _REF:
        return _REF[ck]
    inputs = host_inputs(case) if inputs is None else inputs
    kind, a = LOSS[case["loss"]] if loss is None else loss
    raw_r, raw_J, cor_r, cor_J, rho = [], [], [], [], []
    tot = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in inputs:
            raw = bb.functor(s["image"], s["K"], s["xyz"], q, t, dtype, **s["args"])
            cor = bb.with_loss(raw, kind, a, weights=s["weights"])
            sm = bb.sums(cor)
            tot = sm if tot is None else {k: tot[k] + sm[k] for k in sm}
            raw_r.append(raw["r"]); raw_J.append(raw["J"]); cor_r.append(cor["r"]); cor_J.append(cor["J"]); rho.append(cor["rho"])
    pJ, pr, pc = prior_terms(q, t, **prior(case))
    out = dict(cost=tot["cost"] + pc, JtJ=tot["JtJ"] + pJ, Jtr=tot["Jtr"] + pr, n_invalid=int(tot["n_invalid"]),
               cost_points=tot["cost"], JtJ_points=tot["JtJ"], Jtr_points=tot["Jtr"],
               raw_r=np.concatenate(raw_r), raw_J=np.concatenate(raw_J), r=np.concatenate(cor_r), J=np.concatenate(cor_J),
               rho=np.concatenate(rho), head_rows=len(raw_r[0]))
    if ck is not None:
        _REF[ck] = out
    return out


def auto_scale_a(case, q, t, inputs=None):
    """the scale an auto-scaled solve from (q, t) sets: max(a_min, factor * Q_prob |r|), Q the lower order statistic of the
    head's valid raw residuals (include/ea_hip.h: k = floor(prob * (m - 1)))"""
    s = (host_inputs(case) if inputs is None else inputs)[0]
    r = bb.functor(s["image"], s["K"], s["xyz"], q, t, np.longdouble, **s["args"])["r"]
    a = np.sort(np.abs(r[~np.isnan(r)]).astype(np.float64))
    factor, prob, a_min = AUTO_SCALE
    if len(a) == 0:
        return LOSS[case["loss"]][1]
    return max(a_min, factor * float(a[int(np.floor(prob * float(len(a) - 1)))]))


def solve_loss(case, q, t, inputs=None):
    """(kind, a) a solve from (q, t) runs with"""
    kind, a = LOSS[case["loss"]]
    return (kind, auto_scale_a(case, q, t, inputs)) if case["loss"] == "auto" else (kind, a)


def reference_solve(case, q0=None, t0=None, dtype=np.longdouble, inputs=None, quat_plus=synth.quat_plus, auto=True, key=None, **opts):
    """reduced_lm.solve over `reference` from start (q0, t0) (default: the case's first unit pose) -> q, t, summary.
    auto: an auto-scaled case estimates its scale at the start (ea_solve, ea_batch_solve); False: it runs with the case's own
    (ea_solve_starts)"""
    if q0 is None:
        qs, ts = poses(case, scaled=False)
        q0, t0 = qs[0], ts[0]
    inputs = host_inputs(case) if inputs is None else inputs
    loss = solve_loss(case, q0, t0, inputs) if auto else LOSS[case["loss"]]

    def evaluate(q, t):
        e = reference(case, q, t, dtype, inputs, loss=loss, key=key)
        return dict(cost=float(e["cost"]), JtJ=np.asarray(e["JtJ"], dtype=np.float64), Jtr=np.asarray(e["Jtr"], dtype=np.float64),
                    n_invalid=e["n_invalid"])

    q, t, s = reduced_lm.solve(evaluate, quat_plus, q0, t0, HELD[case["held"]], **opts)
    s["loss"] = loss
    return q, t, s


def reduced_pinv(JtJ, held):
    """the covariance of the free coordinates: the inverse of the reduced JtJ, zero rows and columns for the held ones"""
    free = [i for i in range(6) if not held[i]]
    out = np.zeros((6, 6))
    out[np.ix_(free, free)] = np.linalg.inv(np.asarray(JtJ, dtype=np.float64)[np.ix_(free, free)])
    return out


def tolerances(case, q, t, inputs=None, loss=None, key=None):
    """border_band.bounds of the whole problem at (q, t): the project's base bound of the case's kernels, or 4x the deviation
    of the plain rows in the kernels' precision from the long-double rows, whichever is larger (failed blocks left out)"""
    ty = np_dtype(case)
    base = (bb.VARIANT_BASE if (case["functor"] != "plain" or case["terms"] == "two") else
            bb.WEIGHTED_BASE if case["weights"] != "none" else bb.PROJECT)[ty]
    ref = reference(case, q, t, np.longdouble, inputs, loss, key)
    plain = reference(case, q, t, ty, inputs, loss, key)
    ok = ~np.isnan(ref["r"]) & ~np.isnan(plain["r"])
    image = np.concatenate([s["image"].ravel() for s in (host_inputs(case) if inputs is None else inputs)])
    return bb.bounds({k: ref[k][ok] for k in ("r", "J", "rho")}, {k: plain[k][ok] for k in ("r", "J", "rho")}, base, image)


# ---- shards of a case: the point-sharded solves ------------------------------------------------------------------------------
def _cut_even2(case, n_per_term):
    from edge_alignment_amd import dist as ead
    return [[(lambda s: (s.start, s.stop))(ead.shard_slice(n, r, 2)) for n in n_per_term] for r in range(2)]


def _cut_chunk2(case, n_per_term):
    """rank 0: exactly one full 256-lane chunk of the head and a second term of zero points; rank 1: the partial chunk and the
    whole second term"""
    return [[(0, 256)] + [(0, 0)] * (len(n_per_term) - 1), [(256, n_per_term[0])] + [(0, n) for n in n_per_term[1:]]]


def _cut_lone2(case, n_per_term):
    """rank 0: point 0 of the head and nothing else (where failed_index is 0, the failed block is its only point)"""
    return [[(0, 1)] + [(0, 0)] * (len(n_per_term) - 1), [(1, n_per_term[0])] + [(0, n) for n in n_per_term[1:]]]


def _cut_empty3(case, n_per_term):
    """ranks 0 and 2 split the head at 130 and the second term at 65; rank 1 holds nothing of any term"""
    at = (130, 65)
    return [[(0, at[k]) for k in range(len(n_per_term))], [(at[k], at[k]) for k in range(len(n_per_term))],
            [(at[k], n) for k, n in enumerate(n_per_term)]]


# name -> (world, fn(case, n_per_term) -> per rank, per term (begin, end))
SHARD_CUTS = {"even2": (2, _cut_even2), "chunk2": (2, _cut_chunk2), "lone2": (2, _cut_lone2), "empty3": (3, _cut_empty3)}


def shard_ranges(inputs, cut, case=None):
    """per rank, per term (begin, end) of `cut` over the terms of `inputs`; every point belongs to exactly one rank"""
    world, fn = SHARD_CUTS[cut]
    n = tuple(len(s["xyz"]) for s in inputs)
    out = fn(case, n)
    assert len(out) == world
    for k in range(len(n)):
        assert out[0][k][0] == 0 and out[-1][k][1] == n[k] and all(out[r][k][1] == out[r + 1][k][0] for r in range(world - 1)), (cut, k, out)
    return out


def shard_inputs(inputs, cut, rank, case=None):
    """what rank `rank` of `cut` holds of `inputs` (host_inputs, or what a device holds): its slice of the points and of the
    weights of every term, the whole image, K and args.  A produced term (weights == "depth") is sharded as points plus the
    weights the device produced (tests/test_gpu_feature_pairs.py holds those to depth_weights), so no shard is `produced`."""
    out = []
    for s, (b, e) in zip(inputs, shard_ranges(inputs, cut, case)[rank]):
        failed = s["failed"] if (s.get("failed") is not None and b <= s["failed"] < e) else None
        out.append(dict(s, xyz=np.ascontiguousarray(s["xyz"][b:e]), weights=None if s["weights"] is None else s["weights"][b:e].copy(),
                        produced=False, bgr=None, depth=None, failed=None if failed is None else failed - b))
    return out


def shard_reference(case, q, t, dtype=np.longdouble, inputs=None, cut="even2", rank=0, loss=None, key=None):
    """`reference` over the shard of rank `rank`, the prior left out (it belongs to the reduced system, once): cost_points,
    JtJ_points, Jtr_points, n_invalid and the rows; all zeros for a rank that holds nothing"""
    inputs = host_inputs(case) if inputs is None else inputs
    return reference(case.with_(prior="none"), q, t, dtype, shard_inputs(inputs, cut, rank, case), loss,
                     None if key is None else (key, "shard", cut, rank))


def shard_tolerances(case, q, t, inputs=None, cut="even2", rank=0, loss=None, key=None):
    """`tolerances` over the shard's inputs; a shard without a valid row has nothing that could round: its sums are exact zeros
    (bars of 0)"""
    inputs = host_inputs(case) if inputs is None else inputs
    sh = shard_inputs(inputs, cut, rank, case)
    ref = reference(case.with_(prior="none"), q, t, np.longdouble, sh, loss, None if key is None else (key, "shard", cut, rank))
    if not (~np.isnan(ref["r"].astype(np.float64))).any():
        return dict(r=0.0, J=0.0, sums=0.0)
    return tolerances(case.with_(prior="none"), q, t, sh, loss, None if key is None else (key, "shard", cut, rank))


def sharded_runs():
    """what the sharded forms run, in array order: every case as solve_case (kind "solve"), every fp32 case once more as its
    fp64 twin ("twin": the fp32 solve bars alone would not notice a prior counted twice or weights dropped on one shard), and
    every case with a failed block as itself ("failed": every rank ends at its first evaluation, the pose untouched)"""
    out = []
    for c in cases():
        out.append(("solve", solve_case(c)))
        if c["dtype"] == "f32":
            out.append(("twin", solve_case(c).with_(dtype="f64")))
        if c["failed"] == "one":
            out.append(("failed", c))
    return out


def sharded_system(case, q, t, cut, dtype=np.longdouble, inputs=None, loss=None, key=None, prior_per_rank=False, unit_weights_rank=None,
                   drop_term_rank=None, loss_of_rank=None):
    """The first exchange of a sharded solve at (q, t), restated: -> (local, reduced).  local: per rank dict(cost, JtJ, Jtr,
    n_invalid) as the rank sends it; reduced: their sum plus the prior, once.  The keyword arguments restate the mistakes the
    GPU tests must be able to see: the prior added once per rank (to what the rank sends), the weights of one rank's shard
    replaced by 1, the second term left out on one rank, the loss of one rank another one ((rank, (kind, a)))."""
    inputs = host_inputs(case) if inputs is None else inputs
    world = SHARD_CUTS[cut][0]
    pJ, pr, pc = prior_terms(q, t, **prior(case))
    local = []
    for r in range(world):
        sh = shard_inputs(inputs, cut, r, case)
        k = None if key is None else (key, "shard", cut, r)
        ls = loss
        if unit_weights_rank == r:
            sh, k = [dict(s, weights=None if s["weights"] is None else np.ones_like(s["weights"])) for s in sh], None
        if drop_term_rank == r:
            sh, k = sh[:1], None
        if loss_of_rank is not None and loss_of_rank[0] == r:
            ls = loss_of_rank[1]
        e = reference(case.with_(prior="none"), q, t, dtype, sh, ls, k)
        x = dict(cost=e["cost_points"], JtJ=e["JtJ_points"], Jtr=e["Jtr_points"], n_invalid=e["n_invalid"])
        if prior_per_rank:
            x = dict(cost=x["cost"] + pc, JtJ=x["JtJ"] + pJ, Jtr=x["Jtr"] + pr, n_invalid=x["n_invalid"])
        local.append(x)
    red = dict(cost=sum(x["cost"] for x in local), JtJ=sum(x["JtJ"] for x in local), Jtr=sum(x["Jtr"] for x in local),
               n_invalid=sum(x["n_invalid"] for x in local))
    if not prior_per_rank:
        red = dict(cost=red["cost"] + pc, JtJ=red["JtJ"] + pJ, Jtr=red["Jtr"] + pr, n_invalid=red["n_invalid"])
    return local, red
