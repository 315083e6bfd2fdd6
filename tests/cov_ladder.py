"""Helper of test_cov_ladder_reference.py (CPU) and test_gpu_covariance_ladder.py (device): a ladder of real 64-point problems
whose conditioning is set by one parameter, a 60-digit mpmath reference of what ea_cov.h computes from a 6x6 fp64 JtJ, the
bounds a backward-stable symmetric eigen-solver meets, Ceres' rank rule restated on the reference eigenvalues, and the
assertions both modules run -- one through the host builds of ea_cov.h, one through the device.  No tests in here.

The ladder: image 60x80, camera (65, 68, 39.5, 29.5), the DT grid of synth.make_problem(60, 80, 1025, 12, 3), trivial loss,
pose q = axis-angle([1, 2, 3], 0.01), t = (0.004, -0.002, 0.006); 64 points per rung, pixel = centre + 20 s U(-1, 1),
depth = 2 + s U(-1, 1), back-projected.  A point cloud that shrinks towards one pixel and one depth sees less and less of
the pose: kappa_2(JtJ) runs from below 1e3 (s = 1) to above 1e15 (s = 1e-4).

Bounds (errors are max-abs error over max-abs of the reference; eps = 2^-53; lambda_{m+1} := 0 for a system of size m):
  rank-k (pseudo-)inverse   bound_k = 32 eps (lambda_1 / lambda_k + lambda_1 / (lambda_k - lambda_{k+1}))
  eigenvalues               |computed - lambda_i| <= 32 eps lambda_1
-- own conditioning plus the gap to the dropped part.  Where bound_k >= 0.5 no accuracy is asserted, only the decision.
Rank rule: the computed ratio lambda_i / lambda_1 may be off by 64 eps in absolute terms (32 eps lambda_1 on either
eigenvalue), so a decision is asserted only where every ratio the rule consults is further than that from the threshold."""
import functools

import mpmath as mp
import numpy as np

from edge_alignment_amd import synth

H, W = 60, 80
K = (65.0, 68.0, 39.5, 29.5)
RUNGS = (1.0, 0.3, 0.1, 0.03, 0.01, 3e-3, 1e-3, 3e-4, 1e-4)
POINTS = 64
Q = synth.quat_from_axis_angle([1, 2, 3], 0.01)
T = np.array([0.004, -0.002, 0.006])
MASKS = ((1, 1, 1, 0, 0, 0), (0, 0, 0, 1, 1, 1), (0, 1, 0, 0, 1, 1), (1, 1, 1, 1, 1, 0))
MASK_RUNGS = (0, 3, 6)  # s = 1, 0.03, 1e-3
EPS = 2.0 ** -53
CONST = 32.0
RATIO_SLACK = 64.0 * EPS
LIFT_TOL = 512.0 * EPS  # see check_lift
SPARSE_QR, DENSE_SVD = 0, 1
DPS = 60


@functools.lru_cache(maxsize=None)
def grid():
    g = synth.make_problem(H, W, 1025, 12, 3, *K, normalize=True)["grid"]
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def rung_points(i):
    """the 64 points of rung i (frame A), fixed seed per rung"""
    s = RUNGS[i]
    rng = np.random.default_rng(7100 + i)
    u = K[2] + 20.0 * s * rng.uniform(-1, 1, POINTS)
    v = K[3] + 20.0 * s * rng.uniform(-1, 1, POINTS)
    z = 2.0 + s * rng.uniform(-1, 1, POINTS)
    X = np.stack([(u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z], axis=1)
    X.setflags(write=False)
    return X


def guard_translation(X, q=Q, t=T):
    """t with its z moved so that the pose carries X[0] onto z = 0, inside the functor's guard |z| < 0.01"""
    tb = np.array(t, dtype=np.float64)
    tb[2] = -(synth.quat_to_R(np.asarray(q) / np.linalg.norm(q)) @ X[0])[2]
    return tb


# ---- the reference ------------------------------------------------------------------------------------------------------

class Ref:
    """60-digit eigen-decomposition of the fp64 matrix A restricted to the free coordinates (held[i] != 0: coordinate i
    constant); lam descending (mp numbers), everything handed back as fp64 arrays embedded in 6x6 with zeros at the held
    coordinates."""

    def __init__(self, A, held=None):
        A = np.asarray(A, dtype=np.float64)
        assert A.shape == (6, 6)
        self.free = [i for i in range(6) if not (held is not None and held[i])]
        self.m = m = len(self.free)
        with mp.workdps(DPS):
            M = mp.matrix(m, m)
            for a, i in enumerate(self.free):
                for b, j in enumerate(self.free):
                    M[a, b] = mp.mpf(float(A[i, j]) if i <= j else float(A[j, i]))  # (the upper triangle is what is unpacked)
            E, V = mp.eigsy(M)
            order = sorted(range(m), key=lambda j: -E[j])
            self.lam = [E[j] for j in order]
            self.vec = [[V[a, j] for a in range(m)] for j in order]
        self.lam_f = np.array([float(x) for x in self.lam])

    @property
    def kappa(self):
        return float(self.lam[0] / abs(self.lam[-1]))

    def rho(self, i):
        """lambda_{i+1} / lambda_1 (0-based i), 0 past the end"""
        with mp.workdps(DPS):
            return self.lam[i] / self.lam[0] if i < self.m else mp.mpf(0)

    def pinv(self, k):
        out = np.zeros((6, 6))
        with mp.workdps(DPS):
            for a, i in enumerate(self.free):
                for b, j in enumerate(self.free):
                    out[i, j] = float(sum(self.vec[n][a] * self.vec[n][b] / self.lam[n] for n in range(k)))
        return out

    def bound_over_const(self, k):
        """bound_k / 32, float (inf where lambda_k or the gap is not positive)"""
        with mp.workdps(DPS):
            lk = self.lam[k - 1]
            gap = lk - (self.lam[k] if k < self.m else 0)
            if not (lk > 0 and gap > 0):
                return float("inf")
            return float(EPS * (self.lam[0] / lk + self.lam[0] / gap))

    def bound(self, k):
        return CONST * self.bound_over_const(k)


_REFS = {}


def ref_of(A, held=None):
    """Ref(A, held), computed once per matrix (bytes) and mask"""
    A = np.ascontiguousarray(A, dtype=np.float64)
    key = (A.tobytes(), tuple(int(bool(h)) for h in held) if held is not None else None)
    if key not in _REFS:
        _REFS[key] = Ref(A, held)
    return _REFS[key]


def expected_rank(ref, algorithm, min_rcn, nsr):
    """cov_rank restated on the reference eigenvalues: the rank kept, -1 for "not computed", None where a ratio the rule
    consults lies within RATIO_SLACK of min_rcn (no decision is asserted there)"""
    nsr = 0 if algorithm == SPARSE_QR else nsr
    max_rank = ref.m if nsr < 0 else ref.m - nsr
    if max_rank <= 0:
        return 0
    if not ref.lam[0] > 0:
        return 0 if nsr < 0 else -1
    rank = 0
    with mp.workdps(DPS):
        for i in range(max_rank):
            rho = ref.lam[i] / ref.lam[0]
            if i > 0 and abs(rho - mp.mpf(min_rcn)) <= RATIO_SLACK:  # (i = 0: the computed ratio is exactly 1)
                return None
            if not rho >= min_rcn:
                return rank if nsr < 0 else -1
            rank += 1
    return rank


# ---- what was measured ---------------------------------------------------------------------------------------------------

class Worst:
    """the worst ratios of a module: `inverse` = full-rank error / (kappa eps), `truncated` = rank-k error (k = m included) /
    (bound_k / 32), `eigenvalues` = max |computed - lambda_i| / (eps lambda_1)"""

    def __init__(self):
        self.inverse = self.truncated = self.eigenvalues = 0.0
        self.checked = 0

    def line(self, who):
        return ("%s worst ratios over %d results: inverse %.3g of kappa*2^-53, truncated inverse %.3g (bound: 32), "
                "eigenvalues %.3g (bound: 32)" % (who, self.checked, self.inverse, self.truncated, self.eigenvalues))


def rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def L_of(q):
    return np.array([[-q[1], -q[2], -q[3]], [q[0], q[3], -q[2]], [-q[3], q[0], q[1]], [q[2], -q[1], q[0]]])


def check_lift(c, q):
    """qq = L C_dd L^T, qt = L C_dt through L(q) built here from the returned tangent; tt has the bits of its block.
    L^T L = |q|^2 I, so the lift keeps the 2-norm: max|qq| >= |q|^2 max|C_dd| / 4.  Nine products with at most six roundings
    each, here and in the reference product: <= 108 eps |q|^2 max|C_dd|, 432 eps relative; LIFT_TOL = 512 eps covers both."""
    Lq, Tn = L_of(np.asarray(q, dtype=np.float64)), c["tangent"]
    assert rel(c["qq"], Lq @ Tn[:3, :3] @ Lq.T) <= LIFT_TOL
    assert rel(c["qt"], Lq @ Tn[:3, 3:]) <= LIFT_TOL
    assert c["tt"].tobytes() == np.ascontiguousarray(Tn[3:, 3:]).tobytes()


def check_eigenvalues(c, ref, worst, scale=1.0):
    lam = c["eigenvalues"]
    assert np.all(lam[ref.m:] == 0.0), lam  # unused slots
    assert np.all(np.diff(lam[:ref.m]) <= 0), lam  # descending
    err = np.abs(lam[:ref.m] - ref.lam_f).max() / (EPS * ref.lam_f[0]) if ref.m else 0.0
    worst.eigenvalues = max(worst.eigenvalues, err)
    assert err <= CONST * scale, (err, lam, ref.lam_f)


def check_result(c, A, q, worst, algorithm=SPARSE_QR, min_rcn=1e-14, nsr=0, held=None, scale=1.0, want=None):
    """One result c (covariance_to_dict) of the system A at quaternion q under the given options against the reference:
    eigenvalues, decision, (pseudo-)inverse, shape of the output, lift.  scale widens the accuracy bounds (1 unless the
    caller's A is itself a rounded copy of what was inverted).  want: the decision the caller expects (rank or -1), which
    then must also be what the restated rule gives.  Returns the decision (None: too close to call, nothing asserted on it)."""
    ref = ref_of(A, held)
    assert c["why"] in (0, 1), c["why"]
    check_eigenvalues(c, ref, worst, scale)
    exp = expected_rank(ref, algorithm, min_rcn, nsr)
    if want is not None:
        assert exp == want, (exp, want)
    if exp is None:
        return None
    if exp < 0:
        assert not c["ok"] and c["why"] == 1 and c["rank"] == 0, (c["ok"], c["why"], c["rank"])
        for k in ("tangent", "qq", "qt", "tt"):
            assert not c[k].any(), k
        return exp
    assert c["ok"] and c["why"] == 0 and c["rank"] == exp, (c["ok"], c["why"], c["rank"], exp)
    Tn = c["tangent"]
    assert Tn.tobytes() == np.ascontiguousarray(Tn.T).tobytes()  # symmetric exactly
    hm = np.array([bool(h) for h in held]) if held is not None else np.zeros(6, dtype=bool)
    assert not Tn[hm].any() and not Tn[:, hm].any()
    if exp > 0:
        boc = ref.bound_over_const(exp)
        if CONST * boc < 0.5:
            err = rel(Tn, ref.pinv(exp))
            worst.checked += 1
            worst.truncated = max(worst.truncated, err / boc)
            if exp == ref.m:
                worst.inverse = max(worst.inverse, err / (EPS * ref.kappa))
            assert err <= CONST * boc * scale, (err, CONST * boc, exp, ref.kappa)
    else:
        assert not Tn.any()
    check_lift(c, q)
    return exp


def same_bits(a, b):
    assert a["ok"] == b["ok"] and a["why"] == b["why"] and a["rank"] == b["rank"]
    for k in ("eigenvalues", "tangent", "qq", "qt", "tt"):
        assert a[k].tobytes() == b[k].tobytes(), k


# ---- the assertions of the ladder, on one system ---------------------------------------------------------------------------
# compute(**options) -> covariance_to_dict of the system under test (algorithm, min_rcn, nsr; held where a mask is meant)

def check_defaults(compute, A, q, worst):
    """SPARSE_QR and DENSE_SVD at the defaults and at min_rcn = 1e-12: the full-rank inverse within bound_6 and the
    eigenvalues within theirs where the rule keeps rank 6, "not computed" where it does not; -> {min_rcn: decision}"""
    out = {}
    for rcn in (1e-14, 1e-12):
        d = [check_result(compute(algorithm=alg, min_rcn=rcn, nsr=0), A, q, worst, alg, rcn, 0) for alg in (SPARSE_QR, DENSE_SVD)]
        assert d[0] == d[1]
        out[rcn] = d[0]
    return out


def check_caps(decisions):
    """decisions: check_defaults' result per rung.  At most one rung may be too close to call at 1e-14, none at 1e-12."""
    assert sum(d[1e-14] is None for d in decisions) <= 1, [d[1e-14] for d in decisions]
    assert all(d[1e-12] is not None for d in decisions), [d[1e-12] for d in decisions]


def check_truncation(compute, A, q, worst):
    """every rank k = 1..6 (a rung with kappa <= 1e8): automatic truncation between lambda_{k+1} and lambda_k, the forced
    form's bits, and one direction too few dropped"""
    ref = ref_of(A)
    assert ref.kappa <= 1e8
    for k in range(1, 7):
        with mp.workdps(DPS):
            mid = float(mp.sqrt(ref.rho(k) * ref.rho(k - 1)))
        auto = compute(algorithm=DENSE_SVD, min_rcn=mid, nsr=-1)
        assert check_result(auto, A, q, worst, DENSE_SVD, mid, -1, want=k) == k
        forced = compute(algorithm=DENSE_SVD, min_rcn=0.0, nsr=6 - k)
        assert check_result(forced, A, q, worst, DENSE_SVD, 0.0, 6 - k, want=k) == k
        same_bits(auto, forced)
        if k < 6:
            few = compute(algorithm=DENSE_SVD, min_rcn=mid, nsr=6 - k - 1)
            assert check_result(few, A, q, worst, DENSE_SVD, mid, 6 - k - 1, want=-1) == -1


def check_threshold(compute, A, q, worst):
    """min_rcn a thousandth below rho = lambda_6 / lambda_1 keeps rank 6, a thousandth above gives "not computed" """
    ref = ref_of(A)
    assert ref.kappa <= 1e8
    rho = float(ref.rho(5))
    for alg in (SPARSE_QR, DENSE_SVD):
        lo, hi = rho * (1 - 1e-3), rho * (1 + 1e-3)
        assert check_result(compute(algorithm=alg, min_rcn=lo, nsr=0), A, q, worst, alg, lo, 0, want=6) == 6
        assert check_result(compute(algorithm=alg, min_rcn=hi, nsr=0), A, q, worst, alg, hi, 0, want=-1) == -1


def check_masks(compute, A, q, worst):
    """the four held masks against the reduced reference; min_rcn = 1e-14 and automatic truncation, so that every rung
    has a result (the reduced system of a mask may be better or worse conditioned than the whole)"""
    for mask in MASKS:
        for alg, nsr in ((SPARSE_QR, 0), (DENSE_SVD, -1)):
            check_result(compute(algorithm=alg, min_rcn=1e-14, nsr=nsr, held=mask), A, q, worst, alg, 1e-14, nsr, held=mask)
