"""ea_cov_kernel (csrc/ea_capi.hip running csrc/ea_cov.h on one lane per problem) where the rest of the suite does not take
it: the conditioning ladder of tests/cov_ladder.py from kappa < 1e3 to > 1e15, every rank 1..6 under the automatic and the
forced rule, thresholds a thousandth either side of lambda_6 / lambda_1, held masks, a Cauchy loss on and off, fp32 problems,
and batches of 1, 63, 64, 65 and 130 problems -- more than one workgroup, a partly filled last one -- whose lanes mix full
rank, truncated, "not computed" (why 1), a failed functor (why 2) and no points (why 3) inside one wavefront, under the plain
and the SIDE (mask / prior) instantiation, called twice with a differently configured call in between.

The reference is 60-digit mpmath on the device's own fp64 JtJ (ea_eval / ea_batch_eval at the same pose); two witnesses hold
that it is the matrix the kernel inverted: the covariance's cost equals the evaluation's exactly, and the eigenvalues sum to
the trace within 32 * 2^-53 * lambda_1.  Bounds and decisions: tests/cov_ladder.py, the same as the host builds meet in
tests/test_cov_ladder_reference.py.

Worst ratios, host builds of ea_cov.h (with and without FMA contraction, 240 ladder matrices x 6 ranks): rank-k
(pseudo-)inverse 6.5 of the 32 allowed, full-rank inverse 0.07 of kappa * 2^-53.  MI355X, this module (1149 results, printed
at its end): rank-k (pseudo-)inverse 2.94 of 32, full-rank inverse 0.31 of kappa * 2^-53, eigenvalues 11.6 of 32 -- the
host builds on the same systems: 2.84, 0.31 and 17.4 (with contraction; 14.5 without).  The whole module runs in ~3 s."""
import ctypes as C

import numpy as np
import pytest

import cov_ladder as cl

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 130)
N_ROLES = 13  # nine rungs, failed functor, no points, [masked] rung, [prior] rung
ROLE_GUARD, ROLE_EMPTY, ROLE_MASK, ROLE_PRIOR = 9, 10, 11, 12
BATCH_MASK = cl.MASKS[2]
RUNG_IDS = ["s=%g" % s for s in cl.RUNGS]


@pytest.fixture(scope="module")
def worst():
    w = cl.Worst()
    yield w
    print("\n" + w.line("ea_cov_kernel"))


def _problem(hip, X, dtype=None, loss=None):
    P = hip.Problem(*cl.K, dtype=hip.EA_F64 if dtype is None else dtype)
    if X is not None:
        P.set_points(np.array(X))
    P.set_dt_grid(np.array(cl.grid()))
    P.set_loss(*(loss if loss is not None else (hip.LOSS_TRIVIAL, 1.0)))
    return P


@pytest.fixture(scope="module")
def rungs(hip):
    Ps = [_problem(hip, cl.rung_points(i)) for i in range(len(cl.RUNGS))]
    yield Ps
    for P in Ps:
        P.close()


def _computer(P, q, t, **fixed):
    def compute(algorithm=cl.SPARSE_QR, min_rcn=1e-14, nsr=0, held=None):
        if held is not None:
            P.set_constant_parameters(held)
        try:
            return P.covariance(q, t, algorithm=algorithm, min_reciprocal_condition_number=min_rcn, null_space_rank=nsr, **fixed)
        finally:
            if held is not None:
                P.set_constant_parameters(None)
    return compute


def _witness(c, cost, JtJ, exact_cost=True, held=None):
    """the covariance inverted the JtJ the evaluation returned (under a mask: its free coordinates' part)"""
    if exact_cost:
        assert c["cost"] == cost, (c["cost"], cost)
    lam1 = c["eigenvalues"][0]
    free = [i for i in range(6) if not (held is not None and held[i])]
    assert abs(c["eigenvalues"].sum() - np.trace(JtJ[np.ix_(free, free)])) <= cl.CONST * cl.EPS * lam1


def _system(P, q=cl.Q, t=cl.T):
    """(JtJ, compute) of a single problem, both witnesses checked"""
    g = P.eval(q, t)
    assert g["n_invalid"] == 0
    compute = _computer(P, q, t)
    c = compute(algorithm=cl.DENSE_SVD, min_rcn=0.0, nsr=-1)
    assert c["n_invalid"] == 0
    _witness(c, g["cost"], g["JtJ"])
    return g["JtJ"], compute


# ---- single problems, fp64 -------------------------------------------------------------------------------------------------

def test_ladder_spans_the_conditioning(rungs):
    kappas = [cl.ref_of(_system(P)[0]).kappa for P in rungs]
    print("\nkappa_2 per rung (device JtJ): " + ", ".join("%g: %.2g" % (s, k) for s, k in zip(cl.RUNGS, kappas)))
    assert kappas[0] <= 1e3 and kappas[-1] >= 1e15
    assert all(a < b for a, b in zip(kappas, kappas[1:])), kappas


def test_defaults_and_1e12_on_every_rung(rungs, worst):
    decisions = []
    for P in rungs:
        A, compute = _system(P)
        decisions.append(cl.check_defaults(compute, A, cl.Q, worst))
    cl.check_caps(decisions)
    assert decisions[0][1e-14] == 6 and decisions[-1][1e-14] == -1 and decisions[-1][1e-12] == -1


@pytest.mark.parametrize("i", range(len(cl.RUNGS)), ids=RUNG_IDS)
def test_truncation_at_every_rank(rungs, worst, i):
    A, compute = _system(rungs[i])
    if cl.ref_of(A).kappa > 1e8:
        return  # (the rungs above serve the decisions at the defaults only)
    cl.check_truncation(compute, A, cl.Q, worst)


@pytest.mark.parametrize("i", range(len(cl.RUNGS)), ids=RUNG_IDS)
def test_threshold_a_thousandth_either_side(rungs, worst, i):
    A, compute = _system(rungs[i])
    if cl.ref_of(A).kappa > 1e8:
        return
    cl.check_threshold(compute, A, cl.Q, worst)


@pytest.mark.parametrize("i", cl.MASK_RUNGS, ids=[RUNG_IDS[i] for i in cl.MASK_RUNGS])
def test_held_masks_against_the_reduced_reference(rungs, worst, i):
    A, compute = _system(rungs[i])
    cl.check_masks(compute, A, cl.Q, worst)
    assert rungs[i].get_constant_parameters() == [0] * 6


def test_non_unit_quaternion(rungs, worst):
    q = 1.2 * cl.Q
    for i in (0, 3):
        A, compute = _system(rungs[i], q, cl.T)
        assert cl.check_result(compute(), A, q, worst, want=6) == 6
        assert cl.check_result(compute(algorithm=cl.DENSE_SVD, min_rcn=0.0, nsr=2), A, q, worst, cl.DENSE_SVD, 0.0, 2, want=4) == 4


def test_cauchy_loss_applied_and_not(hip, worst):
    P = _problem(hip, cl.rung_points(3), loss=(hip.LOSS_CAUCHY, 0.7))
    g = P.eval(cl.Q, cl.T)
    on = _computer(P, cl.Q, cl.T, apply_loss_function=1)
    _witness(on(), g["cost"], g["JtJ"])
    cl.check_defaults(on, g["JtJ"], cl.Q, worst)
    cl.check_truncation(on, g["JtJ"], cl.Q, worst)
    # raw rows: the host's sum J^T J of the uncorrected rows -- a re-summed copy of what the device inverted, bounds x 4
    r, J = P.eval_points(cl.Q, cl.T, corrected=False)
    A0 = J.T @ J
    assert cl.rel(A0, g["JtJ"]) > 1e-3  # (the loss does change the system on this rung)
    off = _computer(P, cl.Q, cl.T, apply_loss_function=0)
    c = off()
    assert c["cost"] == pytest.approx(0.5 * np.sum(r * r), rel=1e-12)
    for alg, rcn, nsr in ((cl.SPARSE_QR, 1e-14, 0), (cl.DENSE_SVD, 0.0, 1), (cl.DENSE_SVD, 0.0, 3)):
        ref = cl.ref_of(A0)
        c = off(algorithm=alg, min_rcn=rcn, nsr=nsr)
        assert c["ok"] and c["rank"] == 6 - nsr
        k = c["rank"]
        assert cl.CONST * ref.bound_over_const(k) < 0.5
        assert cl.rel(c["tangent"], ref.pinv(k)) <= 4 * ref.bound(k)
        assert np.abs(c["eigenvalues"] - ref.lam_f).max() <= 4 * cl.CONST * cl.EPS * ref.lam_f[0]
        cl.check_lift(c, cl.Q)
    # the problem keeps its loss
    after = P.eval(cl.Q, cl.T)
    assert after["JtJ"].tobytes() == g["JtJ"].tobytes() and after["cost"] == g["cost"]
    P.close()


# ---- fp32 problems: the same kernel on the sums of the float evaluation -----------------------------------------------------

@pytest.mark.parametrize("i", (0, 1, 2), ids=RUNG_IDS[:3])
def test_fp32_problems(hip, worst, i):
    P = _problem(hip, cl.rung_points(i), dtype=hip.EA_F32)
    A, compute = _system(P)
    d = cl.check_defaults(compute, A, cl.Q, worst)
    assert d[1e-14] == 6 and d[1e-12] == 6
    cl.check_truncation(compute, A, cl.Q, worst)
    cl.check_threshold(compute, A, cl.Q, worst)
    P.close()


# ---- wide batches -----------------------------------------------------------------------------------------------------------

def _role_points(role):
    if role < len(cl.RUNGS):
        return cl.rung_points(role)
    return {ROLE_GUARD: cl.rung_points(0), ROLE_EMPTY: None, ROLE_MASK: cl.rung_points(3), ROLE_PRIOR: cl.rung_points(8)}[role]


@pytest.fixture(scope="module")
def pool(hip):
    """max(COUNTS) problems, lane i in role i % N_ROLES, each built once and shared by every batch"""
    Ps = [_problem(hip, _role_points(i % N_ROLES)) for i in range(max(COUNTS))]
    yield Ps
    for P in Ps:
        P.close()


def _raw_covariance(hip, B, q, t, **opts):
    """ea_batch_covariance -> the ctypes result array itself"""
    o = hip.covariance_options(**opts)
    out = (hip.Covariance * len(B))()
    dp = C.POINTER(C.c_double)
    rc = hip.load().ea_batch_covariance(B._h, q.ctypes.data_as(dp), t.ctypes.data_as(dp), C.byref(o), out)
    assert rc == hip.EA_OK, hip.load().ea_last_error().decode()
    return out


def _result_bytes(hip, out):
    """every byte of the result array but the four of padding between `rank` and `n_invalid`"""
    size = C.sizeof(hip.Covariance)
    assert hip.Covariance.rank.offset == 8 and hip.Covariance.n_invalid.offset == 16
    a = np.frombuffer(out, dtype=np.uint8).reshape(len(out), size)
    return np.delete(a, slice(12, 16), axis=1).tobytes()


def _check_lanes(hip, out, be, q, side, opts, worst):
    """every lane against the reference of its own batch JtJ, or its expected ok / why / rank; -> outcomes of lanes 0..63"""
    seen = set()
    for i in range(len(out)):
        c, role = hip.covariance_to_dict(out[i]), i % N_ROLES
        if role == ROLE_EMPTY:
            assert not c["ok"] and c["why"] == 3 and c["rank"] == 0, i
            what = "why3"
        elif role == ROLE_GUARD:
            assert not c["ok"] and c["why"] == 2 and c["rank"] == 0 and c["n_invalid"] > 0, i
            assert c["n_invalid"] == be["n_invalid"][i]
            assert not c["tangent"].any() and not c["qq"].any()
            what = "why2"
        else:
            held = BATCH_MASK if side and role == ROLE_MASK else None
            assert c["n_invalid"] == 0 and be["n_invalid"][i] == 0
            # (a prior's terms are added by the host for ea_batch_eval and by the kernel for the covariance: the same code in two builds)
            _witness(c, be["cost"][i], be["JtJ"][i], exact_cost=not (side and role == ROLE_PRIOR), held=held)
            want = 6 if side and role == ROLE_PRIOR else None
            d = cl.check_result(c, be["JtJ"][i], q[i], worst, held=held, want=want, **opts)
            what = "undecided" if d is None else "why1" if d < 0 else "full" if d == (6 if held is None else 6 - sum(held)) else "truncated"
        if i < 64:
            seen.add(what)
    return seen


@pytest.mark.parametrize("side", (False, True), ids=("plain", "side"))
def test_wide_batches(hip, pool, worst, side):
    n = max(COUNTS)
    q = np.tile(cl.Q, (n, 1))
    t = np.tile(cl.T, (n, 1))
    for i in range(ROLE_GUARD, n, N_ROLES):
        t[i] = cl.guard_translation(cl.rung_points(0))
    try:
        if side:
            for i in range(n):
                if i % N_ROLES == ROLE_MASK:
                    pool[i].set_constant_parameters(BATCH_MASK)
                if i % N_ROLES == ROLE_PRIOR:
                    pool[i].set_normal_prior(0, 10.0 * np.eye(4), cl.Q)
                    pool[i].set_normal_prior(1, 10.0 * np.eye(3), cl.T + 0.001)
        defaults = dict(algorithm=cl.SPARSE_QR, min_rcn=1e-14, nsr=0)
        auto = dict(algorithm=cl.DENSE_SVD, min_rcn=1e-14, nsr=-1)
        for count in COUNTS:
            B = hip.Batch(pool[:count])
            qc, tc = np.ascontiguousarray(q[:count]), np.ascontiguousarray(t[:count])
            be = B.eval(qc, tc)
            B.set_poses(np.stack([qc, qc]), np.stack([tc, tc + 1e-3]))
            res0 = B.eval_resident_poses()
            first = _raw_covariance(hip, B, qc, tc)
            between = _raw_covariance(hip, B, qc, tc, algorithm="dense_svd", null_space_rank=-1)
            second = _raw_covariance(hip, B, qc, tc)
            res1 = B.eval_resident_poses()
            assert _result_bytes(hip, first) == _result_bytes(hip, second), count
            for k in ("cost", "JtJ", "Jtr", "n_invalid"):
                assert res0[k].tobytes() == res1[k].tobytes(), (count, k)
            seen = _check_lanes(hip, first, be, qc, side, defaults, worst)
            seen_auto = _check_lanes(hip, between, be, qc, side, auto, worst)
            if count >= 63:  # one wavefront holds every outcome
                assert {"full", "why1", "why2", "why3"} <= seen, seen
                assert {"full", "truncated", "why2", "why3"} <= seen_auto, seen_auto
            again = _raw_covariance(hip, B, qc, tc, algorithm="dense_svd", null_space_rank=-1)
            assert _result_bytes(hip, again) == _result_bytes(hip, between), count
            B.close()
    finally:
        for P in pool:
            P.set_constant_parameters(None)
            P.clear_normal_prior(0)
            P.clear_normal_prior(1)
