"""tests/feature_pairs.py without a GPU: the array covers every pair it has to, the composed reference reduces to the references
the suite already trusts (the oracle, weights_ref), and every case the GPU tests solve is a stable one -- the float64 and the
long-double evaluator walk the same iterations, so an iteration count that differs on the device is the device's."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import feature_pairs as fp  # noqa: E402
import weights_ref  # noqa: E402


def _rel(a, b):
    return float(np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)).max() / max(np.abs(np.asarray(b, dtype=np.float64)).max(), 1e-300))


def test_every_pair_is_covered_or_documented():
    cases = fp.cases()
    every = {frozenset(p) for p in fp.all_pairs()}
    excluded = fp.excluded_pairs()
    assert len(every) == 406 and excluded <= every
    every |= {frozenset(p) for p in fp.family_pairs()}   # and every value of the other dimensions meets the plain kernel family
    covered = set()
    for c in cases:
        mine = fp.pairs_of(c)
        assert not (mine & excluded), (c.name(), sorted(map(sorted, mine & excluded)))
        covered |= mine
    missing = every - excluded - covered
    assert not missing, sorted(map(sorted, missing))
    assert fp.cases() is cases and [dict(c) for c in fp.cases.__wrapped__(fp.ARRAY_SEED, 40)] == [dict(c) for c in cases]  # deterministic
    print("FEATURE-PAIRS %d cases, %d pairs: %d covered by comparing cases, %d refused or ignored" % (len(cases), len(every), len(every - excluded), len(excluded)))
    for c in cases:
        print("FEATURE-PAIRS case %s seed %d" % (c.name(), c["seed"]))
    for e in fp.REFUSED_OR_IGNORED:
        print("FEATURE-PAIRS %-8s %-42s %s" % (e["kind"], e["name"], "; ".join("%s=%s x %s=%s" % (a + b) for a, b in e["pairs"]) or "(a term's own setting)"))
        print("FEATURE-PAIRS          header: %s" % e["header"])
        assert e["kind"] in ("refused", "ignored") and e["header"]
    # every dimension's first value is the plain problem: `first_values` is the case the reductions below start from
    assert fp.is_variant(fp.first_values()) is False


def _oracle_problems(oracle, case):
    kind, a = fp.LOSS[case["loss"]]
    out = []
    for s in fp.host_inputs(case):
        g = s["args"]
        out.append(oracle.OracleProblem(s["grid"], *s["K"], loss=kind, loss_a=a, z_guard=g.get("z_guard", 0.01), z_eps=g.get("z_eps", 0.0),
                                        rot_transposed=g.get("rot_transposed", False), distortion=g.get("distortion"), T12=g.get("T12")))
    return out


ORACLE_KNOWS = [(d, v) for d, vs in fp.DIMENSIONS if d in ("dtype", "loss", "functor", "terms", "flavour", "quat", "failed")
                for v in vs if (d, v) != ("loss", "auto")]


@pytest.mark.parametrize("dim,value", ORACLE_KNOWS, ids=["%s-%s" % p for p in ORACLE_KNOWS])
def test_reference_reduces_to_the_oracle(oracle, dim, value):
    case = fp.first_values(**{dim: value})
    inputs = fp.host_inputs(case)
    Os = _oracle_problems(oracle, case)
    q, t = fp.poses(case)
    for k in range(fp.K_POSES):
        e = oracle.eval_terms(Os, [s["xyz"] for s in inputs], q[k], t[k], oracle.JAC_JET)
        ref = fp.reference(case, q[k], t[k])
        assert ref["n_invalid"] == e["n_invalid"] == (1 if (dim, value) == ("failed", "one") else 0), (k, ref["n_invalid"], e["n_invalid"])
        assert abs(float(ref["cost"]) - e["cost"]) <= 1e-12 * e["cost"], k
        assert _rel(ref["JtJ"], e["JtJ"]) <= 1e-12 and _rel(ref["Jtr"], e["Jtr"]) <= 1e-12, (k, _rel(ref["JtJ"], e["JtJ"]), _rel(ref["Jtr"], e["Jtr"]))
        m = Os[0].eval(inputs[0]["xyz"], q[k], t[k], oracle.JAC_JET, materialize=True)
        n = ref["head_rows"]
        ok = ~np.isnan(m["raw_r"])
        assert np.array_equal(ok, ~np.isnan(ref["raw_r"][:n].astype(np.float64)))
        assert np.abs(ref["raw_r"][:n][ok].astype(np.float64) - m["raw_r"][ok]).max() <= 1e-12
        assert _rel(ref["raw_J"][:n][ok], m["raw_J"][ok]) <= 1e-12 and _rel(ref["J"][:n][ok], m["J"][ok]) <= 1e-12
    if dim == "failed" and value == "one":
        assert inputs[0]["failed"] in (0, fp.N_TERM[0] - 1)


@pytest.mark.parametrize("weights", ["real", "depth"])
@pytest.mark.parametrize("loss", ["trivial", "cauchy", "huber"])
def test_reference_reduces_to_weighted_sums(oracle, weights, loss):
    case = fp.first_values(weights=weights, loss=loss)
    s = fp.host_inputs(case)[0]
    w = s["weights"]
    assert w is not None and ((w == 0.0).any() if weights == "real" else ((w == 1.0).any() and (w < 1.0).any()))
    O = _oracle_problems(oracle, case)[0]
    q, t = fp.poses(case)
    e = O.eval(s["xyz"], q[0], t[0], oracle.JAC_JET, materialize=True)
    cost, JtJ, Jtr = weights_ref.weighted_sums(e, w, *fp.LOSS[loss])
    ref = fp.reference(case, q[0], t[0])
    assert abs(float(ref["cost"]) - cost) <= 1e-12 * cost and _rel(ref["JtJ"], JtJ) <= 1e-12 and _rel(ref["Jtr"], Jtr) <= 1e-12


def test_prior_and_mask_enter_as_documented():
    """the prior adds to the full system; the mask is the solve's and the covariance's (held coordinates do not move)"""
    base = fp.first_values(loss="cauchy")
    q, t = fp.poses(base)
    e0 = fp.reference(base, q[0], t[0])
    for prior in ("full", "t2"):
        case = base.with_(prior=prior, held="tz")
        e1 = fp.reference(case, q[0], t[0])
        J, r, c = fp.prior_terms(q[0], t[0], **fp.prior(case))
        assert c > 0 and np.linalg.matrix_rank(J) == (6 if prior == "full" else 2)
        assert _rel(e1["JtJ"], np.asarray(e0["JtJ"], dtype=np.float64) + J) <= 1e-15 and abs(float(e1["cost"] - e0["cost"]) - c) <= 1e-12 * c
        qs, ts, s = fp.reference_solve(case, dtype=np.float64)
        assert ts[2] == t[0][2] and s["num_iterations"] >= 2
        C = fp.reduced_pinv(e1["JtJ"], fp.HELD["tz"])
        assert not C[5].any() and not C[:, 5].any() and _rel(C[:5, :5] @ np.asarray(e1["JtJ"], dtype=np.float64)[:5, :5], np.eye(5)) <= 1e-9


def solved_variants(case):
    """the solves the GPU tests run on a case: (auto-scale estimated, start index).  Every start runs with the problem's own loss
    (solve_starts); the first start also as ea_solve / ea_batch_solve run it, which differs for an auto-scaled loss only"""
    return [(False, k) for k in range(fp.K_POSES)] + ([(True, 0)] if case["loss"] == "auto" else [])


@pytest.mark.parametrize("index", range(len(fp.cases())))
def test_solved_cases_are_stable(index):
    case = fp.solve_case(fp.cases()[index])
    q0, t0 = fp.poses(case, scaled=False)
    for auto, k in solved_variants(case):
        a = fp.reference_solve(case, q0[k], t0[k], np.float64, auto=auto)
        b = fp.reference_solve(case, q0[k], t0[k], np.longdouble, auto=auto, key=("host", index))
        assert a[2]["num_iterations"] == b[2]["num_iterations"] and a[2]["why"] == b[2]["why"], (case.name(), k, auto, a[2]["num_iterations"], b[2]["num_iterations"], a[2]["why"], b[2]["why"])
        assert np.abs(a[0] - b[0]).max() <= 1e-9 and np.abs(a[1] - b[1]).max() <= 1e-9, (case.name(), k, auto)
        assert b[2]["termination"] != 2 and b[2]["num_iterations"] >= 2, (case.name(), k, b[2]["why"])   # a solve, not an ending at the start
        held = fp.HELD[case["held"]]
        assert all(b[1][i] == t0[k][i] for i in range(3) if held[3 + i])
