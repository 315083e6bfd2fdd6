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


# ---- shards of a case (the point-sharded solves: tests/test_gpu_feature_pairs_sharded.py) ------------------------------------
RUNS = fp.sharded_runs()
RUN_IDS = ["%s-%d" % (kind, c["index"]) for kind, c in RUNS]
CUTS = tuple(fp.SHARD_CUTS)


def _start(case):
    q0, t0 = fp.poses(case, scaled=False)
    return q0[0], t0[0]


def _ldrel(a, b):
    a, b = np.asarray(a, dtype=np.longdouble), np.asarray(b, dtype=np.longdouble)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), np.longdouble(1e-300)))


@pytest.mark.parametrize("kind,case", RUNS, ids=RUN_IDS)
def test_shard_references_add_up(kind, case):
    """fp.reference is additive over point shards: for every run and every cut the shard references, summed over the ranks in
    long double, are the whole reference's sums of the points to 1e-17 of the largest entry, and the failed block is seen by
    exactly one rank"""
    q, t = _start(case)
    whole = fp.reference(case, q, t)
    assert whole["n_invalid"] == (1 if kind == "failed" else 0)
    for cut in CUTS:
        world = fp.SHARD_CUTS[cut][0]
        parts = [fp.shard_reference(case, q, t, cut=cut, rank=r) for r in range(world)]
        assert sum(len(p["r"]) for p in parts) == len(whole["r"]), cut
        for k in ("cost_points", "JtJ_points", "Jtr_points"):
            assert parts[0][k].dtype == np.longdouble
            assert _ldrel(sum(p[k] for p in parts), whole[k]) <= 1e-17, (case.name(), cut, k, _ldrel(sum(p[k] for p in parts), whole[k]))
        assert sorted(p["n_invalid"] for p in parts) == [0] * (world - 1) + [whole["n_invalid"]], (case.name(), cut)
        for p in parts:   # the shard references carry no prior
            assert _ldrel(p["cost"], p["cost_points"]) == 0.0 and _ldrel(p["JtJ"], p["JtJ_points"]) == 0.0


def test_every_cut_has_its_edge():
    two = next(c for _, c in RUNS if c["terms"] == "two")
    inputs = fp.host_inputs(two)
    assert [len(s["xyz"]) for s in inputs] == list(fp.N_TERM)
    n = {cut: [[e - b for b, e in rank] for rank in fp.shard_ranges(inputs, cut, two)] for cut in CUTS}
    assert [len(v) for v in n.values()] == [fp.SHARD_CUTS[cut][0] for cut in CUTS] == [2, 2, 2, 3]
    assert n["even2"] == [[160, 65], [161, 65]]
    assert n["chunk2"] == [[256, 0], [65, 130]]          # one full 256-lane chunk beside a term of zero points; the partial chunk
    assert n["lone2"] == [[1, 0], [320, 130]]            # a one-point rank
    assert n["empty3"] == [[130, 65], [0, 0], [191, 65]]  # a rank that holds nothing of any term
    for cut in CUTS:   # the slices themselves, and a failed block goes with its point
        for kind, case in RUNS:
            ins = fp.host_inputs(case)
            sh = [fp.shard_inputs(ins, cut, r, case) for r in range(fp.SHARD_CUTS[cut][0])]
            for k, s in enumerate(ins):
                assert np.array_equal(np.concatenate([x[k]["xyz"] for x in sh]), s["xyz"])
                if s["weights"] is not None:
                    assert np.array_equal(np.concatenate([x[k]["weights"] for x in sh]), s["weights"])
                assert all(x[k]["image"] is s["image"] and x[k]["K"] == s["K"] and x[k]["args"] is s["args"] and not x[k]["produced"] for x in sh)
            if kind == "failed":
                assert [x[0]["failed"] is not None for x in sh].count(True) == 1
                if cut == "lone2" and ins[0]["failed"] == 0:
                    assert sh[0][0]["failed"] == 0 and len(sh[0][0]["xyz"]) == 1
    assert any(kind == "failed" and fp.host_inputs(c)[0]["failed"] == 0 for kind, c in RUNS)   # (the lone point does fail in some run)


TWINS = [c for kind, c in RUNS if kind == "twin"]


@pytest.mark.parametrize("case", TWINS, ids=["twin-%d" % c["index"] for c in TWINS])
def test_twins_are_stable(case):
    """the fp64 twin of an fp32 case holds other inputs (nothing rounded to fp32): it is held to test_solved_cases_are_stable's
    condition on its own, for the one solve the sharded forms run (the first start, the case's own loss)"""
    q0, t0 = _start(case)
    a = fp.reference_solve(case, q0, t0, np.float64, auto=False)
    b = fp.reference_solve(case, q0, t0, np.longdouble, auto=False, key=("twin", case["index"]))
    assert a[2]["num_iterations"] == b[2]["num_iterations"] and a[2]["why"] == b[2]["why"], (case.name(), a[2]["num_iterations"], b[2]["num_iterations"])
    assert np.abs(a[0] - b[0]).max() <= 1e-9 and np.abs(a[1] - b[1]).max() <= 1e-9, case.name()
    assert b[2]["termination"] != 2 and b[2]["num_iterations"] >= 2, (case.name(), b[2]["why"])


def _bars(case, q, t, cut=None, rank=None):
    """the bar of the GPU module's first-exchange comparison: fp64 1e-11 of the largest entry, fp32 fp.tolerances over the
    shard's (rank None: the whole problem's) inputs"""
    if case["dtype"] == "f64":
        return 1e-11
    return (fp.tolerances(case.with_(prior="none"), q, t) if rank is None else fp.shard_tolerances(case, q, t, cut=cut, rank=rank))["sums"]


def _sums_dev(got, ref):
    return fp.bb.dev_sums(got, ref)


def _pose_moves(case, cut, **mistake):
    """how far the fp64 final pose moves under the mistake, as a multiple of the fp64 solve bar (1e-7 rad / 1e-7 m)"""
    from edge_alignment_amd import synth
    q0, t0 = _start(case)

    def solve(**kw):
        def evaluate(q, t):
            e = fp.sharded_system(case, q, t, cut, np.float64, **kw)[1]
            return dict(cost=float(e["cost"]), JtJ=np.asarray(e["JtJ"], dtype=np.float64), Jtr=np.asarray(e["Jtr"], dtype=np.float64), n_invalid=e["n_invalid"])
        return fp.reduced_lm.solve(evaluate, synth.quat_plus, q0, t0, fp.HELD[case["held"]])
    a, b = solve(), solve(**mistake)
    return max(synth.rotation_angle_between(a[0], b[0]), float(np.linalg.norm(a[1] - b[1]))) / 1e-7


# which rank makes the mistake: one that holds weighted points / points of the second term, and more than the lone point
WEIGHTS_RANK = {"even2": 0, "chunk2": 0, "lone2": 1, "empty3": 0}
TERM_RANK = {"even2": 0, "chunk2": 1, "lone2": 1, "empty3": 2}
SEEN_RUNS = [(kind, c) for kind, c in RUNS if kind != "failed"]


@pytest.mark.parametrize("kind,case", SEEN_RUNS, ids=["%s-%d" % (k, c["index"]) for k, c in SEEN_RUNS])
def test_the_sharded_comparisons_can_tell(kind, case):
    """A condition on the inputs, not a measurement of a device: each mistake a sharded driver could make, restated in the
    reference, moves a sum of the first exchange (what the mistaken rank sends, or the reduced system) or the fp64 final pose
    by at least 10x the bar the GPU module holds it to -- on every cut, for every run the mistake applies to.  An fp32 run
    may rely on its fp64 twin for the final pose (the twin is in RUNS); its own sums must show the mistake or the twin's must."""
    q, t = _start(case)
    twin = case.with_(dtype="f64")
    mistakes = []
    if case["prior"] != "none":
        mistakes.append(("prior per rank", lambda cut: dict(prior_per_rank=True), lambda cut: 0))
    if case["weights"] != "none":
        mistakes.append(("weights dropped", lambda cut: dict(unit_weights_rank=WEIGHTS_RANK[cut]), lambda cut: WEIGHTS_RANK[cut]))
    if case["terms"] == "two":
        mistakes.append(("term dropped", lambda cut: dict(drop_term_rank=TERM_RANK[cut]), lambda cut: TERM_RANK[cut]))
    if case["loss"] == "auto":
        def reestimated(cut):
            r = WEIGHTS_RANK[cut]
            return dict(loss_of_rank=(r, (fp.LOSS["auto"][0], fp.auto_scale_a(case, q, t, fp.shard_inputs(fp.host_inputs(case), cut, r, case)))))
        mistakes.append(("loss re-estimated", reestimated, lambda cut: WEIGHTS_RANK[cut]))
    for name, kw, rank in mistakes:
        for cut in CUTS:
            seen = []
            # (a prior counted per rank would show in what a rank sends only if it were added before the exchange: it is held to
            # the stricter condition, the final pose)
            for c in ([] if name == "prior per rank" else [case] if case["dtype"] == "f64" else [case, twin]):
                good, bad = fp.sharded_system(c, q, t, cut), fp.sharded_system(c, q, t, cut, **kw(cut))
                r = rank(cut)
                seen.append(_sums_dev(bad[0][r], good[0][r]) / max(_bars(c, q, t, cut, r), 1e-300))
                # (the reduced sums as the exchange carries them: the points' -- the prior is the solve's)
                pj, pr_, pc = fp.prior_terms(q, t, **fp.prior(c))
                strip = lambda e, n: dict(cost=e["cost"] - n * pc, JtJ=e["JtJ"] - n * pj, Jtr=e["Jtr"] - n * pr_)
                if name != "prior per rank":
                    seen.append(_sums_dev(strip(bad[1], 1), strip(good[1], 1)) / _bars(c, q, t))
            if max(seen, default=0.0) < 10.0:
                seen.append(_pose_moves(twin, cut, **kw(cut)))
            print("FEATURE-PAIRS-SHARDS %-18s %-7s %s: %.3g x its bar" % (name, cut, case.name(), max(seen)))
            assert max(seen) >= 10.0, (case.name(), cut, name, seen)
