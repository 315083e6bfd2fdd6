"""Every pair of problem features on every evaluation and solve form: the covering array of tests/feature_pairs.py run through
Problem.eval, Batch.eval, the per-point outputs, the pose-batched evaluations, the solves, multi-start and covariance, each
against the one composed reference (tests/feature_pairs.py), each with the kernel form ea_batch_get_info reports held to the one
include/ea_hip.h documents for the combination.  One test per form; a test loops over the whole array (a few dozen launches on
60 x 80 images and 321 + 130 points).

Bars (none is this module's own): fp64 rows 1e-12, fp64 sums 1e-11 of the largest entry; fp32 border_band.bounds (the project's
base bound or 4x the deviation of plain fp32 rows); fp64 solves equal iteration count and `why`, poses within 1e-7 rad / 1e-7 m
(tests/test_gpu_variants.py); fp32 solves 1e-4 rad / 1e-3 m; covariance 1e-8 against the reference's JtJ and 1e-12 (1e-10 with a
prior) against the device's own (tests/test_gpu_constant_parameters.py, tests/test_gpu_prior.py).  Every test prints its worst
deviation as a share of its bar (profiles/feature_pairs_deviations.txt keeps the table of one run)."""
import os
import sys

import numpy as np
import pytest

from edge_alignment_amd import synth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import border_band as bb  # noqa: E402
import feature_pairs as fp  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = fp.cases()
N = len(CASES)


# ---- building a case on the device ---------------------------------------------------------------------------------------
class Built:
    """the case's problems (head first), with the inputs as the device holds them.  inputs: what to build from where it is not
    fp.host_inputs(case) -- a rank's shard of them (fp.shard_inputs: uploaded points and weights, a term may have zero points)"""

    def __init__(self, hip, case, inputs=None):
        self.hip, self.case, self.probs, self.inputs = hip, case, [], []
        dt = hip.EA_F32 if case["dtype"] == "f32" else hip.EA_F64
        kind, a = fp.LOSS[case["loss"]]
        try:
            for s in (fp.host_inputs(case) if inputs is None else inputs):
                P = hip.Problem(*s["K"], dtype=dt)
                self.probs.append(P)
                if s["produced"]:   # the producer's own scatter, with the depth weights written behind it
                    P.set_depth_weighting(fp.Z_REF, fp.DEPTH_POWER)
                    P.set_ref_frame(s["bgr"], s["depth"], z_scaling=fp.Z_SCALING)
                else:
                    P.set_points(s["xyz"])
                    if s["weights"] is not None:
                        P.set_weights(s["weights"])
                P.set_dt_grid(s["grid"])
                P.set_loss(kind, a)
                if "distortion" in s["args"]:
                    P.set_distortion(*s["args"]["distortion"])
                if "T12" in s["args"]:
                    P.set_second_camera(s["args"]["T12"])
                if case["flavour"] == "ros":
                    P.set_flavour(0.0, 0.001, True)
                # the reference takes what the device holds; the host's statement of it is held to the same numbers
                xyz, w, image = P.get_points(), P.get_weights(), P.get_dt()
                assert np.array_equal(xyz, s["xyz"]) and xyz.shape == s["xyz"].shape, (case.name(), s["term"], "points")
                want_w = s["weights"] if len(s["xyz"]) else None   # (a term of zero points holds no weights)
                assert (w is None) == (want_w is None) and (w is None or np.array_equal(w, want_w)), (case.name(), s["term"], "weights")
                assert np.array_equal(image, s["image"]), (case.name(), s["term"], "image")
                self.inputs.append(dict(s, xyz=xyz, weights=w, image=image))
            self.P = self.probs[0]
            for T in self.probs[1:]:
                self.P.add_term(T)
            if case["loss"] == "auto":
                self.P.set_loss_auto_scale(*fp.AUTO_SCALE)
            pr = fp.prior(case)
            if pr["Aq"] is not None:
                self.P.set_normal_prior(0, pr["Aq"], pr["bq"])
            if pr["At"] is not None:
                self.P.set_normal_prior(1, pr["At"], pr["bt"])
            if any(fp.HELD[case["held"]]):
                self.P.set_constant_parameters(fp.HELD[case["held"]])
        except BaseException:
            self.close()
            raise
        self.key = tuple(case[n] for n in fp.NAMES) + (case["seed"], case["index"])

    def reset_loss(self):
        self.P.set_loss(*fp.LOSS[self.case["loss"]])   # (an auto-scaled solve leaves its scale behind)

    def ref(self, q, t, loss=None):
        return fp.reference(self.case, q, t, np.longdouble, self.inputs, loss, key=self.key)

    def bars(self, q, t, loss=None):
        if self.case["dtype"] == "f64":
            return dict(r=1e-12, J=1e-12, sums=1e-11)
        return fp.tolerances(self.case, q, t, self.inputs, loss, key=self.key)

    def close(self):
        if self.probs:
            self.probs[0].clear_terms() if len(self.probs) > 1 else None
        for P in self.probs:
            P.close()
        self.probs = []


def trio(index, solve=False):
    """the case with the array's previous and next cases (in the middle case's dtype: a batch has one)"""
    c = CASES[index]
    out = [CASES[(index - 1) % N].with_(dtype=c["dtype"]), c, CASES[(index + 1) % N].with_(dtype=c["dtype"])]
    return [fp.solve_case(x) for x in out] if solve else out


def tune(B, case):
    if case["shape"] == "ppt2":
        B.set_tuning("points_per_thread", 2)
    elif case["shape"] == "nt1024":
        B.set_tuning("threads", 1024)


def expected_shape(case, members):
    """what include/ea_hip.h documents for a batch of `members` tuned as `case` asks: the variant kernels (variant functors,
    weights, shared-pose terms) have the 256-thread shape only and put the whole batch on themselves; fp64 runs one point per
    lane in 1024-thread workgroups"""
    variant = any(fp.is_variant(m) for m in members)
    threads = 1024 if (case["shape"] == "nt1024" and not variant) else 256
    ppt = 2 if case["shape"] == "ppt2" else 1
    f64 = case["dtype"] == "f64"
    pose_ppt = 1 if (threads == 1024 and f64) else 2
    return dict(variant=variant, threads=threads, points_per_thread=ppt, weighted=sum(1 for m in members for s in fp.term_specs(m) if s["weights"] != "none"),
                wide_accumulate=0, dt_f32=1 if (f64 and not variant) else 0, poses_threads=threads, poses_points_per_thread=pose_ppt,
                flat=not variant and threads == 256, lanes=f64 and not variant and threads == 256)


def check_info(B, want, keys, where):
    for k in keys:
        assert B.info(k) == want[k], (where, k, B.info(k), want[k])


class Worst:
    """the comparisons of one form: every deviation as a share of its bar, the worst per dtype; the table is printed, then the
    misses fail"""

    def __init__(self, form):
        self.form, self.worst, self.n, self.missed = form, {"f64": (0.0, ""), "f32": (0.0, "")}, 0, []

    def add(self, dev, bar, where):
        self.n += 1
        share = dev / bar if np.isfinite(dev) else float("inf")
        ty = "f32" if "[f32 " in where else "f64"
        if share > self.worst[ty][0]:
            self.worst[ty] = (share, where)
        if not share <= 1.0:
            self.missed.append((where, float(dev), float(bar)))

    def __enter__(self):
        return self

    def __exit__(self, kind, value, tb):
        for ty in ("f64", "f32"):
            print("FEATURE-PAIRS-GPU %-26s %4d comparisons, %s worst %.3f of its bar at %s" % ((self.form, self.n, ty) + self.worst[ty]))
        for m in self.missed:
            print("FEATURE-PAIRS-GPU %-26s MISSED %s: %.3e against %.3e" % ((self.form,) + m))
        if kind is None:
            assert not self.missed, (self.form, self.missed[:5])
        return False


def got_sums(g, i=None, k=None):
    ix = () if i is None else ((i,) if k is None else (k, i))
    return dict(cost=float(np.asarray(g["cost"])[ix]), JtJ=np.asarray(g["JtJ"])[ix].reshape(6, 6), Jtr=np.asarray(g["Jtr"])[ix].reshape(6))


def check_sums(worst, built, g, q, t, where, i=None, k=None):
    ref, bars = built.ref(q, t), built.bars(q, t)
    assert int(np.asarray(g["n_invalid"])[() if i is None else ((i,) if k is None else (k, i))]) == ref["n_invalid"], (where, "n_invalid")
    assert ref["n_invalid"] == (1 if built.case["failed"] == "one" else 0), where
    worst.add(bb.dev_sums(got_sums(g, i, k), ref), bars["sums"], where)


def same_bits(a, b):
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in ("cost", "JtJ", "Jtr", "n_invalid"))


def pose0(case):
    q, t = fp.poses(case)
    return q[0], t[0]


# ---- the evaluation forms ------------------------------------------------------------------------------------------------
def test_form1_problem_eval(hip):
    with Worst("1 Problem.eval") as worst:
        for case in CASES:
            b = Built(hip, case)
            try:
                q, t = pose0(case)
                g = b.P.eval(q, t)
                check_sums(worst, b, g, q, t, case.name())
                cost, bad = b.P.cost(q, t)
                assert cost == g["cost"] and bad == g["n_invalid"], case.name()
            finally:
                b.close()


def test_form2_batch_eval(hip):
    bits = 0
    with Worst("2 Batch.eval") as worst:
        for i, case in enumerate(CASES):
            members = trio(i)
            built = [Built(hip, m) for m in members]
            B = B1 = None
            try:
                B = hip.Batch([b.P for b in built])
                tune(B, case)
                qt = [pose0(m) for m in members]
                g = B.eval(np.stack([p[0] for p in qt]), np.stack([p[1] for p in qt]))
                want = expected_shape(case, members)
                check_info(B, want, ("threads", "points_per_thread", "weighted", "wide_accumulate", "dt_f32"), case.name())
                for j, b in enumerate(built):
                    check_sums(worst, b, g, qt[j][0], qt[j][1], "%s member %d" % (case.name(), j), i=j)
                # against form 1: rounding only where the shape or the kernel family differs, the same bits otherwise
                B1 = hip.Batch([built[1].P])
                g1 = B1.eval(*qt[1])
                ps = built[1].P.eval(*qt[1])
                assert same_bits(got_sums(ps) | dict(n_invalid=ps["n_invalid"]), got_sums(g1, 0) | dict(n_invalid=g1["n_invalid"][0])), case.name()
                alone = expected_shape(fp.first_values(dtype=case["dtype"]), [case])
                if all(B.info(k) == B1.info(k) for k in ("threads", "points_per_thread")) and alone["variant"] == want["variant"]:
                    assert same_bits(got_sums(g, 1) | dict(n_invalid=g["n_invalid"][1]), got_sums(g1, 0) | dict(n_invalid=g1["n_invalid"][0])), case.name()
                    bits += 1
                else:
                    worst.add(bb.dev_sums(got_sums(g, 1), got_sums(g1, 0)), built[1].bars(*qt[1])["sums"], case.name() + " against form 1")
            finally:
                for x in (B, B1):
                    if x is not None:
                        x.close()
                for b in built:
                    b.close()
        assert bits >= 3, bits   # (the bit-equality leg is not vacuous)


def _check_rows(worst, b, r, J, ref, corrected, bars, where):
    """every row: r absolutely, J relative to the largest entry (border_band.dev_r / dev_J); failed blocks are NaN"""
    want_r, want_J = (ref["r"], ref["J"]) if corrected else (ref["raw_r"], ref["raw_J"])
    n = len(r)
    want_r, want_J = want_r[:n], want_J[:n]
    bad = np.isnan(want_r.astype(np.float64))
    assert np.array_equal(np.isnan(r), bad) and np.array_equal(np.isnan(J).any(axis=1), bad) and np.array_equal(np.isnan(J).all(axis=1), bad), where
    worst.add(bb.dev_r(r[~bad], want_r[~bad]), bars["r"], where + " r")
    worst.add(bb.dev_J(J[~bad], want_J[~bad]), bars["J"], where + " J")


def test_form3_points_and_rows(hip):
    with Worst("3 eval_points / eval_rows") as worst:
        for i, case in enumerate(CASES):
            members = trio(i)
            built = [Built(hip, m) for m in members]
            B = None
            try:
                b = built[1]
                q, t = pose0(case)
                ref, bars = b.ref(q, t), b.bars(q, t)
                total, head = len(ref["r"]), ref["head_rows"]
                for corrected in (True, False):
                    r, J = b.P.eval_points(q, t, corrected=corrected)       # the head's own family, float64
                    assert r.shape == (head,) and J.shape == (head, 6)
                    _check_rows(worst, b, r, J, ref, corrected, bars, "%s eval_points corrected=%d" % (case.name(), corrected))
                r0, J0, bad = b.P.eval_rows(q, t, corrected=True, layout=0)  # every term, the problem's dtype
                assert r0.shape == (total,) and bad == ref["n_invalid"], case.name()
                _check_rows(worst, b, r0, J0, ref, True, bars, case.name() + " eval_rows corrected layout 0")
                r1, J1, bad = b.P.eval_rows(q, t, corrected=False, layout=1)
                assert J1.shape == (6, total) and bad == ref["n_invalid"], case.name()
                _check_rows(worst, b, r1, J1.T, ref, False, bars, case.name() + " eval_rows raw layout 1")
                # the corrected rows sum to form 1's system (the prior is not in the rows)
                ok = ~np.isnan(r0)
                Jc, rc = J0[ok].astype(np.float64), r0[ok].astype(np.float64)
                pJ, pr, pc = fp.prior_terms(q, t, **fp.prior(case))
                g = b.P.eval(q, t)
                worst.add(max(bb.dev_J(Jc.T @ Jc + pJ, g["JtJ"]), bb.dev_J(Jc.T @ rc + pr, g["Jtr"])), bars["sums"], case.name() + " rows sum to eval")
                if case["loss"] == "trivial":
                    worst.add(bb.dev_rel(0.5 * rc @ rc + pc, g["cost"]), bars["sums"], case.name() + " rows sum to the cost")
                # the batch's rows: the middle problem's slice, the other layouts
                B = hip.Batch([x.P for x in built])
                off = B.row_offsets()
                qs, ts = np.stack([pose0(m)[0] for m in members]), np.stack([pose0(m)[1] for m in members])
                assert off[2] - off[1] == total, case.name()
                rb, Jb, bad = B.eval_rows(qs, ts, corrected=True, layout=1)
                assert bad == sum(x.ref(*pose0(x.case))["n_invalid"] for x in built), case.name()
                _check_rows(worst, b, rb[off[1]:off[2]], Jb[:, off[1]:off[2]].T, ref, True, bars, case.name() + " batch rows corrected layout 1")
                rb, Jb, _ = B.eval_rows(qs, ts, corrected=False, layout=0)
                _check_rows(worst, b, rb[off[1]:off[2]], Jb[off[1]:off[2]], ref, False, bars, case.name() + " batch rows raw layout 0")
            finally:
                if B is not None:
                    B.close()
                for x in built:
                    x.close()


def test_form4_eval_poses(hip):
    lanes_seen = 0
    with Worst("4 Batch.eval_poses K=3") as worst:
        for i, case in enumerate(CASES):
            members = trio(i)
            built = [Built(hip, m) for m in members]
            B = B1 = None
            try:
                B = hip.Batch([b.P for b in built])
                tune(B, case)
                want = expected_shape(case, members)
                qt = [fp.poses(m) for m in members]
                q = np.stack([p[0] for p in qt], axis=1)     # (K, n, 4)
                t = np.stack([p[1] for p in qt], axis=1)
                e = B.eval_poses(q, t)
                check_info(B, want, ("poses_threads", "poses_points_per_thread"), case.name())
                assert B.info("poses_lane_per_pose") == 0, case.name()    # (K = 3 is far below the threshold)
                assert B.info("poses_wave_exchange") == (1 if (case["dtype"] == "f64" and want["flat"]) else 0), case.name()
                for k in range(fp.K_POSES):
                    g = B.eval(q[k], t[k])
                    for j, b in enumerate(built):
                        check_sums(worst, b, e, q[k, j], t[k, j], "%s pose %d member %d" % (case.name(), k, j), i=j, k=k)
                        assert e["n_invalid"][k, j] == g["n_invalid"][j]
                        worst.add(bb.dev_sums(got_sums(e, j, k), got_sums(g, j)), b.bars(q[k, j], t[k, j])["sums"],
                                  "%s pose %d member %d against form 2" % (case.name(), k, j))
                if case["dtype"] == "f64" and case["functor"] == "plain":
                    # one pose per lane on and off: another fixed summation order, the same problem; a batch on the variant
                    # kernels (weights, a second term) or in 1024-thread workgroups keeps its kernel whatever the key says
                    b = built[1]
                    B1 = hip.Batch([b.P])
                    tune(B1, case)
                    alone = expected_shape(case, [case])
                    for on in (1, 0):
                        B1.set_tuning("poses_lane_per_pose", on)
                        e1 = B1.eval_poses(qt[1][0][:, None], qt[1][1][:, None])
                        assert B1.info("poses_lane_per_pose") == (1 if (on and alone["lanes"]) else 0), (case.name(), on)
                        lanes_seen += B1.info("poses_lane_per_pose")
                        for k in range(fp.K_POSES):
                            check_sums(worst, b, e1, qt[1][0][k], qt[1][1][k], "%s lanes=%d pose %d" % (case.name(), on, k), i=0, k=k)
            finally:
                for x in (B, B1):
                    if x is not None:
                        x.close()
                for b in built:
                    b.close()
        assert lanes_seen >= 1


def test_form5_cost_poses(hip):
    forms = set()
    with Worst("5 cost_poses") as worst:
        for i, case in enumerate(CASES):
            members = trio(i)
            built = [Built(hip, m) for m in members]
            B = None
            try:
                B = hip.Batch([b.P for b in built])
                tune(B, case)
                want = expected_shape(case, members)
                qt = [fp.poses(m) for m in members]
                c = B.cost_poses(np.stack([p[0] for p in qt], axis=1), np.stack([p[1] for p in qt], axis=1))
                assert B.info("cost_form") == (1 if want["flat"] else 0), (case.name(), B.info("cost_form"))
                forms.add(B.info("cost_form"))
                for k in range(fp.K_POSES):
                    for j, b in enumerate(built):
                        ref, bars = b.ref(qt[j][0][k], qt[j][1][k]), b.bars(qt[j][0][k], qt[j][1][k])
                        assert c["n_invalid"][k, j] == ref["n_invalid"], (case.name(), k, j)
                        worst.add(bb.dev_rel(c["cost"][k, j], ref["cost"]), bars["sums"], "%s pose %d member %d" % (case.name(), k, j))
            finally:
                if B is not None:
                    B.close()
                for b in built:
                    b.close()
        assert forms == {0, 1}


# ---- the solve forms ---------------------------------------------------------------------------------------------------------
def _check_solve(worst, case, got, want, where, counts=True):
    """got / want: (q, t, summary).  fp64: the reference's iteration count and `why`, poses within 1e-7 rad / 1e-7 m; fp32:
    1e-4 rad / 1e-3 m only"""
    q, t, s = got
    qr, tr, sr = want
    f64 = case["dtype"] == "f64"
    if f64 and counts:
        assert s["why"] == sr["why"] and s["num_iterations"] == sr["num_iterations"] and s["termination"] == sr["termination"], \
            (where, s["why"], sr["why"], s["num_iterations"], sr["num_iterations"])
    worst.add(synth.rotation_angle_between(q, qr), 1e-7 if f64 else 1e-4, where + " rotation")
    worst.add(float(np.linalg.norm(t - tr)), 1e-7 if f64 else 1e-3, where + " translation")
    held = fp.HELD[case["held"]]
    for i in range(3):
        if held[3 + i]:
            assert np.float64(t[i]).tobytes() == np.float64(tr[i]).tobytes(), (where, "held t", i)
    if all(held[:3]):
        assert np.asarray(q).tobytes() == np.asarray(qr, dtype=np.float64).tobytes(), (where, "held q")


def _ref_solve(b, q0, t0, auto):
    return fp.reference_solve(b.case, q0, t0, np.longdouble, b.inputs, auto=auto, key=b.key)


def _failed_start_ends_the_solve(hip, case, solve):
    """a case with a failed block: every solve ends at its first evaluation, the pose untouched"""
    b = Built(hip, case)
    try:
        q0, t0 = fp.poses(case, scaled=False)
        q, t, s = solve(b, q0[0], t0[0])
        assert s["termination"] == hip.FAILURE and s["why"] == "initial_eval_failed" and s["num_iterations"] == 0, (case.name(), s["why"])
        assert q.tobytes() == q0[0].tobytes() and t.tobytes() == t0[0].tobytes(), case.name()
    finally:
        b.close()


def test_form6_problem_solve(hip):
    doglegs = 0
    with Worst("6 Problem.solve") as worst:
        for i, c in enumerate(CASES):
            if c["failed"] == "one":
                _failed_start_ends_the_solve(hip, c, lambda b, q, t: b.P.solve(q, t))
            case = fp.solve_case(c)
            b = Built(hip, case)
            try:
                q0, t0 = fp.poses(case, scaled=False)
                want = _ref_solve(b, q0[0], t0[0], True)
                got = b.P.solve(q0[0], t0[0])
                _check_solve(worst, case, got, want, case.name() + " LM")
                if case["loss"] == "auto":
                    kind, a = b.P.get_loss()
                    # an order statistic moves by no more than the largest change of a sample: factor x the bar of the residuals
                    worst.add(abs(a - want[2]["loss"][1]), fp.AUTO_SCALE[0] * b.bars(q0[0], t0[0])["r"], case.name() + " auto scale")
                if i % 3 == 2:
                    # DOGLEG: reduced_lm restates the LM strategy only and no new restatement is written, so the dogleg solve is held
                    # to what the array is about -- no feature dropped on the way: it converges, the costs it reports at its two
                    # ends are the reference's costs of the whole problem (terms, weights, loss scale, prior) at those poses, and
                    # the held coordinates come back untouched.  The dogleg step itself is tests/test_gpu_lm_random.py's subject.
                    b.reset_loss()
                    q, t, s = b.P.solve(q0[0], t0[0], strategy=hip.STRATEGY_DOGLEG)
                    doglegs += 1
                    loss = want[2]["loss"]
                    assert s["termination"] == hip.CONVERGENCE and s["num_successful_steps"] >= 1, (case.name(), s["why"])
                    e0, e1, bars = b.ref(q0[0], t0[0], loss), b.ref(q, t, loss), b.bars(q0[0], t0[0], loss)
                    worst.add(bb.dev_rel(s["initial_cost"], e0["cost"]), bars["sums"], case.name() + " DOGLEG initial cost")
                    worst.add(bb.dev_rel(s["final_cost"], e1["cost"]), bars["sums"], case.name() + " DOGLEG final cost")
                    assert s["final_cost"] < s["initial_cost"], case.name()
                    for j in range(3):
                        assert not fp.HELD[case["held"]][3 + j] or np.float64(t[j]).tobytes() == np.float64(t0[0][j]).tobytes(), (case.name(), "DOGLEG held t")
                    assert not all(fp.HELD[case["held"]][:3]) or q.tobytes() == q0[0].tobytes(), (case.name(), "DOGLEG held q")
            finally:
                b.close()
        assert doglegs == N // 3


def test_form7_batch_solve(hip):
    bits, fused = 0, set()
    with Worst("7 Batch.solve") as worst:
        for i, c in enumerate(CASES):
            if c["failed"] == "one":
                def solve(b, q, t):
                    B = hip.Batch([b.P])
                    try:
                        qs, ts, ss = B.solve(q[None], t[None])
                        return qs[0], ts[0], ss[0]
                    finally:
                        B.close()
                _failed_start_ends_the_solve(hip, c, solve)
            members = trio(i, solve=True)
            case = members[1]
            built = [Built(hip, m) for m in members]
            B = None
            try:
                B = hip.Batch([b.P for b in built])
                tune(B, case)
                st = [fp.poses(m, scaled=False) for m in members]
                q0, t0 = np.stack([p[0][0] for p in st]), np.stack([p[1][0] for p in st])
                q, t, s = B.solve(q0, t0)
                want = expected_shape(case, members)
                check_info(B, want, ("threads", "points_per_thread", "weighted"), case.name())
                assert B.info("fused_iterations") == (1 if want["flat"] else 0), (case.name(), B.info("fused_iterations"))
                fused.add(B.info("fused_iterations"))
                for j, b in enumerate(built):
                    _check_solve(worst, b.case, (q[j], t[j], s[j]), _ref_solve(b, q0[j], t0[j], True), "%s member %d" % (case.name(), j))
                # against form 6: the same bits where the shape and the kernel family are the single solve's
                for b in built:
                    b.reset_loss()
                qs, ts, ss = built[1].P.solve(q0[1], t0[1])
                alone = expected_shape(fp.first_values(dtype=case["dtype"]), [case])
                if (want["threads"], want["points_per_thread"], want["variant"]) == (alone["threads"], alone["points_per_thread"], alone["variant"]):
                    assert np.array_equal(qs, q[1]) and np.array_equal(ts, t[1]) and ss["num_iterations"] == s[1]["num_iterations"], case.name()
                    assert np.array_equal(ss["it_cost"], s[1]["it_cost"]), case.name()
                    bits += 1
            finally:
                if B is not None:
                    B.close()
                for b in built:
                    b.close()
        assert bits >= 3 and fused == {0, 1}, (bits, fused)


def test_form8_solve_starts(hip):
    forms = set()
    with Worst("8 solve_starts K=3") as worst:
        for i, c in enumerate(CASES):
            case = fp.solve_case(c)
            b = Built(hip, case)
            B = None
            try:
                B = hip.Batch([b.P])
                tune(B, case)
                want = expected_shape(case, [case])
                q0, t0 = fp.poses(case, scaled=False)
                q, t, s, best = B.solve_starts(q0[:, None], t0[:, None])
                assert B.info("starts_form") == (1 if want["flat"] else 0), (case.name(), B.info("starts_form"))
                forms.add(B.info("starts_form"))
                kind, a = b.P.get_loss()
                assert (kind, a) == fp.LOSS[case["loss"]], case.name()   # multi-start runs with the problem's own loss: no estimate
                refs = []
                for k in range(fp.K_POSES):
                    refs.append(_ref_solve(b, q0[k], t0[k], False))
                    _check_solve(worst, case, (q[k, 0], t[k, 0], s[k][0]), refs[k], "%s start %d" % (case.name(), k))
                    # a start's result is bit for bit what the same start gives alone
                    q1, t1, s1, b1 = B.solve_starts(q0[k][None, None], t0[k][None, None])
                    assert np.array_equal(q1[0, 0], q[k, 0]) and np.array_equal(t1[0, 0], t[k, 0]) and b1[0] == 0, (case.name(), k)
                    assert s1[0][0]["num_iterations"] == s[k][0]["num_iterations"] and np.array_equal(s1[0][0]["it_cost"], s[k][0]["it_cost"]), (case.name(), k)
                cost = np.array([float(r[2]["final_cost"]) for r in refs])
                # the reference's best.  The order of two starts can differ from the reference's only where their final costs are
                # closer than the device's final costs are to the reference's: those starts are all the best
                mine = np.array([x[0]["final_cost"] for x in s])
                ties = [k for k in range(fp.K_POSES) if cost[k] - cost.min() <= 2.0 * np.abs(mine - cost).max()]
                assert best[0] in ties, (case.name(), int(best[0]), cost)
                assert best[0] == int(np.argmin([x[0]["final_cost"] for x in s])), case.name()
            finally:
                if B is not None:
                    B.close()
                b.close()
        assert forms == {0, 1}


def test_form9_covariance(hip):
    with Worst("9 covariance") as worst:
        for i, case in enumerate(CASES):
            members = trio(i)
            built = [Built(hip, m) for m in members]
            B = None
            try:
                B = hip.Batch([b.P for b in built])
                tune(B, case)
                qt = [fp.poses(m, scaled=False) for m in members]
                q, t = np.stack([p[0][0] for p in qt]), np.stack([p[1][0] for p in qt])
                cb = B.covariance(q, t)
                gb = B.eval(q, t)
                for j, b in enumerate(built):
                    where = "%s member %d" % (case.name(), j)
                    held = fp.HELD[b.case["held"]]
                    m = 6 - sum(held)
                    ref = b.ref(q[j], t[j])
                    c = b.P.covariance(q[j], t[j])
                    if b.case["failed"] == "one":
                        assert not c["ok"] and c["why"] == 2 and c["n_invalid"] == 1 and not cb[j]["ok"] and cb[j]["why"] == 2, where
                        continue
                    assert c["ok"] and c["rank"] == m and c["why"] == 0 and cb[j]["ok"] and cb[j]["rank"] == m, (where, c["rank"], c["why"])
                    g = b.P.eval(q[j], t[j])
                    own = 1e-12 if b.case["prior"] == "none" else 1e-10
                    worst.add(bb.dev_rel(c["tangent"], fp.reduced_pinv(g["JtJ"], held)), own, where + " against the device's own JtJ")
                    worst.add(bb.dev_rel(cb[j]["tangent"], fp.reduced_pinv(gb["JtJ"][j], held)), own, where + " batch against the batch's own JtJ")
                    free = [x for x in range(6) if not held[x]]
                    red = np.asarray(ref["JtJ"], dtype=np.float64)[np.ix_(free, free)]
                    # fp64: the bar of tests/test_gpu_constant_parameters.py.  fp32: the inverse of a matrix known to a relative
                    # delta is known to cond x delta (first-order perturbation of the inverse), delta the bar of the sums
                    bar = 1e-8 if b.case["dtype"] == "f64" else float(np.linalg.cond(red)) * b.bars(q[j], t[j])["sums"]
                    worst.add(bb.dev_rel(c["tangent"], fp.reduced_pinv(ref["JtJ"], held)), bar, where + " against the reference")
                    worst.add(bb.dev_rel(cb[j]["tangent"], fp.reduced_pinv(ref["JtJ"], held)), bar, where + " batch against the reference")
                    h = np.array(held, dtype=bool)
                    assert not c["tangent"][h].any() and not c["tangent"][:, h].any() and not cb[j]["tangent"][h].any(), where
            finally:
                if B is not None:
                    B.close()
                for b in built:
                    b.close()


# ---- the pairs the header refuses or ignores: one dedicated case each ---------------------------------------------------------
def _refused(hip, fn):
    with pytest.raises(hip.EAError) as ei:
        fn()
    assert ei.value.code != hip.EA_OK and hip.load().ea_last_error().decode(), "a refusal carries a message"


def test_refused_or_ignored(hip):
    done = set()
    base = fp.first_values()
    q, t = pose0(base)

    def pair(**kw):
        return Built(hip, base), Built(hip, fp.first_values(**kw))

    # a term cannot carry a prior or a mask, neither before nor after it becomes a term
    for name, setter in (("term with a prior", lambda P: P.set_normal_prior(1, fp.prior(base.with_(prior="t2"))["At"], fp.PLANTED_T)),
                         ("term with a mask", lambda P: P.set_constant_parameters(fp.HELD["tz"]))):
        a, b = pair()
        try:
            a.P.add_term(b.P)
            _refused(hip, lambda: setter(b.P))
            a.P.clear_terms()
            setter(b.P)
            _refused(hip, lambda: a.P.add_term(b.P))
            setter(a.P)                    # the head may carry both
            assert a.P.eval(q, t)["n_invalid"] == 0
        finally:
            a.close(); b.close()
        done.add(name)
    a, b = pair(dtype="f32")
    try:
        _refused(hip, lambda: (a.P.add_term(b.P), a.P.eval(q, t)))
    finally:
        a.P.clear_terms(); a.close(); b.close()
    done.add("terms of two dtypes")
    a, b = pair(flavour="ros")
    try:
        _refused(hip, lambda: (a.P.add_term(b.P), a.P.eval(q, t)))
    finally:
        a.P.clear_terms(); a.close(); b.close()
    done.add("terms that disagree on rot_transposed")
    a, b = pair()
    try:
        a.P.set_loss_auto_scale(*fp.AUTO_SCALE)
        _refused(hip, lambda: a.P.add_term(b.P))
        a.P.set_loss_auto_scale(0.0)
        b.P.set_loss_auto_scale(*fp.AUTO_SCALE)
        _refused(hip, lambda: a.P.add_term(b.P))
        b.P.set_loss_auto_scale(0.0)
        a.P.add_term(b.P)
        _refused(hip, lambda: a.P.set_loss_auto_scale(*fp.AUTO_SCALE))
        _refused(hip, lambda: b.P.set_loss_auto_scale(*fp.AUTO_SCALE))
    finally:
        a.P.clear_terms(); a.close(); b.close()
    done.add("auto-scaled loss with terms")
    # "threads" = 1024 on the variant kernels: the shape and the bits of the same batch without the key
    for kw in [dict(functor=f) for f in fp.VARIANT_FUNCTORS] + [dict(weights="real"), dict(weights="depth"), dict(terms="two")]:
        for dtype in ("f64", "f32"):
            b = Built(hip, fp.first_values(dtype=dtype, **kw))
            B0, B1 = hip.Batch([b.P]), hip.Batch([b.P])
            try:
                B1.set_tuning("threads", 1024)
                g0, g1 = B0.eval(q, t), B1.eval(q, t)
                assert B1.info("threads") == 256 == B0.info("threads") and B1.info("points_per_thread") == B0.info("points_per_thread"), kw
                assert same_bits(g0, g1), kw
            finally:
                B0.close(); B1.close(); b.close()
    # (and it is honoured where the header does not say otherwise)
    b = Built(hip, base)
    B1 = hip.Batch([b.P])
    try:
        B1.set_tuning("threads", 1024)
        B1.eval(q, t)
        assert B1.info("threads") == 1024
    finally:
        B1.close(); b.close()
    done.add("threads = 1024 on the variant kernels")
    # z_guard = 0: the block that fails under the default flavour is an ordinary block
    case = fp.first_values(flavour="ros", failed="one")
    b = Built(hip, case)
    try:
        qr, tr = pose0(case)
        ref = b.ref(qr, tr)
        g = b.P.eval(qr, tr)
        assert g["n_invalid"] == 0 == ref["n_invalid"]
        assert bb.dev_sums(got_sums(g), ref) <= 1e-11
        r, J = b.P.eval_points(qr, tr, corrected=False)
        assert not np.isnan(r).any() and not np.isnan(J).any()
    finally:
        b.close()
    b = Built(hip, case.with_(flavour="default"))
    try:
        assert b.P.eval(*pose0(case.with_(flavour="default")))["n_invalid"] == 1   # (the same block does fail under the default flavour)
    finally:
        b.close()
    done.add("z_guard = 0 has no failed block")
    assert done == {e["name"] for e in fp.REFUSED_OR_IGNORED}


# ---- a tuning key that did not rebuild -----------------------------------------------------------------------------------------
def _solve_state(B, q0, t0):
    q, t, s = B.solve(q0, t0, max_num_iterations=8)
    return dict(q=q, t=t, it=[x["num_iterations"] for x in s], cost=[x["it_cost"] for x in s],
                info={k: B.info(k) for k in ("fused_iterations", "points_per_thread", "threads", "chunk")})


def _same_state(a, b):
    return (np.array_equal(a["q"], b["q"]) and np.array_equal(a["t"], b["t"]) and a["it"] == b["it"] and a["info"] == b["info"]
            and all(np.array_equal(x, y) for x, y in zip(a["cost"], b["cost"])))


def test_fused_iterations_key_rebuilds_the_batch(hip):
    """batch_build reads "fused_iterations" when it picks the workgroup size and the points per lane: 70 000 fp64 points run
    256 x 2 where the fused form is allowed (at most 255 chunks) and 256 x 1 where it is not.  A batch that has already run
    takes the new value's shape and form when the key changes: each state equals a fresh batch created with that value."""
    pr = synth.make_problem(120, 160, 70000, 40, 5, 130.0, 130.0, 79.5, 59.5, planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)),
                            planted_t=(0.01, -0.005, 0.02), normalize=True)
    P = hip.Problem(*pr["K"])
    P.set_points(pr["xyz"]); P.set_dt_grid(pr["grid"]); P.set_loss(hip.LOSS_CAUCHY, 1.0)
    q0, t0 = np.array([[1.0, 0, 0, 0]]), np.zeros((1, 3))
    fresh = {}
    for v in (-1, 0):
        B = hip.Batch([P])
        B.set_tuning("fused_iterations", v)
        fresh[v] = _solve_state(B, q0, t0)
        B.close()
    assert fresh[-1]["info"]["fused_iterations"] == 1 and fresh[-1]["info"]["points_per_thread"] == 2, fresh[-1]["info"]
    assert fresh[0]["info"]["fused_iterations"] == 0 and fresh[0]["info"]["points_per_thread"] == 1, fresh[0]["info"]
    B = hip.Batch([P])
    try:
        for v in (-1, 0, -1, 0):
            B.set_tuning("fused_iterations", v)
            assert _same_state(_solve_state(B, q0, t0), fresh[v]), (v, B.info("points_per_thread"), B.info("fused_iterations"))
    finally:
        B.close()
        P.close()


def test_fused_iterations_key_reaches_the_stream_parts(hip):
    """a batch solved as sub-batches on several streams ("solve_streams"): the parts take the key too, and the batch the caller
    holds reports the form they ran"""
    built = [Built(hip, fp.first_values(loss="cauchy", dtype="f64")) for _ in range(4)]
    q0, t0 = fp.poses(built[0].case, scaled=False)
    qs, ts = np.tile(q0[0], (4, 1)), np.tile(t0[0], (4, 1))
    fresh = {}
    try:
        for v in (-1, 0):
            B = hip.Batch([b.P for b in built])
            B.set_tuning("fused_iterations", v)
            fresh[v] = _solve_state(B, qs, ts)
            B.close()
        assert fresh[-1]["info"]["fused_iterations"] == 1 and fresh[0]["info"]["fused_iterations"] == 0
        B = hip.Batch([b.P for b in built])
        B.set_tuning("solve_streams", 2)
        for v in (-1, 0, -1):
            B.set_tuning("fused_iterations", v)
            assert _same_state(_solve_state(B, qs, ts), fresh[v]), (v, B.info("fused_iterations"))
        B.close()
    finally:
        for b in built:
            b.close()
