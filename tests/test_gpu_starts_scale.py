"""ea_batch_solve_starts with hundreds to 16 384 starts: the live-list compaction of ea_lm_step_starts_kernel over several rounds
of 256 positions, iterations cut into several (evaluate, step) pieces from a stale list length, alive[start] over several
problems, and the 16 384-slot limit -- none of which a call of K <= 12 starts reaches.

Every big call is laid out by INDEXING a catalogue of 26 distinct starts (tests/scale_cases.py; tests/test_scale_catalogue.py
holds what it rests on to the oracle): F fails its first evaluation, Q ends within 2 iterations, 24 S starts end after 13 .. 48.
Each catalogue start is solved ALONE (K = 1) once per module; every position of every big call must equal its catalogue entry
bit for bit under _same of test_gpu_solve_starts.py (pose, iterations, termination, why, the whole it_cost trace) -- the
header's promise that a start does not depend on its company -- and `best` must be the lowest position among the non-failed
starts of minimal final cost.  The lone solves themselves are held to the oracle's solve from the same start at the 1e-7 rad /
1e-7 m of test_gpu_solve_starts.py.  starts_form, starts_launches and starts_iterations are asserted through Batch.info before
a number is compared.

The pinned block a call's results are delivered into is not cleared between calls, and a (start, problem) writes its slot only
when its solve ends: a start that a wrong compaction drops while it runs is never delivered, and the host would hand back what
an earlier call left in that slot.  So every checked call is preceded by scale_cases.scrub of its own layout -- F where the
pattern has S or Q, Q where it has F, max_num_iterations = 0 -- in which every start ends in the first step launch, on the list
the host wrote (asserted: no iteration, F's pose back), and leaves a result in every slot that differs from the checked call's.
A slot the checked call does not deliver then fails the comparison, whatever ran before.

What a wrong compaction does to the patterns (K = 600 is rounds of 256, 256 and 88 positions).  A start dropped from the list is
never delivered: its slot still holds the scrub's result.  One listed twice is stepped by two workgroups, one written to a wrong
slot displaces another start or is lost behind n_out; the iteration count, trace and pose then leave the lone solve's:
  all_s              every round keeps some and drops some at most iterations: a `kept` that is not carried (rounds >= 1 write
                     from slot 0) overwrites round 0's survivors, one carried wrongly leaves holes or a wrong n_out;
  first_round_f      round 0 keeps nothing from the first iteration on: survivors of rounds 1 and 2 must land at slot 0 -- a
                     carry of the round's lane count (256) instead of its kept count puts them at slot 256;
  second_round_f     round 1 keeps nothing: round 2's survivors go right behind round 0's; a slot computed from the round's own
                     masks alone, or a round skipped because the one before it was empty, drops them;
  lone_slowest_at_P  after iteration 2 one start is left, at position 0 (first lane of round 0), 255 (last lane of its last
                     wavefront), 256 (first lane of round 1) or 599 (the last live position, in the partly filled round): a
                     survivor dropped at a round or wavefront edge, or an i < n_live test off by one, loses it;
  alternating        every other lane of every wavefront is dropped at once: the prefix count within a ballot mask;
  alternating_wavefronts  whole wavefronts keep all or nothing: the sum over the lower wavefronts' masks;
  K = 256, 257, 512, 513  the loop bound on a round's edge: a second / third round of no or one position.
The same calls with "poses_per_launch" 100 / 256 / 0 cut an iteration into pieces that end inside a round and on its edge
(only the last piece's step launch counts workgroups in and rebuilds the list).  With iterations_per_sync = 1 the host enqueues
an iteration only after it has read the previous one's word: the length it sizes the pieces from is exact.  With 4 (and the
default 2 of the other cases) it runs ahead, and the pieces are sized from a length up to three iterations old.

Measured on an MI355X: every converged catalogue start (all 25) takes the oracle's iteration count (Q 1, S 13 .. 48) and lands
within 0 rad / 3.2e-16 m of the oracle's pose (the planted pose, cost 0); every position of every call equal to its lone solve.
With the `kept` carry of the compaction taken out on purpose (one run, not committed) every case but the one-round K = 256
failed on a lone-start mismatch; with one survivor of a later round dropped once, at iteration 9 (another such run), every case
that still lists more than 256 starts then failed -- all 24 split cases among them, each of which repeats its predecessor's
layout -- on the slot the scrub had left.  The 42 cases take 3 s, 2 s of it the module's fixture."""
import numpy as np
import pytest

import scale_cases as sc
from edge_alignment_amd import synth
from test_gpu_solve_starts import _problem, _same, _within

pytestmark = pytest.mark.gpu

PATTERNS = [sc.all_s, sc.first_round_f, sc.second_round_f, sc.lone_slowest_at(0), sc.lone_slowest_at(255), sc.lone_slowest_at(256),
            sc.lone_slowest_at(599), sc.alternating, sc.alternating_wavefronts]


def _lone_solves(hip, P, q0, t0):
    """every catalogue start alone: [(q, t, summary)], failed[], final_cost[]"""
    ref = []
    for k in range(len(q0)):
        q, t, s, best = P.solve_starts(q0[k:k + 1], t0[k:k + 1])
        assert best == (0 if s[0]["termination"] != hip.FAILURE else -1), k
        ref.append((q[0], t[0], s[0]))
    failed = np.array([r[2]["termination"] == hip.FAILURE for r in ref])
    cost = np.array([r[2]["final_cost"] for r in ref])
    return ref, failed, cost


@pytest.fixture(scope="module")
def cat(hip, oracle):
    """the catalogue, its problem in a batch of one, and the lone solves: the reference bits of this module"""
    base = sc.starts_base()
    X = base["xyz"][:sc.N_ROW]
    P = _problem(hip, base, X)
    B = hip.Batch([P])
    q0, t0 = sc.catalogue(oracle, X)
    ref, failed, cost = _lone_solves(hip, P, q0, t0)
    its = np.array([r[2]["num_iterations"] for r in ref])
    slowest = sc.S0 + int(np.argmax(its[sc.S0:]))
    yield dict(base=base, X=X, P=P, B=B, q0=q0, t0=t0, ref=ref, failed=failed, cost=cost, its=its, slowest=slowest)
    B.close(); P.close()


def _check_call(w, idx, q, t, s, best, where, ref=None, failed=None, cost=None):
    ref = w["ref"] if ref is None else ref
    for j, c in enumerate(idx):
        if s is not None:
            assert _same((q[j], t[j], s[j]), ref[c]), where + (j, int(c), s[j]["num_iterations"], ref[c][2]["num_iterations"])
        else:
            assert np.array_equal(q[j], ref[c][0]) and np.array_equal(t[j], ref[c][1]), where + (j, int(c))
    assert best == sc.expected_best(idx, w["failed"] if failed is None else failed, w["cost"] if cost is None else cost), where


def _scrub(B, cats, idxs, summaries=True):
    """scale_cases.scrub of the layout idxs (one index array per problem of B, into that problem's catalogue cats[i]) in front of
    a checked call: every slot of the delivery block rewritten in the first step launch, with something the checked call does
    not expect there"""
    sidx = [sc.scrub(a) for a in idxs]
    q0 = np.stack([cats[i][0][a] for i, a in enumerate(sidx)], axis=1); t0 = np.stack([cats[i][1][a] for i, a in enumerate(sidx)], axis=1)
    q, t, s, _ = B.solve_starts(q0, t0, summaries=summaries, max_num_iterations=0)
    assert B.info("starts_form") == 1
    for i, a in enumerate(sidx):
        at_f = a == sc.F
        assert np.array_equal(q[at_f, i], q0[at_f, i]) and np.array_equal(t[at_f, i], t0[at_f, i]), i
        if s is not None:
            for k in range(len(a)):
                assert s[k][i]["num_iterations"] == 0 and (s[k][i]["why"] == "initial_eval_failed") == bool(at_f[k]), (k, i)


def _run(w, idx, summaries=True, **opts):
    B = w["B"]
    _scrub(B, [(w["q0"], w["t0"])], [idx], summaries)
    q, t, s, best = B.solve_starts(w["q0"][idx][:, None, :], w["t0"][idx][:, None, :], summaries=summaries, **opts)
    assert B.info("starts_form") == 1
    longest = int(w["its"][idx].max())
    assert B.info("starts_launches") >= longest and B.info("starts_iterations") >= longest
    return q[:, 0], t[:, 0], None if s is None else [x[0] for x in s], int(best[0])


def test_lone_solves_follow_the_oracle(hip, oracle, cat):
    """Every catalogue start whose oracle solve ends in CONVERGENCE converges on the device to the oracle's pose (1e-7 / 1e-7, the
    bars of test_gpu_solve_starts.py); at most 2 S starts may be left out.  F fails its first evaluation and keeps its pose; Q ends
    within 2 iterations; the S counts spread (the compaction has work at many iterations)."""
    w = cat
    O = oracle.OracleProblem(w["base"]["grid"], *w["base"]["K"], loss=hip.LOSS_CAUCHY, loss_a=sc.LOSS_CAUCHY_A)
    left_out, worst = [], [0.0, 0.0]
    for k in range(sc.Q, len(w["q0"])):
        qo, to, so = O.solve(w["X"], w["q0"][k], w["t0"][k])
        if so["termination"] != 0:
            left_out.append(k)
            continue
        q, t, s = w["ref"][k]
        ang, dt = synth.rotation_angle_between(q, qo), np.linalg.norm(t - to)
        worst = [max(worst[0], ang), max(worst[1], dt)]
        print("start", k, "oracle its", so["num_iterations"], "device its", s["num_iterations"], "angle", ang, "dt", dt)
        assert s["termination"] == hip.CONVERGENCE, k
        assert _within(q, t, qo, to, 1e-7, 1e-7), k
    print("worst angle / dt against the oracle:", worst, "left out:", left_out)
    assert len(left_out) <= 2 and sc.Q not in left_out
    q, t, s = w["ref"][sc.F]
    assert s["why"] == "initial_eval_failed" and s["final_cost"] == -1.0 and w["failed"][sc.F] and not w["failed"][sc.Q:].any()
    assert np.array_equal(q, w["q0"][sc.F]) and np.array_equal(t, w["t0"][sc.F])
    assert w["ref"][sc.Q][2]["num_iterations"] <= 2
    from test_gpu_solve_starts import _starts           # (the helper's restatement of the draw: the same bits)
    assert all(np.array_equal(a, b) for a, b in zip(sc.draw_starts(4.0, sc.N_S, sc.SEED), _starts(4.0, K=sc.N_S, seed=sc.SEED)))
    its = w["its"][sc.S0:]
    assert len(set(its)) >= 6 and its.max() - its.min() >= 5 and its.min() > 2


@pytest.mark.parametrize("pattern", PATTERNS, ids=lambda p: p.__name__)
def test_three_compaction_rounds(hip, cat, pattern):
    """K = 600: rounds of 256, 256 and 88 positions"""
    idx = pattern(600, cat["slowest"])
    cat["B"].set_tuning("poses_per_launch", 0)
    q, t, s, best = _run(cat, idx)
    _check_call(cat, idx, q, t, s, best, (pattern.__name__,))


@pytest.mark.parametrize("K", [256, 257, 512, 513])
def test_rounds_that_end_on_the_edge(hip, cat, K):
    idx = sc.all_s(K)
    cat["B"].set_tuning("poses_per_launch", 0)
    q, t, s, best = _run(cat, idx)
    _check_call(cat, idx, q, t, s, best, (K,))


@pytest.mark.parametrize("summaries", [True, False], ids=["summaries", "poses_only"])
@pytest.mark.parametrize("iterations_per_sync", [1, 4])
@pytest.mark.parametrize("per_launch", [100, 256, 0])
@pytest.mark.parametrize("pattern", [sc.all_s, sc.alternating], ids=lambda p: p.__name__)
def test_pieces_of_an_iteration_and_a_stale_length(hip, cat, pattern, per_launch, iterations_per_sync, summaries):
    """K = 600 in pieces of at most 100 (six per iteration at first, ending inside the rounds), 256 (three pieces of 200) and in
    one piece; iterations_per_sync = 1: the host sizes the pieces from the exact length, 4: from one up to three iterations old"""
    B = cat["B"]
    idx = pattern(600, cat["slowest"])
    B.set_tuning("poses_per_launch", per_launch)
    try:
        q, t, s, best = _run(cat, idx, summaries=summaries, iterations_per_sync=iterations_per_sync)
        assert (s is None) == (not summaries)
        if per_launch:
            assert B.info("starts_launches") > B.info("starts_iterations")
        else:
            assert B.info("starts_launches") == B.info("starts_iterations")
        _check_call(cat, idx, q, t, s, best, (pattern.__name__, per_launch, iterations_per_sync, summaries))
    finally:
        B.set_tuning("poses_per_launch", 0)


def test_a_start_survives_on_one_problem_only(hip, oracle, cat):
    """A ragged batch of 300, 513 and 1 points, K = 300: where problem 0's start is F, problem 1's is S, and the reverse; problem 2
    gets Q everywhere -- alive[start] falls 3 -> 2 -> 1 -> 0 at three different iterations and a start stays listed for one problem.
    Reference: each problem's own catalogue through Problem.solve_starts, bits per (start, problem) as in
    test_ragged_batch_equals_single_problem_calls."""
    base, K = cat["base"], 300
    clouds = [cat["X"], base["xyz"][1000:1513], base["xyz"][2000:2001]]
    probs = [_problem(hip, base, X) for X in clouds]
    B = hip.Batch(probs)
    try:
        cats = [(cat["q0"], cat["t0"])] + [sc.catalogue(oracle, X) for X in clouds[1:]]
        refs = [_lone_solves(hip, P, q0, t0) for P, (q0, t0) in zip(probs, cats)]
        assert all(_same(a, b) for a, b in zip(refs[0][0], cat["ref"]))           # (problem 0 is the module's problem)
        k = np.arange(K)
        idx = [np.where(k % 2 == 0, sc.F, sc.S0 + k % sc.N_S), np.where(k % 2 == 0, sc.S0 + (k + 5) % sc.N_S, sc.F), np.full(K, sc.Q)]
        q0 = np.stack([cats[i][0][idx[i]] for i in range(3)], axis=1); t0 = np.stack([cats[i][1][idx[i]] for i in range(3)], axis=1)
        for per_launch in (0, 100):
            B.set_tuning("poses_per_launch", per_launch)
            _scrub(B, cats, idx)
            q, t, s, best = B.solve_starts(q0, t0)
            assert B.info("starts_form") == 1 and B.info("poses_tiles") == 4
            assert B.info("starts_launches") >= max(x[i]["num_iterations"] for x in s for i in range(3))
            for i in range(3):
                ref, failed, cost = refs[i]
                _check_call(cat, idx[i], q[:, i], t[:, i], [x[i] for x in s], int(best[i]), (per_launch, i), ref=ref, failed=failed, cost=cost)
    finally:
        B.close()
        for P in probs:
            P.close()


def test_the_slot_limit_in_one_problem(hip, cat):
    """K x count = 16 384 exactly, one problem; without summaries (the pinned trace block of 16 384 summaries is about 100 MB)"""
    idx = sc.permuted(16384, 91)
    cat["B"].set_tuning("poses_per_launch", 0)
    q, t, s, best = _run(cat, idx, summaries=False)
    assert s is None
    _check_call(cat, idx, q, t, None, best, ("16384 x 1",))


@pytest.fixture(scope="module")
def four(hip, cat):
    """four problems over the catalogue's cloud"""
    probs = [_problem(hip, cat["base"], cat["X"]) for _ in range(4)]
    B = hip.Batch(probs)
    yield B
    B.close()
    for P in probs:
        P.close()


@pytest.mark.parametrize("K,summaries", [(4096, False), (512, True)], ids=["4096x4_slot_limit", "512x4_traces"])
def test_the_slot_limit_in_four_problems(hip, cat, four, K, summaries):
    """K x count = 16 384 as (4 096, 4), poses and best against the catalogue; 2 048 slots with summaries for the traces.  Each
    problem has its own permutation: a start is alive on its four problems for four different spans."""
    idx = [sc.permuted(K, 100 + i) for i in range(4)]
    q0 = np.stack([cat["q0"][a] for a in idx], axis=1); t0 = np.stack([cat["t0"][a] for a in idx], axis=1)
    _scrub(four, [(cat["q0"], cat["t0"])] * 4, idx, summaries)
    q, t, s, best = four.solve_starts(q0, t0, summaries=summaries)
    assert four.info("starts_form") == 1 and four.info("poses_tiles") == 4 and best.shape == (4,)
    assert four.info("starts_launches") >= cat["its"].max()
    for i in range(4):
        _check_call(cat, idx[i], q[:, i], t[:, i], [x[i] for x in s] if summaries else None, int(best[i]), (K, i))
