"""What the patterns of tests/test_gpu_starts_scale.py rest on, checked on the CPU oracle alone (tests/scale_cases.py builds the
catalogue): F fails its first evaluation, Q ends within 2 iterations, and the S starts converge after iteration counts that
spread -- at least 6 distinct counts, at least 5 apart from shortest to longest -- so that the live list of a big call
shrinks a little at a time, over many compaction passes.  At most 2 S starts may miss CONVERGENCE on the oracle (the GPU test
leaves those out of its comparison with the oracle's pose); with the seed scale_cases.SEED none does (iterations 13 .. 48,
16 distinct counts).  Every pattern is a total map of positions onto catalogue entries with the blocks where its name says."""
import numpy as np

import scale_cases as sc


def test_catalogue_on_the_oracle(oracle):
    base = sc.starts_base()
    X = base["xyz"][:sc.N_ROW]
    O = oracle.OracleProblem(base["grid"], *base["K"], loss=oracle.LOSS_CAUCHY, loss_a=sc.LOSS_CAUCHY_A)
    q, t = sc.catalogue(oracle, X)
    assert q.shape == (2 + sc.N_S, 4) and len({tuple(np.r_[q[k], t[k]]) for k in range(len(q))}) == len(q)   # distinct starts
    _, _, s = O.solve(X, q[sc.F], t[sc.F])
    assert s["why"] == "initial_eval_failed" and s["termination"] == 2
    _, _, s = O.solve(X, q[sc.Q], t[sc.Q])
    assert s["termination"] == 0 and s["num_iterations"] <= 2
    its, left_out = [], []
    for k in range(sc.S0, len(q)):
        _, _, s = O.solve(X, q[k], t[k])
        if s["termination"] != 0:
            left_out.append(k)
        else:
            its.append(s["num_iterations"])
    print("S iterations on the oracle:", sorted(its), "not converged:", left_out)
    assert len(left_out) <= 2
    assert len(set(its)) >= 6 and max(its) - min(its) >= 5
    assert min(its) > 2              # (a lone S among F and Q is the only start left after iteration 2)


def test_patterns_put_their_blocks_where_they_say():
    K, slow = 600, sc.S0 + 7
    n = 2 + sc.N_S
    is_s = lambda idx: idx >= sc.S0
    assert is_s(sc.all_s(K)).all() and set(sc.all_s(K)) == set(range(sc.S0, n))
    a = sc.first_round_f(K)
    assert (a[:256] == sc.F).all() and is_s(a[256:]).all()
    a = sc.second_round_f(K)
    assert is_s(a[:256]).all() and (a[256:512] == sc.F).all() and is_s(a[512:]).all()
    for pos in (0, 255, 256, 599):
        a = sc.lone_slowest_at(pos)(K, slow)
        assert a[pos] == slow and int(is_s(a).sum()) == 1 and {sc.F, sc.Q} <= set(a)
    a = sc.alternating(K)
    assert is_s(a[0::2]).all() and (a[1::2] == sc.F).all()
    a = sc.alternating_wavefronts(K)
    assert is_s(a[:64]).all() and (a[64:128] == sc.F).all() and is_s(a[128:192]).all() and (a[576:] == sc.F).all()
    a = sc.permuted(16384, 1)
    assert np.bincount(a, minlength=n).min() >= 16384 // n and not np.array_equal(a, np.sort(a))
    # best: the lowest position among the non-failed starts of minimal final cost
    failed = np.array([True, False, False]); cost = np.array([-1.0, 2.0, 2.0])
    assert sc.expected_best(np.array([0, 2, 1, 2]), failed, cost) == 1 and sc.expected_best(np.array([0, 0]), failed, cost) == -1
