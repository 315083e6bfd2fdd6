"""The wave-exchange reduction of the fp64 pose-batched evaluation (tuning key "poses_wave_exchange", default 1: the four
wavefronts of a 256-lane workgroup add their 32 sums lane by lane through LDS in two rounds and each runs the butterfly over
the 8 slots it is left with; ea_wave_exchange.h) on the 120 x 160 synthetic pair of test_gpu_poses_flat.py, Cauchy(0.7)
unless a case names another loss, K in {1, 3, 8}.

Point counts {1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 511, 512, 513, 1025, 1537}: one wavefront with data and three
with none (which must still reach both barriers), every wavefront edge of both passes of a lane's two points, the chunk edge
and a ragged third chunk.

Bars (those of test_gpu_eval_poses.py): against ea_batch_eval at the same pose 1e-13 relative, against the CPU oracle 1e-11,
n_invalid exact; the exchange form against "poses_wave_exchange" = 0 on the same inputs 1e-13 (another fixed summation
order of the same terms); fp32 and "threads" = 1024 do not know the key: identical bits under both settings; the same call
twice, a pose alone or in company, every split over launches and both item orders: the same bits."""
import numpy as np
import pytest

from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu

FIELDS = ("cost", "JtJ", "Jtr", "n_invalid")
COUNTS = (1, 64, 65, 128, 129, 192, 193, 256, 257, 320, 511, 512, 513, 1025, 1537)
KS = (1, 3, 8)


def _rel(a, b):
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(np.abs(np.asarray(b)).max(), 1e-300)


def _same(a, b):
    return all(np.array_equal(a[f], b[f]) for f in FIELDS)


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


def _problem(hip, base, n, rng=None, dtype=None, loss=None, grid=None):
    X = base["xyz"][:n] if rng is None else base["xyz"][rng.choice(9000, n, replace=False)]
    P = hip.Problem(*base["K"], dtype=hip.EA_F64 if dtype is None else dtype)
    P.set_points(X.reshape(-1, 3)); P.set_dt_grid(base["grid"] if grid is None else grid)
    P.set_loss(*((hip.LOSS_CAUCHY, 0.7) if loss is None else loss))
    return P, X.reshape(-1, 3)


def _ran(B, want):
    assert B.info("poses_wave_exchange") == want, (B.info("poses_wave_exchange"), want)


def _against_eval(B, q, t, got, tol=1e-13):
    for k in range(q.shape[0]):
        ref = B.eval(q[k], t[k])
        for f in ("cost", "JtJ", "Jtr"):
            assert _rel(got[f][k], ref[f]) <= tol, (k, f, _rel(got[f][k], ref[f]))
        assert np.array_equal(got["n_invalid"][k], ref["n_invalid"]), k


def _against_oracle(O, X, q, t, got, i=0, tol=1e-11):
    for k in range(q.shape[0]):
        e = O.eval(X, q[k, i], t[k, i])
        assert abs(got["cost"][k, i] - e["cost"]) <= tol * abs(e["cost"]), k
        assert np.abs(got["JtJ"][k, i] - e["JtJ"]).max() <= tol * np.abs(e["JtJ"]).max(), k
        assert np.abs(got["Jtr"][k, i] - e["Jtr"]).max() <= tol * np.abs(e["Jtr"]).max(), k
        assert got["n_invalid"][k, i] == e["n_invalid"], k


@pytest.mark.parametrize("n", COUNTS)
def test_point_counts(hip, oracle, base, n):
    rng = np.random.default_rng(1000 + n)
    P, X = _problem(hip, base, n, rng)
    O = oracle.OracleProblem(base["grid"], *base["K"], loss=hip.LOSS_CAUCHY, loss_a=0.7)
    B = hip.Batch([P])
    try:
        for K in KS:
            q, t = _poses(rng, K, 1)
            got = B.eval_poses(q, t)
            _ran(B, 1)
            assert B.info("poses_tiles") == (n + 511) // 512 and B.info("poses_threads") == 256
            _against_eval(B, q, t, got)
            _against_oracle(O, X, q, t, got)
            B.set_tuning("poses_wave_exchange", 0)
            old = B.eval_poses(q, t)
            _ran(B, 0)
            B.set_tuning("poses_wave_exchange", 1)
            for f in ("cost", "JtJ", "Jtr"):
                assert _rel(got[f], old[f]) <= 1e-13, (K, f, _rel(got[f], old[f]))
            assert np.array_equal(got["n_invalid"], old["n_invalid"]), K
    finally:
        B.close(); P.close()


def test_setting_the_key_drops_resident_poses_and_info_reports_the_form(hip, base):
    rng = np.random.default_rng(7)
    P, _ = _problem(hip, base, 1537, rng)
    B = hip.Batch([P])
    try:
        q, t = _poses(rng, 3, 1)
        B.set_poses(q, t)
        B.eval_resident_poses()
        _ran(B, 1)
        for v in (0, 1, -1):
            B.set_tuning("poses_wave_exchange", v)
            with pytest.raises(hip.EAError) as ei:
                B.eval_resident_poses()
            assert ei.value.code == hip.EA_ERR_STATE
            B.set_poses(q, t)
            B.eval_resident_poses()
            _ran(B, 0 if v == 0 else 1)
    finally:
        B.close(); P.close()


@pytest.mark.parametrize("shape", ["fp32", "threads1024"])
def test_the_key_does_not_touch_fp32_and_1024_lane_launches(hip, base, shape):
    rng = np.random.default_rng(11)
    probs = [_problem(hip, base, n, rng, dtype=hip.EA_F32 if shape == "fp32" else hip.EA_F64)[0] for n in (1537, 513)]
    B = hip.Batch(probs)
    try:
        if shape == "threads1024":
            B.set_tuning("threads", 1024)
        q, t = _poses(rng, 3, 2)
        outs = []
        for v in (1, 0):
            B.set_tuning("poses_wave_exchange", v)
            outs.append(B.eval_poses(q, t))
            _ran(B, 0)
        assert _same(outs[0], outs[1])
    finally:
        B.close()
        for P in probs:
            P.close()


@pytest.mark.parametrize("loss_name,loss_a", [("LOSS_TRIVIAL", 1.0), ("LOSS_HUBER", 0.2), ("LOSS_CAUCHY", 0.7)])
@pytest.mark.parametrize("image", ["fp32_grid", "fp64_grid"])
def test_losses_image_forms_and_quaternions(hip, oracle, base, loss_name, loss_a, image):
    rng = np.random.default_rng(13)
    loss = getattr(hip, loss_name)
    # both image forms: a grid of doubles that are floats is read through its float32 mirror, any other as fp64
    grid = base["grid"].astype(np.float32).astype(np.float64) if image == "fp32_grid" else base["grid"] * (1.0 + 2.0 ** -40)
    P, X = _problem(hip, base, 1537, rng, loss=(loss, loss_a), grid=grid)
    O = oracle.OracleProblem(grid, *base["K"], loss=loss, loss_a=loss_a)
    B = hip.Batch([P])
    try:
        q, t = _poses(rng, 3, 1)
        q[1, 0] *= 1.02   # a non-unit quaternion: the general Jacobian
        got = B.eval_poses(q, t)
        _ran(B, 1)
        assert B.info("dt_f32") == (1 if image == "fp32_grid" else 0)
        _against_eval(B, q, t, got)
        _against_oracle(O, X, q, t, got)
        B.set_tuning("poses_wave_exchange", 0)
        old = B.eval_poses(q, t)
        _ran(B, 0)
        for f in ("cost", "JtJ", "Jtr"):
            assert _rel(got[f], old[f]) <= 1e-13, (f, _rel(got[f], old[f]))
        assert np.array_equal(got["n_invalid"], old["n_invalid"])
    finally:
        B.close(); P.close()


@pytest.mark.parametrize("n", [513, 1537])
def test_failed_functors(hip, base, n):
    P, X = _problem(hip, base, n)
    B = hip.Batch([P])
    try:
        zs = np.sort(X[:, 2])
        K = 3
        q = np.tile([1.0, 0, 0, 0], (K, 1, 1)); t = 0.002 * np.arange(K * 3, dtype=np.float64).reshape(K, 1, 3)
        t[1, 0] = [0.0, 0.0, -float(zs[n // 3])]   # part of the cloud inside the z guard
        got = B.eval_poses(q, t)
        _ran(B, 1)
        for k in range(K):
            assert got["n_invalid"][k, 0] == B.eval(q[k], t[k])["n_invalid"][0], k
        assert got["n_invalid"][1, 0] > 0
        B.set_tuning("poses_wave_exchange", 0)
        assert np.array_equal(B.eval_poses(q, t)["n_invalid"], got["n_invalid"])
    finally:
        B.close(); P.close()


def test_determinism(hip, base):
    rng = np.random.default_rng(17)
    probs = [_problem(hip, base, n, rng)[0] for n in (1537, 513)]
    B = hip.Batch(probs)
    try:
        K = 8
        q, t = _poses(rng, K, 2)
        first = B.eval_poses(q, t)
        _ran(B, 1)
        assert _same(B.eval_resident_poses(), first)          # the same call twice
        for k in range(K):                                    # a pose alone against the same pose in company
            one = B.eval_poses(q[k:k + 1], t[k:k + 1])
            assert all(np.array_equal(one[f][0], first[f][k]) for f in FIELDS), k
        for g in (1, 2, 3, 0):                                # every split over launches
            B.set_tuning("poses_per_launch", g)
            assert _same(B.eval_poses(q, t), first), g
        for order in (1, 0):                                  # both item orders of the work list
            B.set_tuning("poses_order", order)
            assert _same(B.eval_poses(q, t), first), order
        _ran(B, 1)
    finally:
        B.close()
        for P in probs:
            P.close()


def test_batches(hip, oracle, base):
    rng = np.random.default_rng(19)
    O = oracle.OracleProblem(base["grid"], *base["K"], loss=hip.LOSS_CAUCHY, loss_a=0.7)
    (A, XA), (C, XC) = _problem(hip, base, 700, rng), _problem(hip, base, 4097, rng)
    E, _ = _problem(hip, base, 0)
    try:
        B = hip.Batch([A, C])
        for K in KS:
            q, t = _poses(rng, K, 2)
            got = B.eval_poses(q, t)
            _ran(B, 1)
            _against_eval(B, q, t, got)
            _against_oracle(O, XA, q, t, got, i=0)
            _against_oracle(O, XC, q, t, got, i=1)
        B.close()
        B = hip.Batch([A, E, C])   # an empty problem: all-zero results at every pose
        for K in KS:
            q, t = _poses(rng, K, 3)
            got = B.eval_poses(q, t)
            _ran(B, 1)
            _against_eval(B, q, t, got)
            assert not got["cost"][:, 1].any() and not got["JtJ"][:, 1].any() and not got["Jtr"][:, 1].any() and not got["n_invalid"][:, 1].any()
        B.close()
    finally:
        A.close(); C.close(); E.close()
