"""ea_problem_pose_stats / ea_batch_pose_stats against the numpy fp64 restatement of the header's definitions
(tests/pose_stats_ref.py): two small images x eight problem kinds (plain, weighted, distortion, second camera, both, and the
ROS knobs rot_transposed, z_eps = 0.001, no guard) x n in {1, 63, 64, 65, 257, 1000} (wave and workgroup tails, one workgroup
against several) x five poses (identity, a small motion, a pose that sends most points outside and some behind the camera, a
pose with a point inside the z guard, a camera moved forward so that points the identity does not see become visible) x
both dtypes.  The five counts exactly; sum_flow to the project's element-parity tolerances (1e-12 relative fp64, 1e-5 fp32),
exactly 0 at the identity; a batch of three gives every problem the bits of its own call; two runs give the same bits.

Every fixture meets, and the test asserts, the condition that no decision lies near its threshold: in the fp64 restatement
no u or v of a point in front of the camera within 1e-9 (fp64 problems) / 1e-3 (fp32) of a visibility bound, no visible |r|
within 1e-9 / 1e-4 of inlier_residual, no depth within 1e-9 / 1e-3 of 0 or of the guard.  The poses and thresholds are
searched for on the CPU (pose_stats_ref.settle); a fixture that misses the condition fails."""
import numpy as np
import pytest

import pose_stats_ref as ps

pytestmark = pytest.mark.gpu
RTOL = {"f64": 1e-12, "f32": 1e-5}
COUNTS = ("n", "n_invalid", "n_visible", "n_inlier", "n_flow")


@pytest.fixture(scope="module")
def images():
    return {name: ps.image(name) for name in ps.IMAGES}


@pytest.fixture(scope="module")
def cases():
    """every case of the file with its fp64 reference: computed once"""
    return ps.cases()


def _dtype(hip, name):
    return hip.EA_F64 if name == "f64" else hip.EA_F32


def _problem(hip, im, kind, n, dtype):
    dist, second, weighted, knobs = ps.KINDS[kind]
    P = hip.Problem(*im["K"], dtype=dtype)
    P.set_points(im["xyz"][:n])
    P.set_dt_grid(im["grid"])
    if dist:
        P.set_distortion(*ps.DIST)
    if second:
        P.set_second_camera(ps.T12)
    if weighted:
        P.set_weights(np.random.default_rng(n).uniform(0.1, 1.0, n))
    if knobs:
        P.set_flavour(**knobs)
    return P


def _bits(s):
    return tuple(s[k] for k in COUNTS) + (np.float64(s["sum_flow"]).view(np.uint64),)


def test_the_fixtures_cover_what_they_must(cases):
    """anti-vacuity, on the reference the device must match count for count"""
    st = [c["stats"] for c in cases]
    assert len(cases) == len(ps.IMAGES) * len(ps.KINDS) * len(ps.SIZES) * len(ps.POSES)
    assert sum(0 < s["n_visible"] < s["n"] for s in st) >= 1
    assert sum(s["n_inlier"] < s["n_visible"] for s in st) >= 1
    assert sum(s["n_invalid"] > 0 for s in st) >= 1
    assert sum(s["n_flow"] < s["n_visible"] for s in st) >= 1
    assert sum(s["n_visible"] == 0 for s in st) >= 1 and sum(0 < s["n_inlier"] for s in st) >= 1
    # the pose `far` sends a good share outside and some behind; `guard` has a point inside the guard where there is one
    for c in cases:
        assert ps.fixture_ok(c["slack"], "f32") and ps.fixture_ok(c["slack"], "f64"), (c["image"], c["kind"], c["n"], c["pose"], c["slack"])
        if c["pose"] == "guard" and c["kind"] != "no_guard":
            assert c["stats"]["n_invalid"] >= 1
        if c["pose"] == "far" and c["n"] >= 63:
            assert c["stats"]["n_visible"] < c["n"] // 2
        if c["pose"] == "identity":
            assert c["stats"]["sum_flow"] == 0.0 and c["stats"]["n_flow"] == c["stats"]["n_visible"]


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("iname", list(ps.IMAGES))
def test_against_the_restatement(hip, images, cases, iname, dtype_name):
    im = images[iname]
    worst = 0.0
    for kind in ps.KINDS:
        for n in ps.SIZES:
            P = _problem(hip, im, kind, n, _dtype(hip, dtype_name))
            for c in cases:
                if (c["image"], c["kind"], c["n"]) != (iname, kind, n):
                    continue
                assert ps.fixture_ok(c["slack"], dtype_name), (iname, kind, n, c["pose"], c["slack"])
                got = P.pose_stats(c["q"], c["t"], margin=c["margin"], inlier_residual=c["inlier_residual"])
                want = c["stats"]
                where = (iname, dtype_name, kind, n, c["pose"], got, want)
                for k in COUNTS:
                    assert got[k] == want[k], where
                if c["pose"] == "identity":
                    assert got["sum_flow"] == 0.0, where
                err = abs(got["sum_flow"] - want["sum_flow"])
                if want["sum_flow"] > 0.0:
                    worst = max(worst, err / want["sum_flow"])
                assert err <= RTOL[dtype_name] * want["sum_flow"], where
                assert _bits(P.pose_stats(c["q"], c["t"], margin=c["margin"], inlier_residual=c["inlier_residual"])) == _bits(got), where
            P.close()
    print(iname, dtype_name, "worst relative error of sum_flow %.3g" % worst)


def test_inf_threshold_counts_every_visible_point(hip, images, cases):
    im = images["37x70"]
    P = _problem(hip, im, "plain", 257, hip.EA_F64)
    c = [c for c in cases if (c["image"], c["kind"], c["n"], c["pose"]) == ("37x70", "plain", 257, "small")][0]
    s = P.pose_stats(c["q"], c["t"], margin=c["margin"])           # inlier_residual = +Inf
    assert s["n_inlier"] == s["n_visible"] == c["stats"]["n_visible"] > 0
    assert P.pose_stats(c["q"], c["t"], margin=10 ** 6)["n_visible"] == 0
    # weights, the loss and a prior do not enter
    base = _bits(P.pose_stats(c["q"], c["t"], margin=c["margin"], inlier_residual=c["inlier_residual"]))
    P.set_weights(np.random.default_rng(3).uniform(0.1, 1.0, 257))
    P.set_loss(hip.LOSS_HUBER, 0.05)
    P.set_normal_prior(1, np.eye(3), np.zeros(3))
    assert _bits(P.pose_stats(c["q"], c["t"], margin=c["margin"], inlier_residual=c["inlier_residual"])) == base
    P.close()


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_batch_gives_every_problem_the_bits_of_its_own_call(hip, images, cases, dtype_name):
    """three problems of different n (and kind, within what one batch takes) in one call; resident poses survive it"""
    im = images["37x70"]
    pick = [("plain", 1000, "forward"), ("distortion", 65, "small"), ("weighted", 257, "forward")]
    cs = [[c for c in cases if (c["image"], c["kind"], c["n"], c["pose"]) == ("37x70",) + p][0] for p in pick]
    Ps = [_problem(hip, im, kind, n, _dtype(hip, dtype_name)) for kind, n, _ in pick]
    q, t = np.array([c["q"] for c in cs]), np.array([c["t"] for c in cs])
    margin, thr = cs[0]["margin"], cs[0]["inlier_residual"]
    single = [P.pose_stats(q[i], t[i], margin=margin, inlier_residual=thr) for i, P in enumerate(Ps)]
    B = hip.Batch(Ps)
    B.set_poses(np.stack([q, q[::-1]]), np.stack([t, t[::-1]]))
    before = B.eval_resident_poses()
    got = B.pose_stats(q, t, margin=margin, inlier_residual=thr)
    again = B.pose_stats(q, t, margin=margin, inlier_residual=thr)
    after = B.eval_resident_poses()
    for key in ("cost", "JtJ", "Jtr"):
        assert np.array_equal(before[key].view(np.uint64), after[key].view(np.uint64)), key
    assert np.array_equal(before["n_invalid"], after["n_invalid"])
    for i in range(3):
        assert _bits(got[i]) == _bits(single[i]) == _bits(again[i]), (dtype_name, i, got[i], single[i])
        assert got[i]["n"] == pick[i][1] and got[i]["sum_flow"] > 0.0
    # the same problem beside other neighbours, in another slot
    B2 = hip.Batch([Ps[2], Ps[0]])
    got2 = B2.pose_stats(q[[2, 0]], t[[2, 0]], margin=margin, inlier_residual=thr)
    assert _bits(got2[0]) == _bits(single[2]) and _bits(got2[1]) == _bits(single[0])
    B2.close()
    B.close()
    for P in Ps:
        P.close()


def test_errors(hip, images):
    im = images["17x61"]
    P = hip.Problem(*im["K"], dtype=hip.EA_F64)
    with pytest.raises(hip.EAError) as ei:
        P.pose_stats(ps.IDENTITY_Q, ps.IDENTITY_T)     # no DT image, no points
    assert ei.value.code == hip.EA_ERR_STATE
    P.set_points(im["xyz"][:65])
    with pytest.raises(hip.EAError) as ei:
        P.pose_stats(ps.IDENTITY_Q, ps.IDENTITY_T)     # no DT image
    assert ei.value.code == hip.EA_ERR_STATE
    Q = hip.Problem(*im["K"], dtype=hip.EA_F64)
    Q.set_dt_grid(im["grid"])
    with pytest.raises(hip.EAError) as ei:
        Q.pose_stats(ps.IDENTITY_Q, ps.IDENTITY_T)     # no points
    assert ei.value.code == hip.EA_ERR_STATE
    P.set_dt_grid(im["grid"])
    for bad in (dict(margin=-1), dict(inlier_residual=-0.5), dict(inlier_residual=float("nan"))):
        with pytest.raises(hip.EAError) as ei:
            P.pose_stats(ps.IDENTITY_Q, ps.IDENTITY_T, **bad)
        assert ei.value.code == hip.EA_ERR_INVALID_ARG
    assert P.pose_stats(ps.IDENTITY_Q, ps.IDENTITY_T)["n"] == 65
    P.close(); Q.close()
