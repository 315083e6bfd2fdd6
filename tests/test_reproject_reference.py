"""tests/reproject_ref.py -- the numpy restatement the device reprojection and overlay are held to bit for bit -- checked on
the CPU before tests/test_gpu_reproject.py relies on it:

(1) against a per-point Python loop that transcribes the four overloads of the reference's reproject
    (standalone/utils.cpp:497-592: b_X = b_T_a * a_X resp. the rig product times a_X, x / z, y / z, the distortion
    polynomial as upstream parenthesises it, K times the result), with the distortion coefficients taken BY NAME (the
    header's one deviation) and the rig product in the header's fixed order: the same bits, NaN and infinities included;
(2) inside_mask against oracle.ea_numpy.pixel_cost's count / outside on a bundled frame pair at three poses;
(3) matrix_to_pose(pose_to_matrix(q, t)) returns a unit q to 1e-15 through all four branches of Eigen's conversion."""
import os

import numpy as np
import pytest

import reproject_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (131.25, 179.5, 33.75, 21.5)
DIST = (0.11, -0.07, 0.013, -0.009, 0.021)    # k1, k2, p1, p2, k3
T12 = rr.pose_to_matrix([0.9998, 0.01, -0.012, 0.008], [0.11, -0.004, 0.006])


def _inv_rigid(T):
    R, t = T[:3, :3], T[:3, 3]
    out = np.eye(4)
    out[:3, :3] = R.T
    out[:3, 3] = -(R.T @ t)
    return out


T12INV = _inv_rigid(T12)


def _div(a, b):
    """IEEE division of Python floats (Python raises where C gives Inf / NaN)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _upstream_loop(xyz, b_T_a, K, dist, rig):
    """one point at a time, in Python floats, as the reference's loops run"""
    fx, fy, cx, cy = K
    if rig is None:
        T = np.asarray(b_T_a, dtype=np.float64)
    else:  # Eigen evaluates the chain of fixed-size 4x4 products first; the association is the header's
        T = rr.mul4(rr.mul4(rig[0], b_T_a), rig[1])
    T = [[float(T[r, c]) for c in range(4)] for r in range(4)]
    out = []
    for x, y, z in ((float(p[0]), float(p[1]), float(p[2])) for p in xyz):
        b = [((T[r][0] * x + T[r][1] * y) + T[r][2] * z) + T[r][3] * 1.0 for r in range(3)]
        xn, yn = _div(b[0], b[2]), _div(b[1], b[2])
        if dist is not None:
            k1, k2, p1, p2, k3 = dist
            r2 = xn * xn + yn * yn
            r4 = r2 * r2
            r6 = r4 * r2
            xd = xn * (1.0 + k1 * r2 + k2 * r4 + k3 * r6) + 2.0 * p1 * xn * yn + p2 * (r2 + 2.0 * xn * xn)
            yd = yn * (1.0 + k1 * r2 + k2 * r4 + k3 * r6) + 2.0 * p2 * xn * yn + p1 * (r2 + 2.0 * yn * yn)
            xn, yn = xd, yd
        out.append((fx * xn + cx, fy * yn + cy))     # K's zero entries contribute nothing
    return np.array(out, dtype=np.float64).reshape(-1, 2)


def _points(n, seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.4, 3.0, n)
    return np.stack([rng.uniform(-0.3, 0.3, n) * z, rng.uniform(-0.2, 0.2, n) * z, z], axis=1)


def _same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(a, b, equal_nan=True):
        return False
    inf = np.isinf(a)
    return bool(np.array_equal(np.signbit(a[inf]), np.signbit(b[inf])))


POSES = {
    "identity": np.eye(4),
    "rigid": rr.pose_to_matrix([0.995, 0.03, -0.05, 0.07], [0.05, -0.02, 0.1]),
    # the third row is (0, 0, 1, -1): points with z == 1 land on bz == 0 exactly, those with z < 1 behind the camera
    "degenerate": np.array([[1.0, 0, 0, 0.01], [0, 1.0, 0, -0.02], [0, 0, 1.0, -1.0], [0, 0, 0, 1.0]]),
}


@pytest.mark.parametrize("variant", ["plain", "distortion", "rig", "both"])
@pytest.mark.parametrize("pose", list(POSES))
def test_restatement_is_the_upstream_loop(variant, pose):
    xyz = _points(300, 5)
    xyz[::7, 2] = 1.0          # bz == 0 under "degenerate" (plain): +-Inf and, where bx is 0 too, NaN
    xyz[3] = (0.01, 0.02, 1.0)
    xyz[10] = (-0.01, 0.0, 1.0)
    dist = DIST if variant in ("distortion", "both") else None
    rig = (T12, T12INV) if variant in ("rig", "both") else None
    T = POSES[pose]
    M = rr.rig_matrix(T, T12, T12INV) if rig else rr.plain_matrix(T)
    got = rr.reproject(xyz, M, K, dist)
    want = _upstream_loop(xyz, T, K, dist, rig)
    assert got.shape == want.shape == (300, 2)
    assert _same_bits(got, want)
    if pose == "degenerate" and variant == "plain":
        assert np.isinf(got).any() and (~np.isfinite(got)).sum() >= 2 * 40
    if pose == "identity" and variant == "plain":
        assert np.isfinite(got).all()


def test_distortion_is_by_name_not_by_upstream_position():
    """upstream reads Kc as (k1, k2, k3, p1, p2); the restatement, like EAResidueEx, takes the names"""
    xyz = _points(50, 6)
    by_name = rr.reproject(xyz, np.eye(4), K, DIST)
    k1, k2, p1, p2, k3 = DIST
    by_position = rr.reproject(xyz, np.eye(4), K, (k1, k2, p2, k3, p1))   # what upstream would make of the same array
    assert not np.array_equal(by_name, by_position)


@pytest.fixture(scope="module")
def bundled_pair():
    from edge_alignment_amd import synth
    from oracle import preprocess_np as pp
    fr = synth.load_bundled_frames(os.path.join(ROOT, "tests", "golden", "rgbd"))
    a_X, _ = pp.get_aX(fr[1][0], fr[1][1], *synth.TUM_K)
    dt = pp.get_distance_transform(fr[2][0])
    return a_X[:3].T.copy(), dt, synth.TUM_K


@pytest.mark.parametrize("pose", [([1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0]),
                                  ([0.9987502603949663, 0.03, -0.03, 0.02829], [0.05, -0.03, 0.08]),
                                  ([0.9689124217106447, 0.0, 0.24740395925452294, 0.0], [0.4, 0.1, -0.3])],
                         ids=["identity", "small", "large"])
def test_inside_mask_counts_what_pixel_cost_counts(bundled_pair, pose):
    from oracle import ea_numpy as en
    xyz, dt, Kc = bundled_pair
    q = np.asarray(pose[0]) / np.linalg.norm(pose[0])
    t = np.asarray(pose[1])
    want = en.pixel_cost(xyz, q, t, *Kc, dt)
    uv = rr.reproject(xyz, rr.pose_to_matrix(q, t), Kc)
    ok = rr.inside_mask(uv, *dt.shape)
    assert int(ok.sum()) == want["count"] and int((~ok).sum()) == want["outside"]
    assert want["count"] > 1000 and want["count"] + want["outside"] == xyz.shape[0]
    if pose[1][0] != 0.0:
        assert want["outside"] > 0
    painted, stats = rr.overlay(np.full(dt.shape + (3,), 128, np.uint8), uv)
    assert stats == dict(n=xyz.shape[0], inside=want["count"], outside=want["outside"])
    red = (painted == np.array([0, 0, 255], np.uint8)).all(axis=2)
    assert 0 < int(red.sum()) <= want["count"] and (painted[~red] == 128).all()


BRANCHES = rr.branch_quaternions()


@pytest.mark.parametrize("branch", list(BRANCHES))
def test_round_trip_through_every_branch(branch):
    worst = 0.0
    for q in BRANCHES[branch]:
        t = np.array([0.25, -1.5, 3.0])
        m = rr.pose_to_matrix(q, t)
        tr = m[0, 0] + m[1, 1] + m[2, 2]
        if branch == "trace":
            assert tr > 0.0
        else:
            i = "xyz".index(branch)
            assert tr <= 0.0 and m[i, i] == max(m[0, 0], m[1, 1], m[2, 2])
        q2, t2 = rr.matrix_to_pose(m)
        worst = max(worst, float(np.abs(q2 - q).max()))
        assert np.array_equal(t2, t)
    print("branch", branch, "worst |q' - q| = %.3g" % worst)
    assert worst <= 1e-15


def test_matrix_to_pose_refuses_m33_not_one():
    m = np.eye(4)
    m[3, 3] = 2.0
    assert rr.matrix_to_pose(m) is None
