"""ea_*_reproject and ea_*_overlay on the device against tests/reproject_ref.py, the numpy restatement of the header's
arithmetic.  Exactness is the requirement: both sides run the same IEEE operations in the same order on the same matrix
and the same stored points (an fp32 problem: the floats it holds, read back with get_points), so every (u, v) has the same
bits -- NaN where the restatement has NaN, infinities of the same sign -- and every painted image the same bytes.

Shapes: n in {1, 63, 64, 65, 255, 256, 257, 513} (wavefront and workgroup edges, several workgroups) on a 5 x 7 image and
one 48 x 64 case; the four variants (plain, distortion, second camera, both); three matrices (identity, a general rigid
one, one whose third row (0, 0, 1, -1) puts the points with z == 1 at bz == 0 exactly and those with z < 1 behind the
camera); both dtypes."""
import os
import struct
import subprocess

import numpy as np
import pytest

import reproject_ref as rr
from edge_alignment_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SIZES = (1, 63, 64, 65, 255, 256, 257, 513)
SMALL = dict(H=5, W=7, K=(6.5, 5.25, 3.25, 2.5))
BIG = dict(H=48, W=64, K=(61.0, 57.5, 31.25, 24.5))
DIST = (0.11, -0.07, 0.013, -0.009, 0.021)            # k1, k2, p1, p2, k3
T12 = rr.pose_to_matrix([0.9998, 0.01, -0.012, 0.008], [0.11, -0.004, 0.006])
T12INV = np.linalg.inv(T12)
T12INV[3] = (0.0, 0.0, 0.0, 1.0)
T12_SHIFT = np.array([[1.0, 0, 0, 0.125], [0, 1.0, 0, -0.25], [0, 0, 1.0, 0.0], [0, 0, 0, 1.0]])   # exact in any order
T12_SHIFT_INV = np.array([[1.0, 0, 0, -0.125], [0, 1.0, 0, 0.25], [0, 0, 1.0, 0.0], [0, 0, 0, 1.0]])
VARIANTS = {"plain": (False, False), "distortion": (True, False), "rig": (False, True), "both": (True, True)}
MATRICES = {
    "identity": np.eye(4),
    "rigid": rr.pose_to_matrix([0.995, 0.03, -0.05, 0.07], [0.05, -0.02, 0.1]),
    # (the translations are powers of two: exact in an fp32 problem's points as well)
    "degenerate": np.array([[1.0, 0, 0, 0.015625], [0, 1.0, 0, -0.03125], [0, 0, 1.0, -1.0], [0, 0, 0, 1.0]]),
}


def _dtype(hip, name):
    return hip.EA_F64 if name == "f64" else hip.EA_F32


def _points(n, seed, im):
    """points that project inside and around the image at the identity; every seventh has z == 1 exactly, some z < 1"""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = im["K"]
    z = rng.uniform(0.5, 3.0, n)
    z[::7] = 1.0
    u = rng.uniform(-0.2 * im["W"], 1.2 * im["W"], n)
    v = rng.uniform(-0.2 * im["H"], 1.2 * im["H"], n)
    return np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], axis=1)


def _dt_image(im, seed=0):
    return np.random.default_rng(seed).uniform(0.0, 1.0, (im["H"], im["W"])).astype(np.float32)


def _problem(hip, im, variant, xyz, dtype, rig=(T12, T12INV), order=None):
    dist, second = VARIANTS[variant]
    P = hip.Problem(*im["K"], dtype=dtype)
    if order is not None:
        P.set_point_order(order)
    if xyz is not None and len(xyz):
        P.set_points(xyz)
    P.set_dt_grid(np.ascontiguousarray(_dt_image(im).astype(np.float64).T))
    if dist:
        P.set_distortion(*DIST)
    if second:
        P.set_second_camera(*rig)
    return P


def _want(P, im, variant, T, rig=(T12, T12INV), xyz=None):
    dist, second = VARIANTS[variant]
    M = rr.rig_matrix(T, *rig) if second else rr.plain_matrix(T)
    return rr.reproject(P.get_points() if xyz is None else xyz, M, im["K"], DIST if dist else None)


def _assert_same_bits(got, want, where):
    assert got.shape == want.shape, where
    assert np.array_equal(got, want, equal_nan=True), where + (np.flatnonzero((got != want) & ~(np.isnan(got) & np.isnan(want)))[:8],)
    inf = np.isinf(want)
    assert np.array_equal(np.signbit(got[inf]), np.signbit(want[inf])), where
    fin = np.isfinite(want)
    assert np.array_equal(got[fin].view(np.uint64), want[fin].view(np.uint64)), where     # (-0.0 against 0.0 too)


# ---- reprojection bits ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_reproject_bits(hip, variant, dtype_name):
    im = SMALL
    saw_inf = saw_nan = saw_behind = 0
    for n in SIZES:
        xyz = _points(n, 100 + n, im)
        if n >= 63:
            xyz[7] = (-0.015625, 0.03125, 1.0)      # with the degenerate matrix: bx == by == bz == 0, 0 / 0
        P = _problem(hip, im, variant, xyz, _dtype(hip, dtype_name))
        for name, T in MATRICES.items():
            got = P.reproject(T)
            want = _want(P, im, variant, T)
            _assert_same_bits(got, want, (variant, dtype_name, n, name))
            if name == "degenerate":
                saw_inf += int(np.isinf(want).sum())
                saw_nan += int(np.isnan(want).sum())
                saw_behind += int((P.get_points()[:, 2] < 1.0).sum())
            if name == "identity" and variant == "plain":
                assert np.isfinite(got).all()
        assert np.array_equal(P.reproject((np.array([1.0, 0, 0, 0]), np.zeros(3))), P.reproject(np.eye(4)))   # the (q, t) form
        P.close()
    assert saw_behind > 0
    if variant == "plain":
        assert saw_inf > 0 and saw_nan > 0      # bz == 0 exactly: +-Inf, and NaN where the numerator is 0 as well


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_reproject_bits_on_the_larger_image_and_the_exact_rig(hip, dtype_name):
    """48 x 64, every variant at 513 points; and a translation-only rig, whose product is exact: bz == 0 under the rig too"""
    for variant in VARIANTS:
        xyz = _points(513, 7, BIG)
        P = _problem(hip, BIG, variant, xyz, _dtype(hip, dtype_name))
        for name, T in MATRICES.items():
            _assert_same_bits(P.reproject(T), _want(P, BIG, variant, T), (variant, dtype_name, name))
        P.close()
    rig = (T12_SHIFT, T12_SHIFT_INV)
    for variant in ("rig", "both"):
        P = _problem(hip, SMALL, variant, _points(257, 9, SMALL), _dtype(hip, dtype_name), rig=rig)
        want = _want(P, SMALL, variant, MATRICES["degenerate"], rig=rig)
        assert np.isinf(want).any() or np.isnan(want).any()
        _assert_same_bits(P.reproject(MATRICES["degenerate"]), want, (variant, dtype_name, "exact rig"))
        P.close()


def test_reproject_ignores_what_reproject_does_not_have(hip):
    """weights, loss, prior, flavour knobs and the DT values do not enter; the distortion coefficients enter by name"""
    xyz = _points(257, 3, SMALL)
    P = _problem(hip, SMALL, "distortion", xyz, hip.EA_F64)
    T = MATRICES["rigid"]
    base = P.reproject(T)
    P.set_weights(np.random.default_rng(3).uniform(0.1, 1.0, 257))
    P.set_loss(hip.LOSS_HUBER, 0.05)
    P.set_normal_prior(1, np.eye(3), np.zeros(3))
    P.set_flavour(z_guard=0.0, z_eps=0.001, rot_transposed=True)
    _assert_same_bits(P.reproject(T), base, ("knobs",))
    k1, k2, p1, p2, k3 = DIST
    P.set_distortion(k1, k2, p2, k3, p1)       # upstream's positional reading of the same array: another result
    assert not np.array_equal(P.reproject(T), base)
    P.close()


# ---- batch forms ------------------------------------------------------------------------------------------------------------

@pytest.fixture()
def five(hip, request):
    """five problems of different n: a plain one that carries a rig TERM, one without points, a distorted one, a
    second-camera one, a plain one"""
    dtype = _dtype(hip, getattr(request, "param", "f64"))
    im = SMALL
    term = _problem(hip, im, "rig", _points(63, 21, im), dtype)
    Ps = [_problem(hip, im, "plain", _points(257, 22, im), dtype),
          _problem(hip, im, "plain", None, dtype),
          _problem(hip, im, "distortion", _points(65, 23, im), dtype),
          _problem(hip, im, "rig", _points(255, 24, im), dtype),
          _problem(hip, im, "plain", _points(513, 25, im), dtype)]
    Ps[0].add_term(term)
    kinds = ["plain", "plain", "distortion", "rig", "plain"]
    Ts = np.stack([MATRICES["rigid"], MATRICES["identity"], MATRICES["degenerate"], MATRICES["rigid"], MATRICES["degenerate"]])
    B = hip.Batch(Ps)
    yield dict(Ps=Ps, term=term, kinds=kinds, Ts=Ts, B=B, im=im)
    B.close()
    Ps[0].clear_terms()
    for P in Ps + [term]:
        P.close()


@pytest.mark.parametrize("five", ["f64", "f32"], indirect=True)
def test_batch_forms_give_the_single_problem_bits(hip, five):
    import torch
    Ps, B, Ts, kinds, im = five["Ps"], five["B"], five["Ts"], five["kinds"], five["im"]
    off = B.row_offsets()
    assert list(off) == [0, 257 + 63, 320, 385, 640, 1153]
    sentinel = 7.25
    uv = B.reproject(Ts, out=np.full((int(off[-1]), 2), sentinel))
    dev = torch.full((int(off[-1]), 2), sentinel, dtype=torch.float64, device="cuda")
    B.reproject_device(Ts, dev)
    assert np.array_equal(dev.cpu().numpy().view(np.uint64), uv.view(np.uint64))
    for i, P in enumerate(Ps):
        n = P.num_points
        rows = uv[off[i]:off[i] + n]
        if n:
            single = P.reproject(Ts[i])
            _assert_same_bits(rows, single, ("batch", i))
            _assert_same_bits(single, _want(P, im, kinds[i], Ts[i]), ("single", i))
    assert (uv[257:320] == sentinel).all()                   # the rows of problem 0's term are left alone
    # the term by itself: call it on the term
    _assert_same_bits(five["term"].reproject(Ts[0]), _want(five["term"], im, "rig", Ts[0]), ("term",))
    # a (q, t) tuple per problem is accepted
    qt = [(np.array([1.0, 0, 0, 0]), np.zeros(3))] * 5
    assert np.array_equal(B.reproject(qt), B.reproject(np.stack([np.eye(4)] * 5)), equal_nan=True)
    # capacity and argument errors, with a real batch
    with pytest.raises(hip.EAError) as ei:
        B.reproject(Ts, out=np.zeros((int(off[-1]) - 1, 2)))
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    bad = Ts.copy()
    bad[3, 3, 3] = 2.0
    with pytest.raises(hip.EAError) as ei:
        B.reproject(bad)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    bad = Ts.copy()
    bad[4, 0, 0] = float("nan")
    with pytest.raises(hip.EAError) as ei:
        B.overlay(bad, [np.zeros((im["H"], im["W"], 3), np.uint8)] * 5)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG


def test_resident_poses_survive_reproject_and_overlay(hip):
    im = SMALL
    kinds = ["plain", "distortion", "plain"]
    Ps = [_problem(hip, im, k, _points(n, 30 + n, im), hip.EA_F64) for k, n in zip(kinds, (257, 65, 513))]
    Ts = np.stack([MATRICES["rigid"], MATRICES["degenerate"], MATRICES["identity"]])
    B = hip.Batch(Ps)
    q0 = np.array([0.999, 0.02, -0.03, 0.01])
    q = np.tile(q0 / np.linalg.norm(q0), (2, 3, 1))
    t = np.zeros((2, 3, 3))
    t[1, :, 0] = 0.05
    B.set_poses(q, t)
    before = B.eval_resident_poses()
    uv = B.reproject(Ts)
    _, stats = B.overlay(Ts, [np.zeros((im["H"], im["W"], 3), np.uint8) for _ in Ps])
    after = B.eval_resident_poses()
    for key in ("cost", "JtJ", "Jtr"):
        assert np.array_equal(before[key].view(np.uint64), after[key].view(np.uint64)), key
    assert np.array_equal(before["n_invalid"], after["n_invalid"])
    assert uv.shape == (257 + 65 + 513, 2) and [s["n"] for s in stats] == [257, 65, 513]
    B.close()
    for P in Ps:
        P.close()


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_point_order_single_gives_the_callers_order_batch_the_storage_order(hip, dtype_name):
    im = BIG
    rng = np.random.default_rng(41)
    n = 513
    z = rng.uniform(0.5, 3.0, n)
    u, v = rng.uniform(1.0, im["W"] - 1.0, n), rng.uniform(1.0, im["H"] - 1.0, n)     # inside at the identity: the tiles are plain
    fx, fy, cx, cy = im["K"]
    xyz = np.stack([(u - cx) * z / fx, (v - cy) * z / fy, z], axis=1)
    P = _problem(hip, im, "plain", xyz, _dtype(hip, dtype_name), order=4)
    assert P.point_order == 4
    T = MATRICES["rigid"]
    single = P.reproject(T)
    _assert_same_bits(single, _want(P, im, "plain", T), ("caller's order",))           # get_points: the caller's order too
    B = hip.Batch([P])
    stored = B.reproject(T[None])
    keys = {row.tobytes(): i for i, row in enumerate(single)}
    assert len(keys) == n
    perm = np.array([keys[row.tobytes()] for row in stored])          # stored row k is the caller's point perm[k]
    assert sorted(perm) == list(range(n)) and not np.array_equal(perm, np.arange(n))
    # storage order = tiles of 4 px of the identity projection in raster order, the caller's order inside a tile
    # (from the caller's doubles, as ea_problem_set_points sees them)
    u0, v0 = fx * xyz[:, 0] / xyz[:, 2] + cx, fy * xyz[:, 1] / xyz[:, 2] + cy
    tile = (np.floor(v0 / 4).astype(int) * 4096 + np.floor(u0 / 4).astype(int))[perm]
    assert len(set(tile)) > 20
    assert (np.diff(tile) >= 0).all()
    assert all(perm[k] < perm[k + 1] for k in range(n - 1) if tile[k] == tile[k + 1])
    B.close()
    P.close()


# ---- overlay ----------------------------------------------------------------------------------------------------------------

PLANT = dict(H=5, W=7, K=(4.0, 4.0, 3.5, 2.5))      # powers of two: u = 4 x + 3.5 is exact for the planted x


def _planted(n, seed):
    """(xyz, what the first points are): u in (-1, 0), u = W - 2^-40, u = W, v = -1, v in (-1, 0), NaN, +Inf, -Inf, two points
    on one pixel; then random filler"""
    fx, fy, cx, cy = PLANT["K"]
    W = PLANT["W"]
    uv = [(-0.5, 1.0), (W - 2.0 ** -40, 2.0), (float(W), 2.0), (3.0, -1.0), (3.0, -0.25), (2.25, 3.5), (2.75, 3.25)]
    pts = [((u - cx) / fx, (v - cy) / fy, 1.0) for u, v in uv]
    pts += [(0.0, 0.0, 0.0), (1.0, 0.25, 0.0), (-1.0, 0.25, 0.0)]     # 0 / 0, +x / 0, -x / 0
    xyz = np.array(pts)
    if n > len(pts):
        xyz = np.concatenate([xyz, _points(n - len(pts), seed, PLANT)])
    return xyz[:n], np.array(uv)


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
@pytest.mark.parametrize("n", [10, 65, 257])
def test_overlay_planted_points(hip, n, dtype_name):
    im = PLANT
    xyz, planted = _planted(n, 50 + n)
    P = _problem(hip, im, "plain", xyz, _dtype(hip, dtype_name))
    uv = P.reproject(np.eye(4))
    _assert_same_bits(uv, rr.reproject(P.get_points(), np.eye(4), im["K"]), ("planted", n))
    if dtype_name == "f64":     # the planted values arrive exactly (an fp32 problem rounds x first: u = W - 2^-40 becomes W)
        assert np.array_equal(uv[:7], planted)
        assert uv[1, 0] < im["W"] and int(uv[1, 0]) == im["W"] - 1
    assert np.isnan(uv[7]).all() and uv[8, 0] == np.inf and uv[9, 0] == -np.inf
    background = np.random.default_rng(n).integers(0, 255, (im["H"], im["W"], 3)).astype(np.uint8)    # (255 is the paint)
    got, stats = P.overlay(np.eye(4), background)
    want, want_stats = rr.overlay(background, uv)
    assert np.array_equal(got, want) and stats == want_stats, (stats, want_stats)
    assert stats["inside"] == int(rr.inside_mask(uv, im["H"], im["W"]).sum()) and stats["inside"] + stats["outside"] == stats["n"] == n
    red = np.array([0, 0, 255], np.uint8)
    assert (got[1, 0] == red).all()                               # u in (-1, 0) paints column 0
    assert (got[0, 3] == red).all()                               # v in (-1, 0) paints row 0
    assert (got[3, 2] == red).all()                               # the shared pixel
    if dtype_name == "f64" and n == 10:
        assert (got[2, im["W"] - 1] == red).all()                 # u = W - 2^-40
        assert stats == dict(n=10, inside=5, outside=5)           # u = W, v = -1, NaN, +Inf, -Inf are outside
        touched = np.zeros((im["H"], im["W"]), bool)
        touched[[1, 0, 3, 2], [0, 3, 2, im["W"] - 1]] = True
        assert np.array_equal(got[~touched], background[~touched])     # every untouched byte is unchanged
    # a custom colour, in place, and the same bytes on a second run
    img = background.copy()
    out, st2 = P.overlay(np.eye(4), img, color=(17, 200, 3), out=img)
    assert out is img and st2 == stats
    assert np.array_equal(img, rr.overlay(background, uv, (17, 200, 3))[0])
    assert np.array_equal(P.overlay(np.eye(4), background)[0], got)
    # an extent mismatch is refused and leaves the image alone
    wrong = np.full((im["H"] + 1, im["W"], 3), 9, np.uint8)
    out = np.full_like(wrong, 77)
    with pytest.raises(hip.EAError) as ei:
        P.overlay(np.eye(4), wrong, out=out)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG and (out == 77).all() and (wrong == 9).all()
    P.close()


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_overlay_every_variant_and_size(hip, dtype_name):
    for variant in VARIANTS:
        for n in SIZES:
            P = _problem(hip, SMALL, variant, _points(n, 300 + n, SMALL), _dtype(hip, dtype_name))
            for name, T in MATRICES.items():
                background = np.full((SMALL["H"], SMALL["W"], 3), 128, np.uint8)
                got, stats = P.overlay(T, background)
                want, want_stats = rr.overlay(background, _want(P, SMALL, variant, T))
                assert np.array_equal(got, want) and stats == want_stats, (variant, n, name, stats, want_stats)
            P.close()


@pytest.mark.parametrize("dtype_name", ["f64", "f32"])
def test_overlay_counts_are_pixel_costs_counts(hip, dtype_name):
    """plain problem, (q, t) input of a unit q: inside / outside = ea_problem_pixel_cost's count / outside"""
    im = BIG
    P = _problem(hip, im, "plain", _points(513, 61, im), _dtype(hip, dtype_name))
    background = np.zeros((im["H"], im["W"], 3), np.uint8)
    for axis, deg, t in (([1, 0, 0], 0.0, (0.0, 0.0, 0.0)), ([1, 2, 3], 2.0, (0.05, -0.02, 0.1)), ([0, 1, 0], 25.0, (0.4, 0.1, -0.3))):
        q = synth.quat_from_axis_angle(axis, np.deg2rad(deg))
        pc = P.pixel_cost(q, t)
        painted, stats = P.overlay((q, np.asarray(t)), background)
        assert (stats["inside"], stats["outside"]) == (pc["count"], pc["outside"]) and stats["n"] == 513
        assert pc["count"] + pc["outside"] == 513 and (deg > 10.0 or 0 < pc["count"] < 513)
        _, ref_stats = rr.overlay(background, rr.reproject(P.get_points(), rr.pose_to_matrix(q, t), im["K"]))
        assert ref_stats == stats
    P.close()


@pytest.mark.parametrize("five", ["f64", "f32"], indirect=True)
def test_overlay_device_paints_tensors_in_place_and_matches_the_host_form(hip, five):
    import torch
    Ps, B, Ts, kinds, im = five["Ps"], five["B"], five["Ts"], five["kinds"], five["im"]
    rng = np.random.default_rng(77)
    backgrounds = [rng.integers(0, 255, (im["H"], im["W"], 3)).astype(np.uint8) for _ in Ps]
    host, host_stats = B.overlay(Ts, backgrounds, color=(9, 8, 250))
    tensors = [torch.from_numpy(b.copy()).cuda() for b in backgrounds]
    dev_stats = B.overlay_device(Ts, tensors, color=(9, 8, 250))
    assert dev_stats == host_stats
    for i, P in enumerate(Ps):
        assert np.array_equal(tensors[i].cpu().numpy(), host[i]), i
        if P.num_points:
            want, want_stats = rr.overlay(backgrounds[i], _want(P, im, kinds[i], Ts[i]), (9, 8, 250))
            single, single_stats = P.overlay(Ts[i], backgrounds[i], color=(9, 8, 250))
            assert np.array_equal(host[i], want) and np.array_equal(single, want) and host_stats[i] == want_stats == single_stats, i
        else:
            assert np.array_equal(host[i], backgrounds[i]) and host_stats[i] == dict(n=0, inside=0, outside=0)
    assert host_stats[0]["n"] == 257                      # the head family, not its term
    # in place on the host, too
    imgs = [b.copy() for b in backgrounds]
    outs, st = B.overlay(Ts, imgs, color=(9, 8, 250), in_place=True)
    assert all(o is i for o, i in zip(outs, imgs)) and st == host_stats
    assert all(np.array_equal(a, b) for a, b in zip(imgs, host))
    # host memory handed to the device form, a NULL entry and an extent mismatch are refused; nothing is painted
    with pytest.raises(hip.EAError) as ei:
        B.overlay_device(Ts, [b.ctypes.data for b in imgs], height=im["H"], width=im["W"])
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    with pytest.raises(hip.EAError) as ei:
        B.overlay_device(Ts, [t.data_ptr() for t in tensors[:4]] + [0], height=im["H"], width=im["W"])
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    keep = [t.clone() for t in tensors]
    with pytest.raises(hip.EAError) as ei:
        B.overlay_device(Ts, [t.data_ptr() for t in tensors], height=im["H"], width=im["W"] + 1)
    assert ei.value.code == hip.EA_ERR_INVALID_ARG
    assert all(torch.equal(a, b) for a, b in zip(keep, tensors))


def test_errors(hip):
    im = SMALL
    P = hip.Problem(*im["K"], dtype=hip.EA_F64)
    img = np.zeros((im["H"], im["W"], 3), np.uint8)
    # no DT image / no points: EA_ERR_STATE, as ea_eval.  (Without points the stub's own output array is empty.)
    P.set_points(_points(65, 1, im))
    for call in (lambda: P.reproject(np.eye(4)), lambda: P.overlay(np.eye(4), img)):
        with pytest.raises(hip.EAError) as ei:
            call()
        assert ei.value.code == hip.EA_ERR_STATE
    Q = _problem(hip, im, "plain", None, hip.EA_F64)
    for call in (lambda: Q.reproject(np.eye(4)), lambda: Q.overlay(np.eye(4), img)):
        with pytest.raises(hip.EAError) as ei:
            call()
        assert ei.value.code == hip.EA_ERR_STATE
    P.set_dt_grid(np.zeros((im["W"], im["H"])))
    bad = np.eye(4)
    bad[3, 2] = 1e-9
    for call in (lambda: P.reproject(bad), lambda: P.overlay(bad, img)):
        with pytest.raises(hip.EAError) as ei:
            call()
        assert ei.value.code == hip.EA_ERR_INVALID_ARG
    import ctypes as C
    uv = np.zeros((64, 2))
    rc = hip.load().ea_problem_reproject(P.handle, np.eye(4).ctypes.data_as(C.POINTER(C.c_double)),
                                         uv.ctypes.data_as(C.POINTER(C.c_double)), 64)       # capacity 64 < 65
    assert rc == hip.EA_ERR_INVALID_ARG and not uv.any()
    assert P.reproject(np.eye(4)).shape == (65, 2)
    P.close(); Q.close()


# ---- the example ------------------------------------------------------------------------------------------------------------

def test_overlay_demo(hip, tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "overlay_demo"])
    pr = synth.make_problem(60, 80, 1500, 20, 1, 65.0, 65.0, 39.5, 29.5,
                            planted_q=synth.quat_from_axis_angle([1, 2, 3], np.deg2rad(1.0)), planted_t=(0.01, -0.005, 0.02),
                            normalize=True)
    path = str(tmp_path / "pair.bin")
    W, H = pr["grid"].shape
    n = pr["xyz"].shape[0]
    with open(path, "wb") as f:
        f.write(struct.pack("<iii", n, H, W))
        f.write(struct.pack("<dddd", *pr["K"]))
        f.write(np.ascontiguousarray(np.concatenate([pr["xyz"], np.ones((n, 1))], axis=1), dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(pr["grid"], dtype=np.float64).tobytes())
    before, after = str(tmp_path / "initial.ppm"), str(tmp_path / "final.ppm")
    out = subprocess.run([os.path.join(ROOT, "examples", "overlay_demo"), path, before, after], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [ln.split() for ln in out.stdout.strip().splitlines()]
    assert [ln[0] for ln in lines] == ["initial", "final", "pose"]
    images = []
    for ln, ppm in zip(lines[:2], (before, after)):
        inside, outside, total, count, pc_outside = int(ln[1]), int(ln[2]), int(ln[3]), int(ln[5]), int(ln[6])
        assert ln[4] == "|" and inside == count and outside == pc_outside and inside + outside == total == n
        raw = open(ppm, "rb").read()
        header = b"P6\n%d %d\n255\n" % (W, H)
        assert raw.startswith(header) and len(raw) == len(header) + H * W * 3
        img = np.frombuffer(raw[len(header):], np.uint8).reshape(H, W, 3)
        red = (img == np.array([255, 0, 0], np.uint8)).all(axis=2)         # PPM is RGB
        assert 0 < int(red.sum()) <= inside and (img[~red] == 128).all()
        images.append(img)
    assert not np.array_equal(images[0], images[1])
    assert float(lines[1][7]) < float(lines[0][7])           # the alignment landed: the integer-pixel cost went down
    assert int(lines[2][8]) == 0
