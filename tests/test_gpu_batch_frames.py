"""ea_batch_set_frames / Batch.set_frames: the Laplacian producers for every problem of a batch in one launch sequence, the
frame as blockIdx.z of each step.  The reference is always the per-problem producers (Problem.set_ref_frame +
Problem.set_now_frame) on fresh problems, compared with np.array_equal on get_points(), get_dt(), get_weights() and
num_points: bit equality, no tolerance.  oracle/preprocess_np.py is a second check on one bundled pair.

Shapes are the smallest at which the frame indexing can go wrong: (3, 3) all border; (37, 70) two 32-row column segments
with a 5-row tail, a width past one wavefront, 2590 pixels = two full 1024-pixel scan blocks and a partial one; (64, 257)
past the 256-lane row block (and the padded width past 256), exactly two segments.  Frames of one call differ in kind, so
that a frame reading its neighbour's workspace, minmax pair, counts or slot cannot go unnoticed."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "rgbd")
K = (525.0, 525.0, 319.5, 239.5)
SHAPES = ((3, 3), (37, 70), (64, 257))
KINDS = ("noise", "lines", "flat", "zero_depth", "sprinkled")


def _frame(kind, H, W, rng):
    """-> (bgr H x W x 3 uint8, depth H x W uint16) of one kind"""
    depth = rng.integers(400, 30000, (H, W)).astype(np.uint16)
    if kind == "flat":          # no edge: no point, the distances saturate and the normalisation degenerates
        return np.full((H, W, 3), 90, np.uint8), depth
    if kind == "lines":         # a few rasterised segments on grey
        from edge_alignment_amd import synth
        bgr = np.full((H, W, 3), 128, np.uint8)
        if min(H, W) >= 24:
            p0, p1 = synth.random_segments(H, W, 4, rng, min_len=6.0, max_len=0.6 * min(H, W))
            mask = synth.rasterize(H, W, p0, p1)
        else:
            mask = np.eye(H, W, dtype=bool)
        bgr[mask] = (255, 20, 200)
        return bgr, depth
    bgr = rng.integers(0, 256, (H, W, 3)).astype(np.uint8)   # dense noise: edges nearly everywhere
    if kind == "zero_depth":    # edges, but no pixel with a depth: zero points
        depth[:] = 0
    if kind == "sprinkled":
        depth[rng.random((H, W)) < 0.3] = 0
    return bgr, depth


def _pairs(H, W, n, seed, kinds=KINDS):
    rng = np.random.default_rng(seed)
    ref = [_frame(kinds[i % len(kinds)], H, W, rng) for i in range(n)]
    now = [_frame(kinds[(i + 1) % len(kinds)], H, W, rng)[0] for i in range(n)]
    return [r[0] for r in ref], [r[1] for r in ref], now


def _camera(i, H, W):
    """a camera of its own per problem"""
    return (0.9 * W + 7.0 * i, 0.8 * W + 3.0 * i, 0.5 * W - 0.5 + 0.25 * i, 0.5 * H - 0.5 - 0.125 * i)


def _problems(hip, n, H, W, dtype, weighting=None):
    probs = [hip.Problem(*_camera(i, H, W), dtype=dtype) for i in range(n)]
    for i, P in enumerate(probs):
        if weighting and weighting[i % len(weighting)]:
            P.set_depth_weighting(*weighting[i % len(weighting)])
    return probs


def _state(P, points=True, image=True):
    st = {}
    if points:
        st.update(n=P.num_points, points=P.get_points(), weights=P.get_weights())
    if image:
        st.update(dt=P.get_dt())
    return st


def _assert_same(got, want, where):
    assert sorted(got) == sorted(want), where
    for key in want:
        a, b = got[key], want[key]
        if key == "n":
            assert a == b, (where, key, a, b)
        elif a is None or b is None:
            assert a is None and b is None, (where, key)
        else:
            assert a.shape == b.shape and np.array_equal(a, b), (where, key, a.shape, b.shape)


def _per_problem(hip, probs, ref, dep, now, z_scaling=5000.0, ref_threshold=35, now_threshold=35, median=True, normalize=True):
    for i, P in enumerate(probs):
        if ref is not None:
            P.set_ref_frame(ref[i], dep[i], z_scaling=z_scaling, threshold=ref_threshold)
        if now is not None:
            P.set_now_frame(now[i], threshold=now_threshold, median=median, normalize=normalize)


def _close(*things):
    for t in things:
        for x in (t if isinstance(t, (list, tuple)) else [t]):
            x.close()


def _compare_call(hip, H, W, n, dtype, ref, dep, now, weighting=None, where=None, **kw):
    """one set_frames call on fresh problems against the per-problem producers on fresh problems -> the batched states"""
    want_p = _problems(hip, n, H, W, dtype, weighting)
    got_p = _problems(hip, n, H, W, dtype, weighting)
    batch = hip.Batch(got_p)
    try:
        _per_problem(hip, want_p, ref, dep, now, **kw)
        batch.set_frames(ref, dep, now, **kw)
        states = []
        for i in range(n):
            st = _state(got_p[i])
            _assert_same(st, _state(want_p[i]), (where, H, W, n, i))
            states.append(st)
        return states
    finally:
        _close(batch, want_p, got_p)


@pytest.mark.parametrize("dtype_name", ["EA_F64", "EA_F32"])
@pytest.mark.parametrize("n", [1, 2, 5])
@pytest.mark.parametrize("shape", SHAPES)
def test_shapes_counts_and_dtypes(hip, shape, n, dtype_name):
    H, W = shape
    ref, dep, now = _pairs(H, W, n, seed=100 * H + n)
    states = _compare_call(hip, H, W, n, getattr(hip, dtype_name), ref, dep, now, where=dtype_name)
    if min(shape) > 3:
        assert states[0]["n"] > 0.5 * H * W          # dense noise with depth everywhere: most pixels are points
    if n == 5:
        assert states[2]["n"] == 0 and states[3]["n"] == 0   # the flat frame, the frame without depth
        assert states[1]["dt"].max() == 0.0                  # (the flat current frame: the normalisation degenerates to 0)
        assert 0 < states[4]["n"] < states[0]["n"]


def test_a_frame_does_not_depend_on_its_neighbours_or_its_position(hip):
    """the five kinds in one call, then the same frames in another order: every problem still gets the per-problem bits, and a
    frame's image -- which no camera enters -- is the same wherever the frame stands"""
    H, W, n = 37, 70, 5
    ref, dep, now = _pairs(H, W, n, seed=7)
    first = _compare_call(hip, H, W, n, hip.EA_F64, ref, dep, now, where="order 0")
    for perm in ([4, 2, 0, 3, 1], [1, 0, 2, 4, 3]):
        got = _compare_call(hip, H, W, n, hip.EA_F64, [ref[k] for k in perm], [dep[k] for k in perm], [now[k] for k in perm],
                            where=("perm", perm))
        for i, k in enumerate(perm):
            assert np.array_equal(got[i]["dt"], first[k]["dt"]), (perm, i)
            assert got[i]["n"] == first[k]["n"], (perm, i)
            # z = depth / z_scaling does not depend on the camera either
            assert np.array_equal(got[i]["points"][:, 2], first[k]["points"][:, 2]), (perm, i)


@pytest.mark.parametrize("dtype_name", ["EA_F64", "EA_F32"])
@pytest.mark.parametrize("median,normalize", [(True, True), (True, False), (False, True), (False, False)])
def test_settings_cameras_and_depth_weighting_are_per_problem(hip, median, normalize, dtype_name):
    """depth weighting with powers 1 and 3 on some problems and off on others, the median and the normalisation on and off,
    different thresholds either side, z_scaling off its default"""
    H, W, n = 64, 257, 5
    ref, dep, now = _pairs(H, W, n, seed=11, kinds=("noise", "sprinkled", "lines"))
    weighting = [(2.0, 1), None, (3.5, 3)]
    states = _compare_call(hip, H, W, n, getattr(hip, dtype_name), ref, dep, now, weighting=weighting, where="settings",
                           z_scaling=4000.0, ref_threshold=20, now_threshold=50, median=median, normalize=normalize)
    assert states[0]["weights"] is not None and states[1]["weights"] is None and states[2]["weights"] is not None
    w = states[0]["weights"]
    assert (w > 0).all() and (w <= 1).all() and (w < 1).any() and (w == 1).any()   # both sides of the clamp at z_ref = 2


@pytest.fixture(scope="module")
def bundled(hip):
    """the five bundled frames at full size and at 160 x 120 (the library's own resize_half for colour, [::4, ::4] for depth)"""
    from edge_alignment_amd import synth
    full = synth.load_bundled_frames(G)
    small = {k: (hip.resize_half(hip.resize_half(bgr)), np.ascontiguousarray(dep[::4, ::4])) for k, (bgr, dep) in full.items()}
    return dict(full=full, small=small)


K_SMALL = (K[0] / 4, K[1] / 4, (K[2] + 0.5) / 4 - 0.5, (K[3] + 0.5) / 4 - 0.5)
FIVE_PAIRS = ((1, 2), (2, 3), (3, 4), (4, 5), (5, 1))
Q0, T0 = np.array([1.0, 0, 0, 0]), np.zeros(3)


def _small_batch(hip, bundled, batched, dtype=0):
    probs = [hip.Problem(*K_SMALL, dtype=dtype) for _ in FIVE_PAIRS]
    ref = [bundled["small"][a][0] for a, _ in FIVE_PAIRS]
    dep = [bundled["small"][a][1] for a, _ in FIVE_PAIRS]
    now = [bundled["small"][b][0] for _, b in FIVE_PAIRS]
    batch = hip.Batch(probs)
    if batched:
        batch.set_frames(ref, dep, now)
    else:
        _per_problem(hip, probs, ref, dep, now)
    return probs, batch, (ref, dep, now)


def _assert_same_eval(a, b, where):
    for key in ("cost", "JtJ", "Jtr", "n_invalid"):
        assert np.array_equal(a[key], b[key]), (where, key)


def test_eval_and_solve_after_set_frames_are_those_of_the_per_problem_producers(hip, bundled):
    n = len(FIVE_PAIRS)
    q, t = np.tile(Q0, (n, 1)), np.tile(T0, (n, 1))
    want_p, want_b, _ = _small_batch(hip, bundled, batched=False)
    got_p, got_b, _ = _small_batch(hip, bundled, batched=True)
    try:
        assert all(P.num_points > 500 for P in got_p)
        ev = got_b.eval(q, t)
        _assert_same_eval(ev, want_b.eval(q, t), "eval")
        assert (ev["cost"] > 0).all() and np.isfinite(ev["cost"]).all()
        gq, gt, gs = got_b.solve(q, t, max_num_iterations=12)
        wq, wt, ws = want_b.solve(q, t, max_num_iterations=12)
        assert np.array_equal(gq, wq) and np.array_equal(gt, wt)
        for a, b in zip(gs, ws):
            for key in ("termination", "why", "num_iterations", "initial_cost", "final_cost"):
                assert a[key] == b[key], key
        assert any(s["num_iterations"] > 1 for s in gs)
    finally:
        _close(want_b, got_b, want_p, got_p)


def test_one_side_at_a_time_another_extent_and_a_per_problem_call_afterwards(hip, bundled):
    n = len(FIVE_PAIRS)
    q, t = np.tile(Q0, (n, 1)), np.tile(T0, (n, 1))
    want_p, want_b, (ref, dep, now) = _small_batch(hip, bundled, batched=False)
    got_p = [hip.Problem(*K_SMALL) for _ in FIVE_PAIRS]
    got_b = hip.Batch(got_p)
    try:
        # only the reference frames: points as the per-problem call leaves them, still no image
        got_b.set_frames(ref_bgr=ref, ref_depth=dep)
        for i in range(n):
            _assert_same(_state(got_p[i], image=False), _state(want_p[i], image=False), ("ref only", i))
            with pytest.raises(hip.EAError) as ei:
                got_p[i].get_dt()
            assert ei.value.code == hip.EA_ERR_STATE
        # only the current frames: the points stay
        got_b.set_frames(now_bgr=now)
        for i in range(n):
            _assert_same(_state(got_p[i]), _state(want_p[i]), ("now only", i))
        _assert_same_eval(got_b.eval(q, t), want_b.eval(q, t), "after the two halves")
        # a larger extent, then the first one again: the workspace is laid out anew each time
        H2, W2 = 131, 200
        r2, d2, n2 = _pairs(H2, W2, n, seed=3)
        big_p = _problems(hip, n, H2, W2, hip.EA_F64)
        try:
            _per_problem(hip, big_p, r2, d2, n2)
            got_b.set_frames(r2, d2, n2)
            for i in range(n):
                want = _state(big_p[i])
                want["points"] = None  # (the cameras differ: of the points only the count and z are comparable)
                got = _state(got_p[i])
                assert np.array_equal(got["points"][:, 2], big_p[i].get_points()[:, 2]), i
                got["points"] = None
                _assert_same(got, want, ("larger extent", i))
        finally:
            _close(big_p)
        got_b.set_frames(ref, dep, now)
        for i in range(n):
            _assert_same(_state(got_p[i]), _state(want_p[i]), ("first extent again", i))
        # a per-problem producer call on one member afterwards: the batch sees that problem's new frame
        a, b = bundled["small"][5], bundled["small"][2]
        for P in (got_p[1], want_p[1]):
            P.set_ref_frame(a[0], a[1])
            P.set_now_frame(b[0])
        _assert_same(_state(got_p[1]), _state(want_p[1]), "member")
        _assert_same_eval(got_b.eval(q, t), want_b.eval(q, t), "after the member's own call")
    finally:
        _close(want_b, got_b, want_p, got_p)


def test_bundled_pairs_at_full_size_in_one_call(hip, bundled):
    """the 20 distinct pairs of the bundled frames 1..5 in one call"""
    from oracle import preprocess_np as pp
    full = bundled["full"]
    pairs = [(a, b) for a in range(1, 6) for b in range(1, 6) if a != b]
    ref, dep, now = [full[a][0] for a, _ in pairs], [full[a][1] for a, _ in pairs], [full[b][0] for _, b in pairs]
    got_p = [hip.Problem(*K) for _ in pairs]
    want_p = [hip.Problem(*K) for _ in range(5)]   # the reference of frame a / image of frame b, once per frame: same camera
    batch = hip.Batch(got_p)
    try:
        batch.set_frames(ref, dep, now)
        for k in range(1, 6):
            want_p[k - 1].set_ref_frame(*full[k])
            want_p[k - 1].set_now_frame(full[k][0])
        want = {k: _state(want_p[k - 1]) for k in range(1, 6)}
        assert want[1]["n"] == 44457
        for i, (a, b) in enumerate(pairs):
            got = _state(got_p[i])
            assert got["n"] == want[a]["n"], (a, b)
            assert np.array_equal(got["points"], want[a]["points"]), (a, b)
            assert got["weights"] is None
            assert np.array_equal(got["dt"], want[b]["dt"]), (a, b)
        # one pair against the numpy restatement of get_aX and of the get_distance_transform chain
        i = pairs.index((1, 3))
        aX, _ = pp.get_aX(full[1][0], full[1][1], *K)
        assert np.array_equal(got_p[i].get_points(), aX[:3].T)
        assert np.array_equal(got_p[i].get_dt(), pp.get_distance_transform(full[3][0]).astype(np.float64))
    finally:
        _close(batch, got_p, want_p)


def test_device_tensors_give_the_bits_of_the_host_entry(hip, bundled):
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch has no device")
    u16 = torch.uint16 if hasattr(torch, "uint16") else torch.int16
    want_p, want_b, (ref, dep, now) = _small_batch(hip, bundled, batched=True)
    got_p = [hip.Problem(*K_SMALL) for _ in FIVE_PAIRS]
    got_b = hip.Batch(got_p)
    try:
        dev = torch.device("cuda", 0)
        t_ref = torch.from_numpy(np.stack(ref)).to(dev)                          # one stacked tensor
        t_dep = [torch.from_numpy(d.view(np.int16)).to(dev).view(u16) for d in dep]   # a list of tensors
        t_now = torch.from_numpy(np.stack(now)).to(dev)
        got_b.set_frames(t_ref, t_dep, t_now)
        for i in range(len(FIVE_PAIRS)):
            _assert_same(_state(got_p[i]), _state(want_p[i]), ("device", i))
        assert torch.equal(t_ref.cpu(), torch.from_numpy(np.stack(ref)))         # read in place, not written
        with pytest.raises(ValueError):
            got_b.set_frames(t_ref, dep, t_now)                                  # a mix of host and device inputs
        with pytest.raises(ValueError):
            got_b.set_frames(now_bgr=t_now.permute(0, 2, 1, 3))                  # not contiguous
        with pytest.raises(ValueError):
            got_b.set_frames(now_bgr=t_now.cpu())                                # a torch tensor, but not on the GPU
    finally:
        _close(want_b, got_b, want_p, got_p)


def test_misuse_is_refused_and_leaves_every_problem_as_it_was(hip, bundled):
    import ctypes as C
    want_p, want_b, (ref, dep, now) = _small_batch(hip, bundled, batched=True)
    got_p, got_b, _ = _small_batch(hip, bundled, batched=True)
    n = len(FIVE_PAIRS)
    dup_b = hip.Batch([got_p[0], got_p[1], got_p[0]])
    L = hip.load()

    def refused(call):
        with pytest.raises(hip.EAError) as ei:
            call()
        assert ei.value.code == hip.EA_ERR_INVALID_ARG, ei.value
        for i in range(n):
            _assert_same(_state(got_p[i]), _state(want_p[i]), ("unchanged", i))

    try:
        other = [f[::-1].copy() for f in now]   # frames that would change every image if a refused call ran
        refused(lambda: got_b.set_frames(ref, dep, other[:2] + [None] + other[3:]))       # a NULL entry
        refused(lambda: got_b.set_frames(ref[:-1], dep[:-1], other[:-1]))                # a wrong count
        refused(lambda: got_b.set_frames(ref, dep, other + other[:1]))
        refused(lambda: dup_b.set_frames(ref[:3], dep[:3], other[:3]))                   # the same problem twice
        refused(lambda: got_b.set_frames(ref, dep, other, z_scaling=0.0))
        refused(lambda: got_b.set_frames(now_bgr=[f[:2].copy() for f in other]))         # an extent of 2
        refused(lambda: got_b.set_frames(now_bgr=[f[:, :2].copy() for f in other]))
        # host pointers handed to the device entry
        prm = hip.FrameParams()
        L.ea_default_frame_params(C.byref(prm), *other[0].shape[:2])
        ptrs = (C.c_void_p * n)(*[f.ctypes.data for f in other])
        refused(lambda: hip._check(L.ea_batch_set_frames_device(got_b._h, None, None, ptrs, C.byref(prm))))
        # both sides NULL; a reference colour frame without its depth
        refused(lambda: hip._check(L.ea_batch_set_frames(got_b._h, None, None, None, C.byref(prm))))
        refused(lambda: hip._check(L.ea_batch_set_frames(got_b._h, ptrs, None, None, C.byref(prm))))
        # and the batch still works
        got_b.set_frames(now_bgr=other)
        assert not np.array_equal(got_p[0].get_dt(), want_p[0].get_dt())
    finally:
        _close(dup_b, want_b, got_b, want_p, got_p)


# ---- anisotropic, off-centre cameras against the restatement ------------------------------------------------------------------
# Every other comparison of this file is device against device.  fx read for fy, or cx and cy handed over in the wrong order,
# would be the same mistake on both sides; the restatement takes the four intrinsics by name.
AXES_CAMERAS = ((61.0, 83.5, 38.25, 14.5), (70.25, 52.0, 30.5, 21.75))


def _held(xyz, dtype_name):
    """what a problem of that dtype holds of the restatement's doubles"""
    return xyz if dtype_name == "EA_F64" else xyz.astype(np.float32).astype(np.float64)


@pytest.mark.parametrize("dtype_name", ["EA_F64", "EA_F32"])
@pytest.mark.parametrize("shape", SHAPES[1:])
def test_a_camera_per_problem_against_the_restatement(hip, shape, dtype_name):
    """set_frames and set_ref_frame with two different cameras: each problem's points are oracle/preprocess_np.get_aX with
    ITS camera, bit for bit; the same camera with the focal lengths swapped gives other points on these frames"""
    from oracle import preprocess_np as pp
    H, W = shape
    ref, dep, now = _pairs(H, W, 2, seed=31 + H, kinds=("noise", "sprinkled"))
    dtype = getattr(hip, dtype_name)
    got_p = [hip.Problem(*Kc, dtype=dtype) for Kc in AXES_CAMERAS]
    one_p = [hip.Problem(*Kc, dtype=dtype) for Kc in AXES_CAMERAS]
    batch = hip.Batch(got_p)
    try:
        batch.set_frames(ref, dep, now)
        for i, Kc in enumerate(AXES_CAMERAS):
            one_p[i].set_ref_frame(ref[i], dep[i])
            want = _held(pp.get_aX(ref[i], dep[i], *Kc)[0][:3].T, dtype_name)
            assert got_p[i].num_points == one_p[i].num_points == want.shape[0] > 100, i
            assert np.array_equal(one_p[i].get_points(), want), ("set_ref_frame", i)
            assert np.array_equal(got_p[i].get_points(), want), ("set_frames", i)
            swapped = _held(pp.get_aX(ref[i], dep[i], Kc[1], Kc[0], Kc[2], Kc[3])[0][:3].T, dtype_name)
            assert not np.array_equal(swapped[:, 0], want[:, 0]) and not np.array_equal(swapped[:, 1], want[:, 1]), i
    finally:
        _close(batch, got_p, one_p)
