"""ea_resize_half_levels / resize_half_levels: the halving chain by itself -- a workgroup stages a tile of the frame in LDS,
halves it up to three times there and writes the levels that are kept -- against two references: ea_resize_half applied
repeatedly (bit for bit, NaN payloads included), and a numpy restatement (bit for bit but for the payload of a NaN) (integer (a + b + c + d + 2) >> 2 rounded to uint8 at every level for bgr8;
np.float32 ((a + b) + (c + d)) * 0.25 for float, NaN -> 0 on the first step only for kind 1).  The float frames hold NaN,
+-inf, negatives, denormals and quadruples whose ((a + b) + c) + d differs from (a + b) + (c + d) in the last bit.

Shapes: (40, 296) with 3 steps -- the 32 x 64 tile's edges in both directions, width * 3 no multiple of 256; (48, 304) with 4
steps -- a second launch continues from the third level; (8, 8) with 3 steps down to 1 x 1; (6, 10) with 1 step -- a width
that is no multiple of four, so the colour rows are fetched as bytes.  (skip, keep): first level only, all levels, a window,
one level behind levels that are only passed through, one behind a full launch of them, and for the 4-step shape one
behind a staged third level and a window across the two launches."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
SHAPES = (((40, 296), 3), ((48, 304), 4), ((8, 8), 3), ((6, 10), 1))
WINDOWS = ((0, 1), (0, 4), (1, 2), (2, 1), (3, 1), (4, 1), (2, 3))   # (the last two: the 4-step shape only)


def _bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype == np.float32:
        return a.shape == b.shape and b.dtype == np.float32 and np.array_equal(a.view(np.int32), b.view(np.int32))
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)


def _same(a, b):
    """against numpy: a NaN is a NaN whatever its payload (the host's and the device's adders differ there), every other
    value to the bit (signed zeros and denormals included)"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.dtype != np.float32:
        return _bits(a, b)
    both = np.isnan(a) & np.isnan(b)
    return a.shape == b.shape and b.dtype == np.float32 and np.array_equal(np.isnan(a), np.isnan(b)) and \
        np.array_equal(np.where(both, 0, a.view(np.int32)), np.where(both, 0, b.view(np.int32)))


def _np_half(img, nan_to_zero=False):
    """one step, restated"""
    if img.dtype == np.uint8:
        v = img.astype(np.int32)
        return ((v[0::2, 0::2] + v[0::2, 1::2] + v[1::2, 0::2] + v[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    v = img.copy()
    if nan_to_zero:
        v[v != v] = np.float32(0)
    with np.errstate(invalid="ignore", over="ignore"):
        top = (v[0::2, 0::2] + v[0::2, 1::2]).astype(np.float32)
        bot = (v[1::2, 0::2] + v[1::2, 1::2]).astype(np.float32)
        return ((top + bot).astype(np.float32) * np.float32(0.25)).astype(np.float32)


def _float_frame(H, W, rng):
    d = (rng.random((H, W)) * 4.0 + 0.4).astype(np.float32)
    r = rng.random((H, W))
    d[r < 0.05] = np.nan
    d[(r >= 0.05) & (r < 0.08)] = np.inf
    d[(r >= 0.08) & (r < 0.10)] = -np.inf
    d[(r >= 0.10) & (r < 0.20)] = -d[(r >= 0.10) & (r < 0.20)]
    d[(r >= 0.20) & (r < 0.25)] = np.float32(1e-41)             # denormal
    d[(r >= 0.25) & (r < 0.27)] = 0.0
    # a quadruple whose summation order shows in the last bit: (1 + 2^-24) + (2^-24 + 2^-24) != ((1 + 2^-24) + 2^-24) + 2^-24
    e = np.float32(2.0 ** -24)
    d[0:2, 0:2] = [[1.0, e], [e, e]]
    assert np.float32(np.float32(np.float32(1.0) + e) + np.float32(e + e)) != np.float32(np.float32(np.float32(np.float32(1.0) + e) + e) + e)
    return d


def _frames(H, W, seed):
    rng = np.random.default_rng(seed)
    return {0: rng.integers(0, 256, (H, W, 3)).astype(np.uint8), 1: _float_frame(H, W, rng), 2: _float_frame(H, W, rng)}


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("case", SHAPES, ids=lambda c: "%dx%d_s%d" % (c[0] + (c[1],)))
def test_every_level_is_the_repeated_single_step_and_the_numpy_restatement(hip, case, kind):
    (H, W), steps = case
    img = _frames(H, W, seed=H * W + steps)[kind]
    nz = kind == 1
    by_step, by_numpy = [img], [img]
    for k in range(steps):
        by_step.append(hip.resize_half(by_step[-1], nan_to_zero=nz and k == 0))
        by_numpy.append(_np_half(by_numpy[-1], nan_to_zero=nz and k == 0))
        assert _same(by_step[-1], by_numpy[-1]), ("the references disagree", k)
    ran = 0
    for skip, keep in WINDOWS:
        if skip + keep - 1 > steps:
            continue
        got = hip.resize_half_levels(img, skip=skip, keep=keep, nan_to_zero=nz)
        assert len(got) == keep
        for j, g in enumerate(got):
            assert g.shape[:2] == (H >> (skip + j), W >> (skip + j)), (skip, keep, j, g.shape)
            assert _bits(g, by_step[skip + j]), ("against ea_resize_half", skip, keep, j)
            assert _same(g, by_numpy[skip + j]), ("against numpy", skip, keep, j)
        ran += 1
    assert ran >= (1 if steps == 1 else 5)
    full = hip.resize_half_levels(img, skip=0, keep=steps + 1, nan_to_zero=nz)
    for k in range(steps + 1):
        assert _bits(full[k], by_step[k]), k
    if kind == 1:
        assert np.isnan(full[0]).any()                           # level 0 is the frame itself: NaN kept


def test_misuse(hip):
    img = np.zeros((8, 12, 3), np.uint8)
    for kw in (dict(skip=0, keep=4), dict(skip=3, keep=1), dict(skip=0, keep=0), dict(skip=-1, keep=1), dict(skip=5, keep=5)):
        with pytest.raises(hip.EAError) as ei:                   # 12 is not divisible by 8; keep < 1; skip < 0; more than 8 steps
            hip.resize_half_levels(img, **kw)
        assert ei.value.code == hip.EA_ERR_INVALID_ARG, kw
    import ctypes as C
    L = hip.load()
    out = np.zeros((4, 6, 3), np.uint8)
    ptrs = (C.c_void_p * 1)(out.ctypes.data)
    src = img.ctypes.data_as(C.c_void_p)
    assert L.ea_resize_half_levels(0, 0, None, 8, 12, 1, 1, ptrs) == hip.EA_ERR_INVALID_ARG
    assert L.ea_resize_half_levels(0, 0, src, 8, 12, 1, 1, None) == hip.EA_ERR_INVALID_ARG
    assert L.ea_resize_half_levels(0, 0, src, 8, 12, 1, 1, (C.c_void_p * 1)(None)) == hip.EA_ERR_INVALID_ARG
    assert L.ea_resize_half_levels(0, 7, src, 8, 12, 1, 1, ptrs) == hip.EA_ERR_INVALID_ARG
    assert L.ea_resize_half_levels(0, 0, src, 8, 12, 1, 1, ptrs) == hip.EA_OK
    assert not out.any()
