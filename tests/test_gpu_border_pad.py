"""The three kernels that write the replicated border of the image copy, checked through evaluations that land on it.

ea_problem_get_dt returns the interior only, so the pad written by ea_pad_image_kernel (set_dt_image_device) and by
ea_dt_store_kernel (the frame producers set_now_frame / _canny / _ros) is visible to nothing but a stencil that reaches
into it.  Here the same border-band cloud (tests/border_band.py) is evaluated after every way an image can arrive:

  * set_dt_grid (transposing upload, 32-texel tiles) and set_dt_image_device (a torch tensor, row-major) of the same
    texels, on every shape: both against the extended-precision reference, and bit-identical to each other;
  * each frame producer on crops of a bundled frame -- the full 480 x 640 frame, and odd sizes either side of the
    producers' small-frame path and of the upload's tile and pitch boundaries -- where the reference takes
    Problem.get_dt() as the image.  What the producers compute inside the image is test_gpu_preprocess.py's business;
    this pins the border they replicate around it;
  * raw-buffer and flat addressing both read the pad; per-point rows and fused sums are compared.

Tolerances: border_band.tolerances (the project's bounds, or 4x the deviation of plain arithmetic of the same precision
from the reference where that is larger); fp32 row by row."""
import os

import numpy as np
import pytest

import border_band as bb

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W, top, left) crops of the bundled frame, each with edges in it: whole, tall, wide, and small ones (64 x 64 is
# the first size on the producers' large-frame path)
CROPS = ((480, 640, 0, 0), (160, 120, 200, 300), (33, 257, 150, 100), (59, 43, 133, 142), (27, 41, 447, 135),
         (64, 64, 200, 300), (5, 3, 88, 631))
POSES = (bb.POSES[0], bb.POSES[2])


def _frame():
    from oracle import preprocess_np as pp
    return pp.load_rgb_as_bgr(os.path.join(ROOT, "tests", "golden", "rgbd", "rgb_1.png"))


def _check(hip, c, poses):
    """per-point rows, materialised rows and fused sums (raw-buffer and flat addressing) of a case against the reference
    -> (everything the kernels returned, largest deviation of r)"""
    B = hip.Batch([c.P])
    out, seen = [], {}
    try:
        for pi, pose in enumerate(poses):
            loss = bb.LOSSES[pi % 3]
            c.P.set_loss(*loss)
            c.raw(pose)   # (asserts the workload)
            r, J = c.P.eval_points(*pose, corrected=True)
            c.check_rows(r, J, pose, loss, True, ("eval_points", pi), seen)
            rr, JJ, bad = B.eval_rows(*pose, corrected=False, layout=0)
            assert bad == 0
            c.check_rows(rr, JJ, pose, loss, False, ("eval_rows", pi), seen)
            out += [r, J, rr, JJ]
            for buf in (1, 0):
                B.set_tuning("buffer_loads", buf)
                g = B.eval(*pose)
                assert B.info("buffer_loads") == buf
                c.check_sums(g, pose, loss, ("eval", pi, buf), seen)
                out += [g["cost"], g["JtJ"], g["Jtr"]]
    finally:
        B.close()
    return out, seen


@pytest.mark.parametrize("dtype_name", ["EA_F64", "EA_F32"])
def test_grid_upload_and_device_image_upload_agree_on_the_band(hip, dtype_name):
    dtype = getattr(hip, dtype_name)
    for (H, W), kind in [(s, "noise") for s in bb.SHAPES] + [(s, "dt") for s in bb.CORE_SHAPES]:
        results = []
        for way in ("grid", "device image"):
            c = bb.make_case(hip, H, W, kind, dtype, upload=way)   # (None: refused with an error, small images only)
            if c is None:
                results.append(None)
                continue
            try:
                assert np.array_equal(c.P.get_dt(), c.pr["image"]), (H, W, way)
                results.append(_check(hip, c, bb.POSES)[0])
            finally:
                c.close()
        a, b = results
        assert (a is None) == (b is None), (H, W)
        if a is not None:   # the two uploads build the same padded copy: the same bits out of every kernel
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (H, W, kind)


@pytest.mark.parametrize("producer", ["now_frame", "now_frame_canny", "now_frame_ros"])
@pytest.mark.parametrize("dtype_name", ["EA_F64", "EA_F32"])
def test_frame_producers_replicate_the_border(hip, dtype_name, producer):
    dtype = getattr(hip, dtype_name)
    frame = _frame()
    assert frame.shape == (480, 640, 3)
    for H, W, top, left in CROPS:
        crop = np.ascontiguousarray(frame[top:top + H, left:left + W])
        # (of the band problem only the cloud and the camera are used: the producer fills the image)
        c = bb.Case(hip, H, W, "noise", dtype, upload=lambda P: getattr(P, "set_" + producer)(crop), tag=producer)
        try:
            image = c.image
            assert image.shape == (H, W) and np.isfinite(image).all() and image.max() > image.min()   # (a constant image tests no border)
            assert np.array_equal(image, image.astype(np.float32).astype(np.float64))   # the producers make float32 texels
            _, seen = _check(hip, c, POSES)
            c.report(seen, POSES[1], bb.LOSSES[1], "producer")
        finally:
            c.close()
