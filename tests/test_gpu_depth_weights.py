"""ea_depth_weights_kernel (ea_problem_set_depth_weighting: w_i = clamp((z_ref / z_i)^power, 0, 1) written behind the points
of a reference-frame producer) bit for bit against numpy's fp64 computation

    np.fmax(0, np.fmin(1, ratio ** p))      # ratio = z_ref / z, p - 1 left-to-right multiplications

from the z the problem holds (Problem.get_points), rounded once to the problem dtype: every power 1..8, z_ref below, at and
above the depths, both dtypes, through the three reference-frame producers.  The ROS scatter keeps edge pixels without a
depth test, so its depth image gets a band of negative depths, a band of NaN and a band of 0 (stored as z = 1): the clamp
must turn NaN into weight 1, a negative odd power into 0, a negative even power into min(1, .), and leave every stored
weight finite and in [0, 1].  Only the weights are compared: what a solve does with NaN points is not under test.

Depths are kept where the power product is a normal fp32 number or exactly 0 or 1 (golden frame 1: z in [0.92, 3.46] m, the
smallest product (0.5 / 3.46)^8 = 1.9e-7; whether the device keeps an fp32 denormal when it rounds is not what this is about)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = os.path.join(ROOT, "tests", "golden", "rgbd")
K = (525.0, 525.0, 319.5, 239.5)
POWERS = tuple(range(1, 9))
Z_REFS = (0.5, 1.0, 2.75)
TINY32 = float(np.finfo(np.float32).tiny)


@pytest.fixture(scope="module")
def frame():
    from oracle import preprocess_np as pp
    return pp.load_rgb_as_bgr(os.path.join(G, "rgb_1.png")), pp.load_depth_u16(os.path.join(G, "depth_1.png"))


def _expected(z, z_ref, power, f32):
    """-> (weights as the problem dtype holds them, mask of the depths kept: product normal in fp32, or exactly 0 or 1)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = z_ref / z
        v = ratio.copy()
        for _ in range(power - 1):
            v = v * ratio
        w = np.fmax(0.0, np.fmin(1.0, v))
    keep = (w == 0.0) | (w == 1.0) | (w >= TINY32)
    return (w.astype(np.float32).astype(np.float64) if f32 else w), keep


def _check(hip, P, produce, dtype, where, extra=None):
    """every power and z_ref on one producer -> the z the weights were computed from; extra(z, w, z_ref, power): more checks"""
    z = None
    for z_ref in Z_REFS:
        for power in POWERS:
            P.set_depth_weighting(z_ref, power)
            produce(P)
            z = P.get_points()[:, 2]
            w = P.get_weights()
            assert w is not None and w.shape == z.shape, where
            assert np.isfinite(w).all() and (w >= 0.0).all() and (w <= 1.0).all(), (where, z_ref, power)
            want, keep = _expected(z, z_ref, power, dtype == hip.EA_F32)
            assert keep.mean() > 0.99, (where, z_ref, power, float(keep.mean()))
            same = w[keep] == want[keep]
            assert same.all(), (where, z_ref, power, int((~same).sum()), z[keep][~same][:4], w[keep][~same][:4], want[keep][~same][:4])
            if extra is not None:
                extra(z, w, z_ref, power)
    P.set_depth_weighting(1.0, 0)
    return z


@pytest.mark.parametrize("dtype_name", ["EA_F64", "EA_F32"])
@pytest.mark.parametrize("producer", ["set_ref_frame", "set_ref_frame_canny"])
def test_depth_weights_of_the_u16_producers(hip, frame, producer, dtype_name):
    bgr, depth = frame
    dtype = getattr(hip, dtype_name)
    P = hip.Problem(*K, dtype=dtype)
    try:
        z = _check(hip, P, lambda P: getattr(P, producer)(bgr, depth), dtype, (producer, dtype_name))
        assert len(z) > 5000 and (z > 0).all()
        # the workload: weights on both sides of the clamp at z_ref = 1 and 2.75, all below it at 0.5
        assert (z < 1.0).sum() >= 50 and (z > 1.0).sum() >= 50 and z.min() > 0.5 and z.max() > 2.75
    finally:
        P.close()


@pytest.mark.parametrize("dtype_name", ["EA_F64", "EA_F32"])
def test_depth_weights_of_the_ros_producer_with_invalid_depths(hip, frame, dtype_name):
    bgr, depth = frame
    dtype = getattr(hip, dtype_name)
    metres = depth.astype(np.float32) / np.float32(5000.0)
    metres[60:160] = -1.5
    metres[180:280] = np.nan
    metres[300:400] = 0.0
    P = hip.Problem(*K, dtype=dtype)

    def bands(z, w, z_ref, power):
        """the expected values on the bands, stated without the formula under test"""
        neg, nan = z < 0, np.isnan(z)
        assert (w[nan] == 1.0).all(), (z_ref, power)
        if power % 2:
            assert (w[neg] == 0.0).all(), (z_ref, power)
        else:
            even = min(1.0, (z_ref / 1.5) ** power)   # (pow, not the kernel's multiplications: within 1e-6, never 0)
            assert (w[neg] > 0.0).all() and (np.abs(w[neg] - even) <= 1e-6 * even).all(), (z_ref, power)

    try:
        z = _check(hip, P, lambda P: P.set_ref_frame_ros(bgr, metres), dtype, ("set_ref_frame_ros", dtype_name), bands)
        neg, nan, one = z < 0, np.isnan(z), z == 1.0
        assert neg.sum() >= 50 and nan.sum() >= 50 and one.sum() >= 50, (int(neg.sum()), int(nan.sum()), int(one.sum()))
        assert (z[neg] == -1.5).all() and not (z == 0).any()
    finally:
        P.close()
