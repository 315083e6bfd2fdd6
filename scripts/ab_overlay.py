"""What the reference's reproject + s_overlay self-check costs for a 32-stream tracker: same process, same box, fp64, 32
problems of 50 000 points each on 640 x 480 images.

  new    ea_batch_overlay_device (32 device images painted in place), ea_batch_reproject_device (the (u, v) rows into a
         device tensor) and, for a caller whose images live on the host, ea_batch_overlay (images up, painted, back).
  today  what a caller of the library had to do before these calls existed: ea_problem_get_points per problem (a read-back),
         the projection in numpy on the host, and a numpy paint of the host image.

A leg is WARM warm-up calls and TIMED timed ones; its figure is the MEDIAN call, with the fastest and slowest beside it; the
legs run today, new, today, new.  Every timed call ends synchronised (the library's calls return complete; the host route
is host work), so a time is a host clock around the call.  Asserted: both routes paint the same images and count the same
points.  Launches, synchronisations and copies per call are counted from the code (csrc/ea_segments.hip), not measured.

usage: python scripts/ab_overlay.py > profiles/overlay_ab.txt"""
import sys
import time

import numpy as np

sys.path.insert(0, ".")
import torch  # noqa: E402  (first: one HIP runtime in the process)

if torch.cuda.is_available():
    torch.cuda.init()
from edge_alignment_amd import capi  # noqa: E402

K = (525.0, 525.0, 319.5, 239.5)
H, W, N, POINTS, WARM, TIMED = 480, 640, 32, 50000, 3, 15


def make_points(seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.5, 5.0, POINTS)
    u, v = rng.uniform(0.0, W, POINTS), rng.uniform(0.0, H, POINTS)
    return np.stack([(u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z], axis=1)


def host_route(problems, Ts, images):
    """read the points back, project and paint on the host: one problem at a time"""
    stats = []
    for P, T, img in zip(problems, Ts, images):
        xyz = P.get_points()
        x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        with np.errstate(all="ignore"):
            bx = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
            by = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
            bz = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]
            u = K[0] * (bx / bz) + K[2]
            v = K[1] * (by / bz) + K[3]
            fin = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
            iu = np.where(fin, np.trunc(np.where(fin, u, 0.0)), -1).astype(np.int64)
            iv = np.where(fin, np.trunc(np.where(fin, v, 0.0)), -1).astype(np.int64)
            ok = fin & (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H) & (u > -1.0) & (v > -1.0)
        img[iv[ok], iu[ok]] = (0, 0, 255)
        stats.append(dict(n=POINTS, inside=int(ok.sum()), outside=int((~ok).sum())))
    return stats


def leg(fn, reset):
    times = []
    for k in range(WARM + TIMED):
        reset()
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    t = np.sort(times[WARM:])
    return float(np.median(t)), float(t[0]), float(t[-1])


def main():
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: this script measures, it has no CPU form")
    problems = []
    grid = np.ascontiguousarray(np.random.default_rng(0).uniform(0.0, 1.0, (W, H)))
    for i in range(N):
        P = capi.Problem(*K, dtype=capi.EA_F64)
        P.set_points(make_points(100 + i))
        P.set_dt_grid(grid)
        problems.append(P)
    B = capi.Batch(problems)
    Ts = np.stack([capi.pose_to_matrix([0.9995, 0.01 + 0.001 * i, -0.02, 0.015], [0.02, -0.01, 0.03 + 0.002 * i]) for i in range(N)])
    grey = np.full((H, W, 3), 128, np.uint8)
    host_images = [grey.copy() for _ in range(N)]
    dev_images = [torch.from_numpy(grey.copy()).cuda() for _ in range(N)]
    uv_dev = torch.zeros((N * POINTS, 2), dtype=torch.float64, device="cuda")
    out = {}

    def reset_host():
        for img in host_images:
            img[:] = 128

    def reset_dev():
        for img in dev_images:
            img.fill_(128)
        torch.cuda.synchronize()

    legs = [("today: get_points + numpy projection + numpy paint", lambda: out.__setitem__("today", host_route(problems, Ts, host_images)), reset_host),
            ("new: ea_batch_overlay_device", lambda: out.__setitem__("new", B.overlay_device(Ts, dev_images)), reset_dev),
            ("new: ea_batch_reproject_device", lambda: B.reproject_device(Ts, uv_dev), lambda: None),
            ("new: ea_batch_overlay (host images up and back)", lambda: out.__setitem__("host", B.overlay(Ts, host_images, in_place=True)[1]), reset_host)]
    print("overlay A/B: %d problems x %d points, %d x %d images, fp64; %d warm-up + %d timed calls per leg, median [min .. max] ms per call"
          % (N, POINTS, W, H, WARM, TIMED))
    for rep in range(2):
        for name, fn, reset in legs:
            med, lo, hi = leg(fn, reset)
            print("  run %d  %-52s %9.3f  [%9.3f .. %9.3f]" % (rep, name, med, lo, hi))
    # the same images and counts from both routes
    reset_host()
    today = host_route(problems, Ts, host_images)
    reset_dev()
    new = B.overlay_device(Ts, dev_images)
    assert today == new == out["host"], "the routes disagree on the counts"
    for a, b in zip(host_images, dev_images):
        assert np.array_equal(a, b.cpu().numpy()), "the routes disagree on an image"
    print("both routes paint the same %d images; inside per problem %d .. %d of %d"
          % (N, min(s["inside"] for s in new), max(s["inside"] for s in new), POINTS))
    print("per call, counted from the code:")
    print("  ea_batch_overlay_device / ea_batch_reproject_device: 1 kernel launch, 1 stream synchronisation, 1 upload (segments and")
    print("    matrices, %d bytes), overlay: 1 download (%d bytes of counters); no per-point data crosses the bus" % (N * 120 + N * 16, N * 16))
    print("  today's route: 0 launches, %d read-backs of the points (ea_problem_get_points, %d bytes each as doubles), every point"
          % (N, POINTS * 24))
    print("    projected and painted by the host")
    B.close()
    for P in problems:
        P.close()


if __name__ == "__main__":
    main()
