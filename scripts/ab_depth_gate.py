"""What occlusion weights from the current frame's depth cost for a 32-stream tracker: same process, same box, fp64, 32
problems of 50 000 points each on 640 x 480 images with uint16 depth, window radius 1, weights written (apply).

  new    ea_batch_depth_gate_device with apply and no class buffer: one launch, one wait, nothing per point crosses the bus.
  today  the route a caller had before the gate existed, on that API: ea_problem_get_points per problem (a read-back), the
         classification in numpy on the host (the restatement of the header's arithmetic, written out here so that the script
         stands alone), ea_problem_set_weights per problem (an upload).

A leg is WARM warm-up calls and TIMED timed ones; its figure is the MEDIAN call, with the fastest and slowest beside it; the
legs run today, new, today, new, and the verdict line sets the new leg's SLOWER run against today's FASTER run.  Every timed
call ends synchronised, so a time is a host clock around the call.  Asserted: both routes leave the same weights, bit for
bit, and count the same classes.

usage: python scripts/ab_depth_gate.py > profiles/depth_gate_ab.txt
       python scripts/ab_depth_gate.py trace CALLS     CALLS gate calls after the set-up and nothing else, to be run under
                                                       rocprofv3 --kernel-trace --hip-trace --stats: two runs with different
                                                       CALLS give the launches and waits per call as a difference"""
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
Z_SCALING = 5000.0
PRM = dict(radius=1, abs_tol=0.02, rel_tol=0.02, w_occluded=0.0, w_free=0.0, w_unknown=1.0)


def make_points(seed):
    rng = np.random.default_rng(seed)
    z = rng.uniform(0.5, 5.0, POINTS)
    u, v = rng.uniform(0.0, W, POINTS), rng.uniform(0.0, H, POINTS)
    return np.stack([(u - K[2]) * z / K[0], (v - K[3]) * z / K[1], z], axis=1)


def make_depth(seed):
    """a smooth surface between 0.5 and 5 m with steps (occluders) and holes (no measurement)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    metres = 2.75 + 2.0 * np.sin(xx / 97.0 + seed) * np.cos(yy / 71.0)
    metres[100:220, 150:300] -= 1.0
    raw = np.clip(metres * Z_SCALING, 1, 65535).astype(np.uint16)
    raw[rng.uniform(size=(H, W)) < 0.05] = 0
    return raw


def classify(xyz, T, depth):
    """the header's steps 1-6 in numpy (plain problem, uint16 depth)"""
    x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    r = PRM["radius"]
    with np.errstate(all="ignore"):
        bx = ((T[0, 0] * x + T[0, 1] * y) + T[0, 2] * z) + T[0, 3]
        by = ((T[1, 0] * x + T[1, 1] * y) + T[1, 2] * z) + T[1, 3]
        bz = ((T[2, 0] * x + T[2, 1] * y) + T[2, 2] * z) + T[2, 3]
        u = K[0] * (bx / bz) + K[2]
        v = K[1] * (by / bz) + K[3]
        behind = ~((bz > 0.0) & (bz < np.inf))
        fin = np.isfinite(u) & np.isfinite(v) & (np.abs(u) < 1e9) & (np.abs(v) < 1e9)
        iu = np.where(fin, np.trunc(np.where(fin, u, 0.0)), -1).astype(np.int64)
        iv = np.where(fin, np.trunc(np.where(fin, v, 0.0)), -1).astype(np.int64)
        act = ~behind & fin & (iu >= 0) & (iu < W) & (iv >= 0) & (iv < H) & (u > -1.0) & (v > -1.0)
        iu, iv = np.where(act, iu, 0), np.where(act, iv, 0)
        metres, valid = depth.astype(np.float64) / Z_SCALING, depth != 0
        have = np.zeros(len(z), bool)
        best, best_e = np.zeros(len(z)), np.zeros(len(z))
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                row, col = iv + dy, iu + dx
                inb = act & (row >= 0) & (row < H) & (col >= 0) & (col < W)
                rc, cc = np.clip(row, 0, H - 1), np.clip(col, 0, W - 1)
                ok = inb & valid[rc, cc]
                d = metres[rc, cc]
                e = np.abs(d - bz)
                take = ok & (~have | (e < best_e))
                best, best_e = np.where(take, d, best), np.where(take, e, best_e)
                have |= take
        tol = PRM["abs_tol"] + PRM["rel_tol"] * bz
        diff = best - bz
        cons = np.abs(diff) <= tol
    cls = np.full(len(z), 1, np.uint8)
    cls[behind] = 0
    cls[act & ~have] = 2
    cls[act & have & cons] = 3
    cls[act & have & ~cons & (diff < 0.0)] = 4
    cls[act & have & ~cons & ~(diff < 0.0)] = 5
    g = np.ones(len(z))
    g[cls == 2], g[cls == 4], g[cls == 5] = PRM["w_unknown"], PRM["w_occluded"], PRM["w_free"]
    return cls, g


def host_route(problems, Ts, depths):
    counts = []
    for P, T, depth in zip(problems, Ts, depths):
        cls, w = classify(P.get_points(), T, depth)
        P.set_weights(w)
        counts.append(np.bincount(cls, minlength=6).tolist())
    return counts


def leg(fn):
    times = []
    for _ in range(WARM + TIMED):
        t0 = time.perf_counter()
        fn()
        times.append((time.perf_counter() - t0) * 1e3)
    t = np.sort(times[WARM:])
    return float(np.median(t)), float(t[0]), float(t[-1])


def main():
    if capi.device_count() < 1:
        raise SystemExit("no gfx950 device: this script measures, it has no CPU form")
    problems, depths = [], [make_depth(i) for i in range(N)]
    grid = np.ascontiguousarray(np.random.default_rng(0).uniform(0.0, 1.0, (W, H)))
    for i in range(N):
        P = capi.Problem(*K, dtype=capi.EA_F64)
        P.set_points(make_points(100 + i))
        P.set_dt_grid(grid)
        problems.append(P)
    B = capi.Batch(problems)
    B.set_now_depth(depths, Z_SCALING)
    Ts = np.stack([capi.pose_to_matrix([0.9995, 0.01 + 0.001 * i, -0.02, 0.015], [0.02, -0.01, 0.03 + 0.002 * i]) for i in range(N)])
    if len(sys.argv) > 2 and sys.argv[1] == "trace":
        calls = int(sys.argv[2])
        for _ in range(calls):
            B.depth_gate_device(Ts, None, apply=1, **PRM)
        print("trace: %d ea_batch_depth_gate_device calls of %d problems x %d points" % (calls, N, POINTS))
        return
    out = {}
    legs = [("today: get_points + numpy classification + set_weights", lambda: out.__setitem__("today", host_route(problems, Ts, depths))),
            ("new: ea_batch_depth_gate_device (apply, no class buffer)", lambda: out.__setitem__("new", B.depth_gate_device(Ts, None, apply=1, **PRM)))]
    print("depth gate A/B: %d problems x %d points, %d x %d uint16 depth, radius %d, fp64, weights written; %d warm-up + %d timed calls per leg, median [min .. max] ms per call"
          % (N, POINTS, W, H, PRM["radius"], WARM, TIMED))
    med = {}
    for rep in range(2):
        for name, fn in legs:
            m, lo, hi = leg(fn)
            med.setdefault(name, []).append(m)
            print("  run %d  %-58s %9.3f  [%9.3f .. %9.3f]" % (rep, name, m, lo, hi))
    slow_new, fast_today = max(med[legs[1][0]]), min(med[legs[0][0]])
    print("the device call's slower run against the host route's faster run: %.3f against %.3f ms, x %.0f"
          % (slow_new, fast_today, fast_today / slow_new))
    # the same weights and counts from both routes
    today = host_route(problems, Ts, depths)
    w_today = [P.get_weights().copy() for P in problems]
    new = B.depth_gate_device(Ts, None, apply=1, **PRM)
    names = ("n_behind", "n_outside", "n_unknown", "n_consistent", "n_occluded", "n_free")
    assert [[s[k] for k in names] for s in new] == today, "the routes disagree on the counts"
    for P, w in zip(problems, w_today):
        assert np.array_equal(P.get_weights().view(np.uint64), w.view(np.uint64)), "the routes disagree on a weight"
    tot = np.sum(today, axis=0)
    print("both routes write the same %d x %d weights; classes over the batch: behind %d outside %d unknown %d consistent %d occluded %d free %d"
          % ((N, POINTS) + tuple(int(v) for v in tot)))
    B.close()
    for P in problems:
        P.close()


if __name__ == "__main__":
    main()
