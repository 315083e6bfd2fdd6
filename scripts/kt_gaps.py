#!/usr/bin/env python3
"""rocprofv3 --kernel-trace: the idle time between consecutive dispatches, per (previous kernel, this kernel) pair.

kt_by_grid.py gives the durations per (kernel, grid); this gives what lies between them -- the kernel boundaries of the
pose-batched call (evaluation -> fold -> evaluation ...), which is where a call of several launches loses the time its
kernels do not account for.  Only pairs less than 1 ms apart are counted (the same call).
usage: kt_gaps.py <dir or csv> [substring the kernel names must contain, default ea_]
"""
import csv
import glob
import os
import sys


def main():
    src = sys.argv[1]
    want = sys.argv[2] if len(sys.argv) > 2 else "ea_"
    files = [src] if os.path.isfile(src) else glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True)
    ev = []
    for f in files:
        with open(f, newline="") as fh:
            for r in csv.DictReader(fh):
                name = r.get("Kernel_Name", "").split("(")[0].replace("void ea::", "").split("<")[0]
                grid = "x".join(str(int(r.get(k, 0) or 0)) for k in ("Grid_Size_X", "Grid_Size_Y") if k in r)
                ev.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name, grid))
    ev.sort()
    pairs = {}
    for a, b in zip(ev, ev[1:]):
        gap = b[0] - a[1]
        if want in a[2] and want in b[2] and gap < 1000000:
            pairs.setdefault((a[2], a[3], b[2], b[3]), []).append(gap)
    print("%-28s %-12s -> %-28s %-12s %6s %9s %9s %9s" % ("previous", "grid", "next", "grid", "pairs", "median_ns", "min_ns", "max_ns"))
    for k, g in sorted(pairs.items(), key=lambda kv: -len(kv[1])):
        g.sort()
        print("%-28s %-12s -> %-28s %-12s %6d %9d %9d %9d" % (k[0][:28], k[1], k[2][:28], k[3], len(g), g[len(g) // 2], g[0], g[-1]))


if __name__ == "__main__":
    main()
