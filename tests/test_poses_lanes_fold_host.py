"""The fold inside the launches of the one-pose-per-lane evaluation (edge_alignment_amd/csrc/ea_poses_map.h: runs of 16 rows,
two levels of arrival counters, lane-minor rows and run partials, one pinned flag per (group of the call, problem)) on the CPU:
the stand-alone program tests/poses_lanes_fold_host_shim.cpp, built with the host compiler under AddressSanitizer and UBSan,
plays every launch of a call -- row counts 1 .. 40 and 98, 1 - 4 ragged problems (one of them without a point), K in
{1, 63, 64, 65, 130, 2000}, launches of K, 64 and 7 poses, both item orders -- into arrays of the sizes the host allocates and
checks: every row in exactly one run, runs of 16 except the last, ticket targets equal to the arrivals, every offset inside
its array, one flag per (group, problem)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fold_mapping_sweep_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "poses_lanes_fold_host")
    src = os.path.join(ROOT, "tests", "poses_lanes_fold_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_poses_map.h"), os.path.join(csrc, "ea_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    # 41 row counts x 4 problem counts x (K, G) pairs {1: 1, 63: 2, 64: 3, 65: 3, 130: 3, 2000: 2} x 2 orders + 2
    assert r.stdout.strip().startswith("ok ") and int(r.stdout.split()[1]) == 41 * 4 * 14 * 2 + 2
