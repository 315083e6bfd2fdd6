"""The candidate ranking of ea_batch_search_starts (edge_alignment_amd/csrc/ea_search_rank.h: eligible = finite cost and no
failed functor, by ascending cost, ties to the lower index, the ineligible behind them by index) on the CPU: the stand-alone
program tests/search_rank_host_shim.cpp, built with the host compiler under AddressSanitizer and UBSan, sweeps count {1, 3} x
K {1, 2, 9, 257} x M {1, K / 2, K} over random costs with planted exact ties, NaN and +-Inf, failed functors, every candidate
ineligible and exactly M - 1 eligible, against a stable sort by (ineligible, cost, index) written out in the shim, and checks
that every column of `picked` is a permutation prefix without repeats."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_ranking_sweep_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "search_rank_host")
    src = os.path.join(ROOT, "tests", "search_rank_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("ea_search_rank.h", "ea_starts_map.h", "ea_poses_map.h", "ea_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 2 * 4 * 3 * 3 * 6 and int(words[3]) > 100000
