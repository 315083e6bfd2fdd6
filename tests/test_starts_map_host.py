"""The live-list mapping of a multi-start solve (edge_alignment_amd/csrc/ea_starts_map.h: position -> start -> pose slot /
partial row, the pieces the host cuts from a stale list length, the order-preserving compaction of the step kernel's last
workgroup, the word it posts) on the CPU: the stand-alone program tests/starts_map_host_shim.cpp, built with the host compiler
under AddressSanitizer and UBSan, sweeps rows {1, 7, 98} x problems {1, 3} x live {0, 1, 8, 9} x stale lengths >= live x
launch sizes x both item orders and checks that every (position < live, row) and (position < live, problem) is taken exactly
once, at its own start, and nothing at or beyond live."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_live_list_mapping_sweep_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "starts_map_host")
    src = os.path.join(ROOT, "tests", "starts_map_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("ea_starts_map.h", "ea_poses_map.h", "ea_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 3 * 2 * 4 * 2 * 4 * 2 and int(words[3]) > 100000
