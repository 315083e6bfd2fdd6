"""The work-list mapping of the pose-batched evaluation with one pose per lane (edge_alignment_amd/csrc/ea_poses_map.h:
workgroup -> rider or (row, group of 64 poses) -> (term, chunk, first pose, live lanes); G and the split of K poses over
launches) on the CPU: the stand-alone program tests/poses_lanes_map_host_shim.cpp, built with the host compiler under
AddressSanitizer and UBSan, sweeps rows x poses x 1-4 ragged terms x rider counts x both item orders and checks that every
(row, pose) and every rider comes up exactly once, riders first, live-lane counts, no XCD residue class above ceil(T / 8)
items, contiguous rows per XCD in order 0, at most 7 empty workgroups, and launch sizes that are multiples of 64 except the
last for every K up to 2100."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_lanes_mapping_sweep_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "poses_lanes_map_host")
    src = os.path.join(ROOT, "tests", "poses_lanes_map_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_poses_map.h"), os.path.join(csrc, "ea_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().startswith("ok ") and int(r.stdout.split()[1]) == 2 * 2 * 8 * 5 * 7 * 4
