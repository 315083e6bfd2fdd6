"""The halving stage of the batched ROS producers (edge_alignment_amd/csrc/ea_frame_ws.h: frame_stage -- full extent,
halvings, host or device frames -> where the full-size frames and the ping-pong partners of the halving steps lie behind a
frame's workspace, and the stride from one frame's block to the next) on the CPU: the stand-alone program
tests/frame_stage_host_shim.cpp, built with the host compiler under AddressSanitizer and UBSan, lays it out for full extents
(12, 12) with 2 halvings, (74, 140) with 1, (256, 1028) with 2, (480, 640) with 0..3, and the smallest and largest frames the
call accepts, for host and for device frames, and checks that each region starts 256-aligned, that regions are pairwise
disjoint and none overlaps frame_ws of the working extent, that the total stays within the bound the header states, and that
every halving step finds a source and a destination large enough for its extent that are not the same region."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_layout_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "frame_stage_host")
    src = os.path.join(ROOT, "tests", "frame_stage_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_frame_ws.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().startswith("ok ") and int(r.stdout.split()[1]) == 16 * 2
