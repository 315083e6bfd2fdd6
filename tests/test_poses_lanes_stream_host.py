"""The coordinate stream of the one-pose-per-lane evaluation (edge_alignment_amd/csrc/ea_lanes_stream.h: which indices a
wavefront loads in which iteration, one pair ahead, and which pair an iteration consumes) on the CPU: the stand-alone program
tests/poses_lanes_stream_host_shim.cpp, built with the host compiler under AddressSanitizer and UBSan, plays the stream for every
sub-run length 1 .. 130 out of arrays of exactly that length and checks: every loaded index inside [0, n_sub), 16-byte loads of
adjacent points only, every iteration consumes (i, min(i + 1, last)) out of the registers the slot in front of it loaded, every
point consumed exactly once and in order."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stream_sweep_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "poses_lanes_stream_host")
    src = os.path.join(ROOT, "tests", "poses_lanes_stream_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_lanes_stream.h"), os.path.join(csrc, "ea_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "ok 130"
