"""The workspace layout of the frame producers (edge_alignment_amd/csrc/ea_frame_ws.h: frame extent -> offset and size of
every named region, and the total ensure_ws allocates) on the CPU: the stand-alone program tests/frame_ws_host_shim.cpp,
built with the host compiler under AddressSanitizer and UBSan, sweeps H, W over {3, 4, 31, 32, 33, 63, 64, 65, 255, 256, 257}^2
plus 480x640, 1536x2048, 3x16384, 32768x3 and 32767x32768 and checks for every shape that each region starts 256-aligned,
that regions are pairwise disjoint, that each is at least as large as its kernels need, that the last one ends inside the
total, that nothing overflows size_t and that the total stays within the bound the header derives."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_layout_sweep_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "frame_ws_host")
    src = os.path.join(ROOT, "tests", "frame_ws_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_frame_ws.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().startswith("ok ") and int(r.stdout.split()[1]) == 11 * 11 + 5
