"""The frame block of the batched ROS pyramid producers (edge_alignment_amd/csrc/ea_frame_ws.h: frame_pyramid -- full extent,
halvings, levels, host or device frames -> every level's workspace, one behind the other, the stage behind them, and the one
stride from a frame's block to the next) on the CPU: the stand-alone program tests/frame_pyramid_host_shim.cpp, built with the
host compiler under AddressSanitizer and UBSan, lays it out for ten full extents -- the GPU tests', 640 x 480, 1280 x 960 and
the largest accepted -- with every (halvings, levels) of at most eight halving steps that the extent is divisible for, and
checks that no two regions overlap, that each starts 256-aligned, that every level's layout is frame_ws of its extent shifted,
that the total stays within the stated bound, that levels = 1 is frame_stage number for number, and that the halving chain's
launches each find a source in memory and room for what they write."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


EXTENTS = ((74, 140), (296, 560), (272, 1040), (24, 48), (480, 640), (960, 1280), (768, 768), (1024, 4096), (32768, 32512),
           (256, 32768))


def _expected_cases():
    """the sweep of the program's main(), counted here: host and device frames for every accepted (extent, halvings, levels)"""
    n = 0
    for H, W in EXTENTS:
        for halvings in range(9):
            for levels in range(1, 10 - halvings):
                T = halvings + levels - 1
                if H % (1 << T) == 0 and W % (1 << T) == 0 and (H >> T) >= 3 and (W >> T) >= 3:
                    n += 2
    return n


def test_pyramid_layout_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "frame_pyramid_host")
    src = os.path.join(ROOT, "tests", "frame_pyramid_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_frame_ws.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().startswith("ok ") and int(r.stdout.split()[1]) == _expected_cases()

