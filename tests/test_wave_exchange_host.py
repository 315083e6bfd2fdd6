"""The slot ownership and LDS layout of the wave-exchange reduction (edge_alignment_amd/csrc/ea_wave_exchange.h, shared with
fused_chunk) on the CPU: the stand-alone program tests/wave_exchange_host_shim.cpp, built with the host compiler under
AddressSanitizer and UBSan, replays both exchange rounds and the 8-value butterfly on symbolic (wave, lane, slot) sets for all
4 waves x 64 lanes and checks that every one of the 32 slots ends as the union of all 256 lanes' entries of that slot in
exactly one storing lane, that no LDS cell is read before its last write of the same round, and that round 2 never writes a
cell another wave still has to read."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exchange_replay_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "wave_exchange_host")
    src = os.path.join(ROOT, "tests", "wave_exchange_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_wave_exchange.h"), os.path.join(csrc, "ea_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip() == "ok 32"
