"""The fp64 logarithm of the Cauchy loss, per point and per pair of points (edge_alignment_amd/csrc/ea_pair_log.h, shared with
fused_chunk and cost_item), on the CPU: the stand-alone program tests/pair_log_host_shim.cpp, built with the host compiler under
AddressSanitizer and UBSan, compiles the header with host stand-ins for the device's frexp / ldexp / reciprocal and sweeps
pairs of arguments 1 + x, x log-uniform over 1e-300 .. 1e300, plus x = 0, a member exactly 1 and members and products at the
edges of the mantissa interval, against logl of the two rounded sums.

Bar: the paired log's worst relative error is at most twice the worst error of two separate logs measured in the same sweep
(both printed); the paired form WITHOUT its error term misses that bar around x = 1e-8."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_log_sweep_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pair_log_host")
    src = os.path.join(ROOT, "tests", "pair_log_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_pair_log.h"), os.path.join(csrc, "ea_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("ok")
