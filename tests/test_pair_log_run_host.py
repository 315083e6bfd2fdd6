"""The running product of the Cauchy loss' factors (pl_run_* in edge_alignment_amd/csrc/ea_pair_log.h: what a lane of the
pose-per-lane kernel does over its sub-run -- multiply the factors up with the rounding error carried along, one logarithm
behind the run), on the CPU: the stand-alone program tests/pair_log_run_host_shim.cpp, built with the host compiler under
AddressSanitizer and UBSan, compiles the header with host stand-ins for the device's frexp / ldexp / reciprocal.

Runs of 1, 2, 127 and 128 factors 1 + x -- all ones, x <= 1e-15, x in [0, 1e-12], 10^U(-15, 8), 10^U(0, 100), one 1e200 among
tiny x, one factor at 1e300 -- against the sum of logl of the same rounded factors.  Bars: relative error <= 8 * 2^-53, nothing
non-finite, exactly 0 for all ones, no renormalisation in the first three cases and some in the last three."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pair_log_run_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "pair_log_run_host")
    src = os.path.join(ROOT, "tests", "pair_log_run_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src, os.path.join(csrc, "ea_pair_log.h"), os.path.join(csrc, "ea_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert r.stdout.strip().endswith("ok")
