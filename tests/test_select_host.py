"""The radix select of ea_*_residual_quantiles (edge_alignment_amd/csrc/ea_select.h: key of a double, digit of a pass, prefix
match, leading quantile, histogram scan, rank rule, loss-scale rule) on the CPU: the stand-alone program
tests/select_host_shim.cpp, built with the host compiler under AddressSanitizer and UBSan, runs the six passes as the kernels
run them over sizes {1, 2, 63, 64, 65, 257, 4099} x {random, all equal, one ulp apart, +-0, denormals, 1e300 / +Inf, NaN
dropped, all NaN} x probs {0, 0.25, 0.5, 1 - 2^-53, 1} and compares bit for bit with a plain sort written out in the shim."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_select_sweep_under_sanitizers():
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "select_host")
    src = os.path.join(ROOT, "tests", "select_host_shim.cpp")
    csrc = os.path.join(ROOT, "edge_alignment_amd", "csrc")
    deps = [src] + [os.path.join(csrc, h) for h in ("ea_select.h", "ea_types.h")]
    if not os.path.exists(exe) or any(os.path.getmtime(d) > os.path.getmtime(exe) for d in deps):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-I", csrc, "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) == 7 * 8 and int(words[3]) > 7 * 8 * 5
