"""examples/auto_scale_demo.c on the GPU: plain C99 against include/ea_hip.h, the same frame pair with the DT image as given
and times 255.  With CauchyLoss(1.) fixed the two runs are different problems and their iterates part; with
ea_problem_set_loss_auto_scale the scale follows the image (a x 255) and the poses agree.  The program's numbers are the ones
the ctypes stub gives for the same calls."""
import os
import subprocess

import numpy as np
import pytest

import weights_ref as wr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_auto_scale_demo(hip, tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "examples"), "auto_scale_demo"])
    pb = wr.solve_problem(*wr.SOLVE_PROBLEMS[0])
    X = np.ascontiguousarray(pb["xyz"][:, :3], dtype=np.float64)
    grid = np.ascontiguousarray(pb["grid"], dtype=np.float64)
    pts, gr = str(tmp_path / "points.f64"), str(tmp_path / "grid.f64")
    X.tofile(pts); grid.tofile(gr)
    out = subprocess.run([os.path.join(ROOT, "examples", "auto_scale_demo"), str(X.shape[0]), str(grid.shape[0]), str(grid.shape[1]),
                          *[repr(float(k)) for k in pb["K"]], pts, gr], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = [ln.split() for ln in out.stdout.strip().split("\n")]
    assert [ln[:2] for ln in lines[:4]] == [["fixed", "1"], ["fixed", "255"], ["auto", "1"], ["auto", "255"]]
    rows = [[float(x) for x in ln[2:]] for ln in lines[:4]]
    ratio, rot_fixed, tr_fixed, rot_auto, tr_auto = [float(x) for x in lines[4]]
    print(out.stdout)
    # fixed scale: a stays 1 and the two images give different answers; auto: a = max(1e-6, 2.385 median), 255 times apart
    assert rows[0][8] == 1.0 and rows[1][8] == 1.0
    assert max(rot_fixed, tr_fixed) > 1e-6
    for r in rows[2:]:
        assert r[8] == max(1e-6, 2.385 * r[9]) and int(r[10]) == X.shape[0]
    assert abs(ratio - 255.0) <= 1e-12 * 255.0
    assert rot_auto < 1e-6 and tr_auto < 1e-6
    # the same calls through the stub: the same bits
    P = hip.Problem(*pb["K"], dtype=hip.EA_F64)
    P.set_points(X); P.set_dt_grid(grid); P.set_loss(hip.LOSS_CAUCHY, 1.0)
    P.set_loss_auto_scale(2.385, 0.5, 1e-6)
    v, m = P.residual_quantiles(wr.Q0, wr.T0, [0.5])
    q, t, s = P.solve(wr.Q0, wr.T0)
    assert rows[2][:4] == list(q) and rows[2][4:7] == list(t) and int(rows[2][7]) == s["num_iterations"]
    assert rows[2][9] == v[0] and rows[2][8] == P.get_loss()[1] and m == X.shape[0]
    P.close()
