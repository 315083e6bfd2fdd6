"""bench.py --dump-outputs on CPU: float64 files, every step below the size limit, above it a fixed seeded sample of the
steps that always holds the last one, with the steps' indices beside the arrays."""
import os

import numpy as np

import bench


def _arrays(K):
    rng = np.random.default_rng(1)
    return {"cost": rng.random((K, 1)), "JtJ": rng.random((K, 1, 6, 6)), "n_invalid": np.arange(K, dtype=np.int64)[:, None]}


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_every_step_below_the_limit(tmp_path):
    a = _arrays(20)
    bench.dump_outputs(str(tmp_path), a)
    got = _load(str(tmp_path))
    assert set(got) == {"cost", "JtJ", "n_invalid", "step_index"}
    assert all(x.dtype == np.float64 for x in got.values())
    assert np.array_equal(got["step_index"], np.arange(20))
    for k in a:
        assert np.array_equal(got[k], a[k])


def test_a_fixed_sample_above_the_limit(tmp_path):
    a = _arrays(1000)
    limit = 100 * (8 + 36 * 8 + 8 + 8)
    bench.dump_outputs(str(tmp_path / "x"), a, limit=limit)
    bench.dump_outputs(str(tmp_path / "y"), a, limit=limit)
    x, y = _load(str(tmp_path / "x")), _load(str(tmp_path / "y"))
    assert sum(v.nbytes for v in x.values()) <= limit
    idx = x["step_index"].astype(np.int64)
    assert len(idx) == 100 and idx[-1] == 999 and np.all(np.diff(idx) > 0)
    for k in a:
        assert np.array_equal(x[k], a[k][idx]) and np.array_equal(x[k], y[k])
