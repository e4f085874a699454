"""bench.py --dump-outputs without a GPU: the helper that writes the timed path's arrays keeps their dtype, writes the
whole batch when it fits, and beyond the size budget the same seeded sample of batch entries every time."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("ilqr_bench", os.path.join(ROOT, "bench.py"))
bench = importlib.util.module_from_spec(spec)
spec.loader.exec_module(bench)


def _arrays(B, axis=0):
    rng = np.random.default_rng(0)
    a = {"X": rng.standard_normal((B, 4, 21)).astype(np.float32), "K": rng.standard_normal((B, 20, 1, 4)),
         "cost": np.repeat(np.arange(B, dtype=np.float64)[:, None], 3, axis=1)}      # cost[b, :] = b
    return {k: np.moveaxis(v, 0, axis) for k, v in a.items()}


def test_whole_batch_when_it_fits(tmp_path):
    a = _arrays(16)
    d = bench.dump_outputs(str(tmp_path), a)
    assert d["batch_entries"] == d["of"] == 16
    for k, v in a.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == v.dtype
        np.testing.assert_array_equal(got, v)


@pytest.mark.parametrize("axis", [0, 1])
def test_seeded_sample_beyond_the_budget(tmp_path, axis):
    a = _arrays(500, axis)
    budget = 100_000
    d1 = bench.dump_outputs(str(tmp_path / "a"), a, axis=axis, budget=budget)
    d2 = bench.dump_outputs(str(tmp_path / "b"), a, axis=axis, budget=budget)
    assert d1 == dict(d2, dir=d1["dir"]) and 0 < d1["batch_entries"] < 500
    assert sum(os.path.getsize(tmp_path / "a" / f"{k}.npy") for k in a) <= budget
    idx = np.take(np.load(tmp_path / "a" / "cost.npy"), 0, axis=1 - axis).astype(int)   # the entries written
    assert np.all(np.diff(idx) > 0)
    for k, v in a.items():
        got = np.load(tmp_path / "a" / f"{k}.npy")
        np.testing.assert_array_equal(got, np.load(tmp_path / "b" / f"{k}.npy"))
        np.testing.assert_array_equal(got, np.take(v, idx, axis=axis))


def test_only_float_arrays(tmp_path):
    with pytest.raises(TypeError):
        bench.dump_outputs(str(tmp_path), {"status": np.zeros(4, dtype=np.int32)})
