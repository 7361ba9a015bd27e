"""bench.py --dump-outputs on the host: the arrays go out as float32 (status as float64, its bits exactly), and over the size limit
every array keeps the same fixed, seeded sample of arena rows, listed in arena_rows.npy."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import bench  # noqa: E402  (the repository root is on sys.path: tests/conftest.py)


def _outs(n):
    g = torch.Generator().manual_seed(5)
    return (torch.randn(n, 11, generator=g), torch.randn(n, generator=g), torch.randint(0, 2, (n,), generator=g, dtype=torch.uint8),
            None, torch.randn(n, generator=g), torch.randint(0, 1 << 30, (n,), generator=g, dtype=torch.int32))


def test_dump_outputs_writes_every_array_as_float(tmp_path):
    outs = _outs(1000)
    bench.dump_outputs(str(tmp_path), outs)
    assert sorted(os.listdir(tmp_path)) == ["done.npy", "grumpy_score.npy", "obs.npy", "reward.npy", "status.npy"]
    for name, t in zip(bench.DUMP_NAMES, outs):
        if t is None:
            continue
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == (np.float64 if name == "status" else np.float32), name
        assert np.array_equal(a, t.numpy()), name


def test_dump_outputs_over_the_limit_keeps_one_seeded_sample_of_rows(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 40000)
    outs = _outs(1000)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), outs)
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= 40000
    rows = np.load(tmp_path / "a" / "arena_rows.npy")
    assert np.array_equal(rows, np.load(tmp_path / "b" / "arena_rows.npy"))
    idx = rows.astype(np.int64)
    assert 0 < len(idx) < 1000 and np.array_equal(idx, rows) and (np.diff(idx) > 0).all()
    for name, t in zip(bench.DUMP_NAMES, outs):
        if t is not None:
            assert np.array_equal(np.load(tmp_path / "a" / f"{name}.npy"), t.numpy()[idx]), name
