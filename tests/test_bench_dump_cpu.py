"""bench.py --dump-outputs on the CPU: dump_outputs writes float32 arrays, whole within the byte budget, and past it
the same seeded sample of elements on every call, so that two builds' dumps line up element for element."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def test_dump_whole_within_budget(tmp_path):
    ent = torch.arange(12, dtype=torch.float32).reshape(3, 4)
    losses = torch.tensor([1.5, 0.25], dtype=torch.float64)
    bench.dump_outputs(str(tmp_path / "d"), {"ent": ent, "losses": losses})
    got = np.load(tmp_path / "d" / "ent.npy")
    assert got.dtype == np.float32 and got.shape == (3, 4) and (got == ent.numpy()).all()
    got = np.load(tmp_path / "d" / "losses.npy")
    assert got.dtype == np.float32 and got.tolist() == [1.5, 0.25]


def test_dump_sample_is_fixed_and_bounded(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 4 * 1000)
    monkeypatch.setattr(bench, "DUMP_WHOLE_BELOW", 16)
    big = torch.arange(10000, dtype=torch.float32).reshape(100, 100)
    small = torch.arange(10, dtype=torch.float32)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"big": big, "small": small})
    a, b = np.load(tmp_path / "a" / "big.npy"), np.load(tmp_path / "b" / "big.npy")
    assert a.dtype == np.float32 and a.ndim == 1 and 16 <= a.size <= 1000
    assert (a == b).all()                       # the same elements on every run
    assert (np.diff(a) >= 0).all() and a.max() > 5000   # sorted flat indices spread over the whole array
    assert (np.load(tmp_path / "a" / "small.npy") == small.numpy()).all()   # small arrays stay whole
    # another array's values at the same positions: the sample depends on sizes and order only, not on contents
    bench.dump_outputs(str(tmp_path / "c"), {"big": big * 2, "small": small})
    assert (np.load(tmp_path / "c" / "big.npy") == 2 * a).all()
