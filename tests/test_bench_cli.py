"""bench.py's command line without a GPU: a plain run is the headline only
(--full off by default), and --dump-outputs writes float64 .npy files of
bounded size with a fixed sample of a longer array."""
import os
import sys

import numpy as np
import pytest


@pytest.fixture()
def bench(monkeypatch):
    # bench.py sets GPU_MAX_HW_QUEUES for a one-GPU benchmark process when it
    # is first imported; keep that out of the test process's environment
    monkeypatch.setenv("WORLD_SIZE", "2")
    import bench as mod
    return mod


def test_plain_run_is_headline_only_by_default(bench, monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 3, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == "d"


def test_dump_outputs_float64_bounded_and_repeatable(bench, tmp_path, monkeypatch):
    import torch
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMENTS", 100)
    g = torch.arange(37, dtype=torch.float64) * 0.5
    v = torch.arange(1001, dtype=torch.float64) - 3.0
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"g": g, "jac_values": v})
    ga, va = np.load(tmp_path / "a" / "g.npy"), np.load(tmp_path / "a" / "jac_values.npy")
    assert ga.dtype == np.float64 and np.array_equal(ga, g.numpy())     # short: written whole
    assert va.dtype == np.float64 and va.shape == (100,)                # long: a sample of its entries
    idx = (va + 3.0).astype(int)
    assert np.all(np.diff(idx) > 0) and np.array_equal(v.numpy()[idx], va)
    assert np.array_equal(va, np.load(tmp_path / "b" / "jac_values.npy"))   # the same entries every run
    assert sorted(os.listdir(tmp_path / "a")) == ["g.npy", "jac_values.npy"]
