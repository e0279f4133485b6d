"""bench.py --dump-outputs: what it writes (float32 / float64 only, within its byte budget, the same sample every run).
No GPU: dump_outputs takes whatever tensors it is given."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_types_budget_and_fixed_sample(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BYTES", 1 << 20)
    monkeypatch.setattr(bench, "DUMP_ARRAY_ELEMS", 1 << 16)
    g = torch.Generator().manual_seed(0)
    arrays = {"render": torch.rand(3, 300, 400, generator=g), "radii": torch.randint(0, 50, (200_000,), generator=g, dtype=torch.int32),
              "visibility_filter": torch.rand(200_000, generator=g) > 0.5, "loss": torch.tensor(0.25),
              "grad_xyz": torch.randn(200_000, 3, generator=g), "small": torch.arange(10, dtype=torch.float32)}
    n1 = bench.dump_outputs(str(tmp_path / "a"), arrays)
    n2 = bench.dump_outputs(str(tmp_path / "b"), arrays)
    assert n1 == n2 <= bench.DUMP_BYTES
    assert sorted(os.listdir(tmp_path / "a")) == sorted(k + ".npy" for k in arrays)
    for name, t in arrays.items():
        a, b = np.load(tmp_path / "a" / (name + ".npy")), np.load(tmp_path / "b" / (name + ".npy"))
        assert a.dtype == (np.float32 if t.dtype == torch.float32 else np.float64)
        assert np.array_equal(a, b)                                       # the same sample in every run
        flat = t.reshape(-1).double().numpy()
        if a.size == flat.size:
            assert np.array_equal(a.reshape(-1), flat)                    # small arrays whole, in their own order
        else:
            assert a.size <= bench.DUMP_ARRAY_ELEMS and np.isin(a, flat).all()   # large ones: a sample of their elements
    assert np.load(tmp_path / "a" / "loss.npy") == np.float32(0.25)
