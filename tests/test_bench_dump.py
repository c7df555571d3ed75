"""CPU: bench.py --dump-outputs' sampling -- exact values in float32 / float64, the 64 MB budget, the same cells from
run to run and from raster to raster."""
import importlib
import os

import numpy as np
import torch

bench = importlib.import_module("bench")


def _rasters(H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    return {"slope": torch.rand((H, W), generator=g) * 100,
            "fdr": torch.randint(0, 256, (H, W), generator=g, dtype=torch.int32).to(torch.uint8),
            "river": torch.randint(0, 2, (H, W), generator=g, dtype=torch.int8),
            "fac": torch.randint(-100, 2 ** 31 - 1, (H, W), generator=g, dtype=torch.int32),
            "idx": torch.randint(-100, 2 ** 40, (H, W), generator=g, dtype=torch.int64)}


def test_whole_rasters_when_they_fit_exact_values():
    r = _rasters(64, 96)
    d = bench.dump_sample(r)
    assert set(d) == set(r)
    assert {k: v.dtype for k, v in d.items()} == {"slope": np.float32, "fdr": np.float32, "river": np.float32,
                                                  "fac": np.float64, "idx": np.float64}
    for k, t in r.items():
        assert d[k].shape == (64, 96)
        assert np.array_equal(d[k].astype(t.numpy().dtype), t.numpy()), k


def test_sample_within_budget_same_cells_every_call(tmp_path):
    H, W = 600, 700
    r = _rasters(H, W)
    budget = 1 << 20
    a, b = bench.dump_sample(r, budget=budget), bench.dump_sample(_rasters(H, W), budget=budget)
    n = len(a["slope"])
    assert 0 < n < H * W and all(v.shape == (n,) for v in a.values())
    assert all(np.array_equal(a[k], b[k]) for k in a)
    names = bench.write_dump(str(tmp_path), a)
    assert sum(os.path.getsize(tmp_path / f) for f in names) <= budget
    # the same cells of every raster: recover them from one raster whose value is the flat index
    lin = torch.arange(H * W, dtype=torch.int64).view(H, W)
    cells = bench.dump_sample({"lin": lin, **{k: v for k, v in r.items() if k != "lin"}}, budget=budget)
    flat = cells["lin"].astype(np.int64)
    assert np.all(np.diff(flat) > 0)
    for k, t in r.items():
        assert np.array_equal(cells[k].astype(t.numpy().dtype), t.numpy().reshape(-1)[flat]), k
    # a strided view (a rank tile's core) gives the values of a contiguous copy
    big = torch.zeros((H + 8, W + 8), dtype=torch.float32)
    big[4:4 + H, 4:4 + W] = r["slope"]
    v = bench.dump_sample({"slope": big[4:4 + H, 4:4 + W]}, budget=budget // 4)
    c = bench.dump_sample({"slope": r["slope"].clone()}, budget=budget // 4)
    assert np.array_equal(v["slope"], c["slope"])
