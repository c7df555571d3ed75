"""GPU (-m gpu): tools/cost_distance_bench.py runs in-process at --size 512 and prints what its docstring says: one JSON
line, the same line in --out, its documented keys, times that are finite and > 0 and counts that fit the raster."""
import importlib
import json
import math
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPS = ("cost_distance_uniform", "cost_distance_slope", "nearest_river", "dinf_distance_down")


@pytest.mark.gpu
def test_tool_prints_one_json_line(tmp_path, capsys, monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    out = tmp_path / "cost_distance_bench.json"
    importlib.import_module("cost_distance_bench").main(["--size", "512", "--steps", "2", "--warmup", "1",
                                                         "--out", str(out)])
    line = capsys.readouterr().out.strip()
    assert "\n" not in line
    res = json.loads(line)
    assert out.read_text() == line + "\n"
    assert res["tool"] == "cost_distance_bench" and res["size"] == [512, 512]
    assert res["steps"] == 2 and res["warmup"] == 1 and res["connectivity"] == 8 and res["px"] == 10.0
    assert isinstance(res["timing"], str) and res["timing"]
    assert res["tile"] == [64, 64] and res["tiles"] == 64 and res["river_cells"] > 0
    assert set(res["ms"]) == set(OPS) and set(res["ms_min_max"]) == set(OPS)
    for k in OPS:
        lo, hi = res["ms_min_max"][k]
        for v in (res["ms"][k], lo, hi):
            assert isinstance(v, float) and math.isfinite(v) and v > 0
        assert lo <= res["ms"][k] <= hi
    assert set(res["modes"]) == {"uniform", "slope"}
    for m in res["modes"].values():
        assert set(m) == {"rounds", "reached", "tile_visits", "reached_fraction", "visits_per_tile"}
        # no barriers on the benchmark terrain: every cell is reached; every tile is visited in the first round
        assert m["reached"] == 512 * 512 and m["reached_fraction"] == 1.0
        assert m["rounds"] >= 1 and m["tile_visits"] >= 64 and m["visits_per_tile"] >= 1.0
