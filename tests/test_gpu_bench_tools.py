"""GPU: the eight op benchmark tools run in-process on a small raster and each prints what it says it prints -- one JSON
line, the same line in --out, its own name, the size, how it timed, and times that are finite and > 0.  This holds the
shared scaffold (tools/_bench.py) together; what the ops compute has tests of its own.

512 is more than one 64-cell tile in each direction, and the river threshold N // 512 = 512 cells still leaves a network
on the benchmark terrain."""
import importlib
import json
import math
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOOLS = ["stream_order_bench", "watershed_bench", "fa_weighted_bench", "dinf_bench", "reach_bench", "proximity_bench",
         "dinf_distance_bench", "regions_bench"]
# a key that holds times (ms, count_ms, ms_min_max, device_ms ...) or a rate derived from them
TIME_KEY = re.compile(r"(^|_)ms($|_)|GB|ratio|_over_")


def _times(obj, timed=False):
    """every number under a key that holds times, at any depth"""
    if isinstance(obj, dict):
        for k, v in obj.items():
            yield from _times(v, timed or bool(TIME_KEY.search(k)))
    elif isinstance(obj, list):
        for v in obj:
            yield from _times(v, timed)
    elif timed:
        yield obj


@pytest.mark.gpu
@pytest.mark.parametrize("tool", TOOLS)
def test_tool_prints_one_json_line(tool, tmp_path, capsys, monkeypatch):
    monkeypatch.syspath_prepend(os.path.join(ROOT, "tools"))
    out = tmp_path / (tool + ".json")
    importlib.import_module(tool).main(["--size", "512", "--steps", "2", "--warmup", "1", "--out", str(out)])
    line = capsys.readouterr().out.strip()
    res = json.loads(line)
    assert out.read_text() == line + "\n"
    assert res["tool"] == tool and res["size"] == [512, 512] and res["steps"] == 2 and res["warmup"] == 1
    # regions_bench times two tiers: its device times are described in its docstring, its host times under
    # "host_timing"; every other tool says how it timed under "timing"
    how = res["host_timing" if tool == "regions_bench" else "timing"]
    assert isinstance(how, str) and how
    times = list(_times(res))
    assert len(times) >= 3
    for v in times:
        assert isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) and v > 0, (v, res)
