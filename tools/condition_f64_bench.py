"""Conditioning on float32 and on float64 heights, same terrain, one process.

Rasters: the bundled Example DEM (2178 x 1534) and tools/condition_bench.py's rough synthetic terrain at --sizes.
Tiers: "float32" (dt_dev_condition_d8 / _async), "float64" (dt_dev_condition_d8_f64 / _async) on the SAME heights cast
to float64 -- same fixed points, same rounds: what the float64 kernels cost -- and, for rasters up to 4096^2,
"float64_sub" on those heights plus k * 1e-5 (k < 8: sub-metre structure that breaks most flats): what a genuinely
float64 DEM costs (fewer flat cells, other rounds).  The synchronous form
iterates to the fixed point (one flag read per batch of rounds); the asynchronous one gets the synchronous round
count + 4 as its budget.  HIP events around each call on the launch stream, median of --reps.  Prints one JSON line
(and writes it to --out when given)."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from descriptools_amd import _lib  # noqa: E402
from descriptools_amd.device import Context  # noqa: E402
from condition_bench import example, rough  # noqa: E402

L = _lib.lib()


def time_tier(dem, px, wide, reps):
    H, W = dem.shape
    ft = np.float64 if wide else np.float32
    sync = L.dt_dev_condition_d8_f64 if wide else L.dt_dev_condition_d8
    asyn = L.dt_dev_condition_d8_f64_async if wide else L.dt_dev_condition_d8_async
    st = torch.cuda.Stream()
    ctx = Context(0, st.cuda_stream)
    d, f, c = ctx.to_device(np.ascontiguousarray(dem, ft)), ctx.empty((H, W), ft), ctx.empty((H, W), np.uint8)
    info = (C.c_int32 * 3)()

    def timed(call):
        ms = []
        for k in range(reps + 1):  # (the first call: warm-up, scratch allocation)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(st)
            _lib.check(call())
            e1.record(st)
            ctx.sync()
            if k:
                ms.append(e0.elapsed_time(e1))
        return round(float(np.median(ms)), 3)
    t_sync = timed(lambda: sync(ctx.h, d.ptr, H, W, px, f.ptr, c.ptr, info))
    assert info[0] == 0
    budget = max(info[1], info[2]) + 4
    t_async = timed(lambda: asyn(ctx.h, d.ptr, H, W, px, f.ptr, c.ptr, budget))
    ctx.raise_on_status()
    out = {"sync_ms": t_sync, "async_ms": t_async, "async_budget": budget, "fill_rounds": int(info[1]),
           "flat_rounds": int(info[2]), "fdr_sum": int(c.to_host().astype(np.int64).sum())}
    for b in (d, f, c):
        b.free()
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    rasters = [("example", example(), 12.5)] + [("rough%d" % n, rough(n), 10.0) for n in map(int, a.sizes.split(","))]
    res = {}
    for name, dem, px in rasters:
        r = {"shape": list(dem.shape), "float32": time_tier(dem, px, False, a.reps),
             "float64": time_tier(dem, px, True, a.reps)}
        assert r["float32"]["fdr_sum"] == r["float64"]["fdr_sum"], "same heights: the tiers must agree"
        if dem.size <= 4096 * 4096:
            d64 = dem.astype(np.float64)
            valid = dem != -100
            d64[valid] += np.random.default_rng(5).integers(0, 8, int(valid.sum())) * 1e-5
            r["float64_sub"] = time_tier(d64, px, True, a.reps)
        r["f64_over_f32_sync"] = round(r["float64"]["sync_ms"] / r["float32"]["sync_ms"], 3)
        r["f64_over_f32_async"] = round(r["float64"]["async_ms"] / r["float32"]["async_ms"], 3)
        res[name] = r
        print(name, json.dumps(r), file=sys.stderr, flush=True)
    out = {"tool": "condition_f64_bench", "reps": a.reps,
           "timing": "median of HIP events around each call on its stream (first call dropped)",
           "rasters": res, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
