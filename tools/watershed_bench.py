"""Drainage and upslope length (dt_dev_drainage, dt_dev_upslope_length) at 16384^2 on two inputs: the
benchmark terrain's D8 (dt_dev_synth_dem with bench.py's seed, dt_dev_slope_d8: the chain's fdr) and a rough DEM
conditioned with flowdir.d8_conditioned, whose paths run to the raster edge.  After --warmup runs, each op is timed
--steps times per input, bracketed by HIP events on the context's stream with a sync after each; medians are reported
with the basin count, the longest flow length and the largest upslope length.  Prints one JSON line (and writes it to
--out when given)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from descriptools_amd import _lib, flowdir  # noqa: E402
from descriptools_amd.device import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    st = torch.cuda.Stream()
    ctx = Context(0, st.cuda_stream)
    dev = torch.device("cuda", 0)
    # the rough DEM: white noise (every cell a pit or a flat neighbour), conditioned on the host tier
    rng = np.random.default_rng(a.seed)
    rough = np.ascontiguousarray(rng.random((H, W), dtype=np.float32) * 100.0)
    fdr_rough = flowdir.d8_conditioned(rough, px)
    del rough
    with torch.cuda.stream(st):
        dem = torch.empty((H, W), dtype=torch.float32, device=dev)
        slope = torch.empty((H, W), dtype=torch.float32, device=dev)
        fdrs = {"terrain": torch.empty((H, W), dtype=torch.uint8, device=dev),
                "conditioned": torch.from_numpy(fdr_rough).to(dev)}
        _lib.check(L.dt_dev_synth_dem(ctx.h, a.seed, H, W, 0, 0, H, W, 0, dem.data_ptr()))
        _lib.check(L.dt_dev_slope_d8(ctx.h, dem.data_ptr(), H, W, px, slope.data_ptr(), fdrs["terrain"].data_ptr(),
                                     None))
        del slope, dem, fdr_rough
        tg = torch.empty((H, W), dtype=torch.int64, device=dev)
        ln = torch.empty((H, W), dtype=torch.float64, device=dev)
        up = torch.empty((H, W), dtype=torch.float64, device=dev)

        def drainage(k):
            _lib.check(L.dt_dev_drainage(ctx.h, fdrs[k].data_ptr(), None, None, H, W, px, tg.data_ptr(),
                                         ln.data_ptr(), None))

        def upslope(k):
            _lib.check(L.dt_dev_upslope_length(ctx.h, fdrs[k].data_ptr(), None, H, W, px, up.data_ptr()))

        ops = {"drainage": drainage, "upslope_length": upslope}
        stats = {}
        for k in fdrs:
            drainage(k)
            upslope(k)
            ctx.sync()
            ok = tg.view(-1) >= 0
            stats[k] = {"basins": int(torch.unique(tg.view(-1)[ok]).numel()), "cells_without_target":
                        int((~ok).sum()), "max_length": float(ln.max()), "max_upslope_length": float(up.max())}
        for _ in range(a.warmup):
            for k in fdrs:
                for f in ops.values():
                    f(k)
        ctx.sync()
        t = {(k, o): [] for k in fdrs for o in ops}
        for _ in range(a.steps):
            for k in fdrs:
                for o, f in ops.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(st)
                    f(k)
                    e1.record(st)
                    ctx.sync()
                    t[(k, o)].append(e0.elapsed_time(e1))
    for (k, o), v in t.items():
        stats[k][o + "_ms"] = round(float(np.median(v)), 3)
        stats[k][o + "_ms_min_max"] = [round(min(v), 3), round(max(v), 3)]
    res = {"tool": "watershed_bench", "size": [H, W], "seed": a.seed, "px": px, "steps": a.steps, "warmup": a.warmup,
           "timing": "median of HIP events around each call on its stream, inputs and ops alternating",
           "scratch_bytes": int(L.dt_ctx_scratch_bytes(ctx.h)), "runs": stats, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
