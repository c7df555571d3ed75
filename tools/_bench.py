"""What the op benchmark tools (tools/*_bench.py) share: the common options, the device, the benchmark terrain, the two
ways this project times one call, the summary of a list of times and the JSON line at the end.  Importing it makes the
package importable from a checkout, so a tool imports it before descriptools_amd."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

from descriptools_amd import _lib  # noqa: E402
from descriptools_amd.device import Context  # noqa: E402


def parser(steps, warmup):
    """the options every tool takes; the tool adds its own"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=steps)
    ap.add_argument("--warmup", type=int, default=warmup)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    return ap


def device():
    """(ctx, stream, device): a context of the package on a torch stream of its own on GPU 0"""
    import torch
    st = torch.cuda.Stream()
    return Context(0, st.cuda_stream), st, torch.device("cuda", 0)


def terrain(ctx, stream, dev, size, seed, want, px=10.0, fac_nodata=False):
    """The benchmark terrain, size x size on the device, as a dict of the rasters named in `want`: "dem"
    (dt_dev_synth_dem with bench.py's arguments), "fdr" and "slope" (dt_dev_slope_d8), "fac" (dt_dev_flowacc, int32; the
    DEM as its nodata raster with fac_nodata), "river" (int8, fac > N // 512: bench.py's threshold) and "hand"
    (dt_dev_flowhand, the flow-path HAND alone).  Only what `want` needs is computed, in that order, and the rest is
    freed on return."""
    import torch
    H = W = size
    L = _lib.lib()
    r = {}
    with torch.cuda.stream(stream):
        def empty(dtype):
            return torch.empty((H, W), dtype=dtype, device=dev)

        r["dem"] = empty(torch.float32)
        _lib.check(L.dt_dev_synth_dem(ctx.h, seed, H, W, 0, 0, H, W, 0, r["dem"].data_ptr()))
        if set(want) - {"dem"}:
            r["fdr"], r["slope"] = empty(torch.uint8), empty(torch.float32)
            _lib.check(L.dt_dev_slope_d8(ctx.h, r["dem"].data_ptr(), H, W, px, r["slope"].data_ptr(),
                                         r["fdr"].data_ptr(), None))
        if set(want) & {"fac", "river", "hand"}:
            r["fac"] = empty(torch.int32)
            _lib.check(L.dt_dev_flowacc(ctx.h, r["fdr"].data_ptr(), r["dem"].data_ptr() if fac_nodata else None, H, W,
                                        r["fac"].data_ptr()))
            ctx.sync()
        if set(want) & {"river", "hand"}:
            r["river"] = (r["fac"] > (H * W) // 512).to(torch.int8)
        if "hand" in want:
            r["hand"] = empty(torch.float32)
            _lib.check(L.dt_dev_flowhand(ctx.h, r["dem"].data_ptr(), r["fdr"].data_ptr(), r["river"].data_ptr(), None,
                                         H, W, px, None, None, r["hand"].data_ptr(), None))
            ctx.sync()
    return {k: r[k] for k in want}


def events(ctx, stream, calls, steps, warmup):
    """Device time of the named calls -> {name: [ms] * steps}.  After `warmup` rounds of every call and a sync, each
    call of each step sits between two timing events on the context's stream with a sync after it, the calls
    alternating inside a step."""
    import torch
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    ctx.sync()
    t = {name: [] for name in calls}
    for _ in range(steps):
        for name, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            fn()
            e1.record(stream)
            ctx.sync()
            t[name].append(e0.elapsed_time(e1))
    return t


def timed(fn, steps, warmup):
    """Wall clock of a host-tier call (it synchronises before it returns) -> [ms] * steps, after `warmup` calls"""
    for _ in range(warmup):
        fn()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return t


def median(ms):
    return float(np.median(ms))


def summary(ms, places=3):
    """(median, [min, max]) of a list of times, rounded"""
    return round(median(ms), places), [round(min(ms), places), round(max(ms), places)]


def emit(res, out, show=True):
    """print the result as one JSON line (with show) and write it to the file `out` when there is one"""
    line = json.dumps(res)
    if show:
        print(line)
    if out:
        with open(out, "w") as f:
            f.write(line + "\n")
