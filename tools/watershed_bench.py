"""Drainage and upslope length (dt_dev_drainage, dt_dev_upslope_length) at 16384^2 on two inputs: the
benchmark terrain's D8 (dt_dev_synth_dem with bench.py's seed, dt_dev_slope_d8: the chain's fdr) and a rough DEM
conditioned with flowdir.d8_conditioned, whose paths run to the raster edge.  After --warmup runs, each op is timed
--steps times per input, bracketed by HIP events on the context's stream with a sync after each; medians are reported
with the basin count, the longest flow length and the largest upslope length.  Prints one JSON line (and writes it to
--out when given)."""
import numpy as np
import torch

import _bench
from descriptools_amd import _lib, flowdir


def main(argv=None):
    a = _bench.parser(steps=20, warmup=3).parse_args(argv)
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    # the rough DEM: white noise (every cell a pit or a flat neighbour), conditioned on the host tier
    rng = np.random.default_rng(a.seed)
    rough = np.ascontiguousarray(rng.random((H, W), dtype=np.float32) * 100.0)
    fdr_rough = flowdir.d8_conditioned(rough, px)
    del rough
    with torch.cuda.stream(st):
        fdrs = {"terrain": _bench.terrain(ctx, st, dev, a.size, a.seed, ("fdr",), px)["fdr"],
                "conditioned": torch.from_numpy(fdr_rough).to(dev)}
        del fdr_rough
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
        calls = {(k, o): (lambda k=k, f=f: f(k)) for k in fdrs for o, f in ops.items()}
        t = _bench.events(ctx, st, calls, a.steps, a.warmup)
    for (k, o), v in t.items():
        stats[k][o + "_ms"], stats[k][o + "_ms_min_max"] = _bench.summary(v)
    res = {"tool": "watershed_bench", "size": [H, W], "seed": a.seed, "px": px, "steps": a.steps, "warmup": a.warmup,
           "timing": "median of HIP events around each call on its stream, inputs and ops alternating",
           "scratch_bytes": int(L.dt_ctx_scratch_bytes(ctx.h)), "runs": stats, "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
