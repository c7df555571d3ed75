"""Stream order (dt_dev_stream_order) on the benchmark terrain: D8 of dt_dev_synth_dem (bench.py's
seed, 16384^2 by default), flow accumulation, then two networks in one process: the chain's river = fac > N/512 and a
dense one, fac > 1000.  After --warmup runs of each, the two thresholds alternate for --steps runs, each bracketed by
HIP events on the context's stream with a sync after it; medians are reported with the network size M, the number of
junctions (confluence heads), the largest Strahler order and the number of cells on cycles.  Prints one JSON line
(and writes it to --out when given)."""
import torch

import _bench
from descriptools_amd import _lib


def main(argv=None):
    a = _bench.parser(steps=20, warmup=3).parse_args(argv)
    H = W = a.size
    N = H * W
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    thr = {"chain": N // 512, "dense": 1000}
    with torch.cuda.stream(st):
        ter = _bench.terrain(ctx, st, dev, a.size, a.seed, ("fdr", "fac"), fac_nodata=True)
        fdr = ter["fdr"]
        river = {k: (ter["fac"] > v).to(torch.int8) for k, v in thr.items()}
        del ter
        so = torch.empty((H, W), dtype=torch.int8, device=dev)
        sh = torch.empty((H, W), dtype=torch.int64, device=dev)
        lk = torch.empty((H, W), dtype=torch.int64, device=dev)

        def run(k):
            _lib.check(L.dt_dev_stream_order(ctx.h, fdr.data_ptr(), river[k].data_ptr(), H, W, so.data_ptr(),
                                             sh.data_ptr(), lk.data_ptr()))

        stats = {}
        for k in thr:
            run(k)
            ctx.sync()
            flat = torch.arange(N, device=dev)
            net = river[k].view(-1) != 0
            stats[k] = {"threshold": thr[k], "M": int(net.sum()),
                        "junctions": int(((lk.view(-1) == flat) & (sh.view(-1) >= 2)).sum()),
                        "max_order": int(so.max()), "cycle_cells": int((so == -100).sum()),
                        "max_shreve": int(sh.max())}
            del flat, net
        t = _bench.events(ctx, st, {k: (lambda k=k: run(k)) for k in thr}, a.steps, a.warmup)
    for k in thr:
        stats[k]["ms"], stats[k]["ms_min_max"] = _bench.summary(t[k])
    res = {"tool": "stream_order_bench", "size": [H, W], "seed": a.seed, "steps": a.steps, "warmup": a.warmup,
           "timing": "median of HIP events around each dt_dev_stream_order on its stream, thresholds alternating",
           "scratch_bytes": int(L.dt_ctx_scratch_bytes(ctx.h)), "runs": stats, "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
