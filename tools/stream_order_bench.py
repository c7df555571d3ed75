"""Stream order (dt_dev_stream_order) on the benchmark terrain: D8 of dt_dev_synth_dem (bench.py's
seed, 16384^2 by default), flow accumulation, then two networks in one process: the chain's river = fac > N/512 and a
dense one, fac > 1000.  After --warmup runs of each, the two thresholds alternate for --steps runs, each bracketed by
HIP events on the context's stream with a sync after it; medians are reported with the network size M, the number of
junctions (confluence heads), the largest Strahler order and the number of cells on cycles.  Prints one JSON line
(and writes it to --out when given)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from descriptools_amd import _lib  # noqa: E402
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
    L = _lib.lib()
    st = torch.cuda.Stream()
    ctx = Context(0, st.cuda_stream)
    dev = torch.device("cuda", 0)
    thr = {"chain": N // 512, "dense": 1000}
    with torch.cuda.stream(st):
        dem = torch.empty((H, W), dtype=torch.float32, device=dev)
        fdr = torch.empty((H, W), dtype=torch.uint8, device=dev)
        slope = torch.empty((H, W), dtype=torch.float32, device=dev)
        acc = torch.empty((H, W), dtype=torch.int32, device=dev)
        _lib.check(L.dt_dev_synth_dem(ctx.h, a.seed, H, W, 0, 0, H, W, 0, dem.data_ptr()))
        _lib.check(L.dt_dev_slope_d8(ctx.h, dem.data_ptr(), H, W, 10.0, slope.data_ptr(), fdr.data_ptr(), None))
        _lib.check(L.dt_dev_flowacc(ctx.h, fdr.data_ptr(), dem.data_ptr(), H, W, acc.data_ptr()))
        del slope, dem
        river = {k: (acc > v).to(torch.int8) for k, v in thr.items()}
        del acc
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
        for _ in range(a.warmup):
            for k in thr:
                run(k)
        ctx.sync()
        t = {k: [] for k in thr}
        for _ in range(a.steps):
            for k in thr:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                run(k)
                e1.record(st)
                ctx.sync()
                t[k].append(e0.elapsed_time(e1))
    for k in thr:
        stats[k]["ms"] = round(float(np.median(t[k])), 3)
        stats[k]["ms_min_max"] = [round(min(t[k]), 3), round(max(t[k]), 3)]
    res = {"tool": "stream_order_bench", "size": [H, W], "seed": a.seed, "steps": a.steps, "warmup": a.warmup,
           "timing": "median of HIP events around each dt_dev_stream_order on its stream, thresholds alternating",
           "scratch_bytes": int(L.dt_ctx_scratch_bytes(ctx.h)), "runs": stats, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
