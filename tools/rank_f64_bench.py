"""The rank-tiled step on float64 heights against its float32 control and the untiled float64 chain.

One process, one GPU, ty x tx LOGICAL ranks of n x n cells each (default 2 x 2 of 8192^2: a 16384^2 global raster).
The float64 DEM is chain_f64_bench's (the benchmark terrain plus sub-float32 structure); the float32 control runs on
that terrain's float32 heights, Chain(heights="float64") on the same global raster.  The ranks run tiling.rank_ops()
stage by stage in lock-step (run_ranks_local's schedule, LocalExchange: the all-gathers become concatenations).

  step_ms     HIP events on rank 0's stream around a whole lock-step step (the ranks' streams are joined to it by
              the LocalExchange synchronisations and a final sync), median of --steps
  per_op_ms   every stage of every rank bracketed by HIP events on that rank's stream, with a sync after each stage
              (no overlap between ranks), summed over the ranks; median of --steps
Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle  # noqa: E402
from chain_f64_bench import dem64_of, time_chain  # noqa: E402
from descriptools_amd import tiling  # noqa: E402


def time_ranks(layout, dem, heights, px, steps, warmup):
    h = tiling.HALO
    thr = (layout.Hg * layout.Wg) // 512
    tiles = []
    for r in range(layout.size):
        t = tiling.RankTile(layout, r, device=0, px=px, river_threshold=thr, tune_placement=False, heights=heights)
        y0, x0 = layout.origin(r)
        ext = np.full((t.He, t.We), -100.0, np.float64 if heights == "float64" else np.float32)
        gy0, gx0 = max(y0 - h, 0), max(x0 - h, 0)
        gy1, gx1 = min(y0 + t.H + h, layout.Hg), min(x0 + t.W + h, layout.Wg)
        ext[gy0 - (y0 - h):gy1 - (y0 - h), gx0 - (x0 - h):gx1 - (x0 - h)] = dem[gy0:gy1, gx0:gx1]
        t.set_dem_ext(ext)
        del ext
        tiles.append(t)
    ex = tiling.LocalExchange(tiles)
    names = [n for n, _ in tiling.RANK_OPS]
    for _ in range(warmup):
        tiling.run_ranks_local(tiles, layout)
    ts0 = tiles[0].ts
    whole = []
    for _ in range(steps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(ts0)
        tiling.run_ranks_local(tiles, layout)
        torch.cuda.synchronize()
        b.record(ts0)
        b.synchronize()
        whole.append(a.elapsed_time(b))
    per = {n: [] for n in names}
    for _ in range(steps):
        ops = [tiling.rank_ops(t, layout, ex) for t in tiles]
        acc = {n: 0.0 for n in names}
        for i, n in enumerate(names):
            for t, o in zip(tiles, ops):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record(t.ts)
                o[i][1]()
                b.record(t.ts)
                t.ctx.sync()
                acc[n] += a.elapsed_time(b)
        for n in names:
            per[n].append(acc[n])
    for t in tiles:
        t.check_status()
        assert t.unresolved_downslope() == 0
    res = {"step_ms": round(float(np.median(whole)), 3),
           "per_op_ms": {n: round(float(np.median(v)), 3) for n, v in per.items()}}
    res["per_op_sum_ms"] = round(sum(res["per_op_ms"].values()), 3)
    for t in tiles:
        t.free()
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=8192, help="rank tile side")
    ap.add_argument("--ty", type=int, default=2)
    ap.add_argument("--tx", type=int, default=2)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert a.steps >= 5
    px = 10.0
    layout = tiling.Layout([a.n] * a.ty, [a.n] * a.tx)
    t0 = time.perf_counter()
    d32 = oracle.synth_dem(1, layout.Hg, layout.Wg)
    d64 = dem64_of(d32)
    t_gen = time.perf_counter() - t0
    r64 = time_ranks(layout, d64, "float64", px, a.steps, a.warmup)
    r32 = time_ranks(layout, d64.astype(np.float32), "float32", px, a.steps, a.warmup)
    del d32
    c64 = time_chain(d64, "float64", px, a.steps, a.warmup)
    c32 = time_chain(d64.astype(np.float32), "float32", px, a.steps, a.warmup)
    out = {
        "tool": "rank_f64_bench", "layout": "%d x %d ranks of %d^2 on one GPU (logical ranks)" % (a.ty, a.tx, a.n),
        "raster": "%dx%d synthetic (oracle.synth_dem seed 1) + sub-float32 structure" % (layout.Hg, layout.Wg),
        "steps": a.steps, "warmup": a.warmup,
        "rank_float64": r64, "rank_float32": r32, "chain_float64": c64, "chain_float32": c32,
        "rank_f64_over_rank_f32": round(r64["per_op_sum_ms"] / r32["per_op_sum_ms"], 3),
        "tiled_over_untiled_f64": round(r64["per_op_sum_ms"] / c64["ms_per_step"], 3),
        "tiled_over_untiled_f32": round(r32["per_op_sum_ms"] / c32["ms_per_step"], 3),
        "dem_gen_s": round(t_gen, 1), "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
