"""Cost distance beside the straight-line and the D-infinity distance to the same river network, in
one process: the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by default, px = 10), its river network
fac > N // 512, then cost.cost_distance over a uniform friction (1 everywhere: the geodesic distance) and over a
slope-derived one (1 + 10 * min(slope, 5)), proximity.nearest_river and dinf.distance_down (stat 'ave', no heights) on
the angles of dt_dev_dinf_direction.

These are host-tier calls: each time is the wall clock of the whole call, uploads and downloads included (5 B/cell up
and 16 B/cell down for cost_distance), the median of --steps after --warmup; every call synchronises before it returns.
For each friction the tool records the rounds that lowered something, the reached cells and the tile visits per tile.

The device time comes from a second run of its own, `rocprofv3 --kernel-trace --stats -- python
tools/cost_distance_bench.py --profile-only` (one call of each op), summarised by `--trace DIR`: the dispatches are
grouped into calls at each k_cost_init, per call the span from the first launch to the last end, each kernel's total and
the share of the allocation (k_cost_jump and k_cost_index); the kernels of nearest_river (k_px_*) and of distance_down
(k_dd_*) beside them.  Prints one JSON line (and writes it to --out)."""
import csv
import glob
import json
import os

import numpy as np

import _bench

TILE = 64
KERNELS = ("k_cost_init", "k_cost_round", "k_cost_link", "k_cost_fill", "k_cost_jump", "k_cost_index")


def summarise_trace(d, out_txt):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    ker = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
    calls = []
    for name, t0, t1 in ker:
        if "k_cost_init" in name:
            calls.append([])
        if "k_cost_" in name and calls:
            calls[-1].append((name, t0, t1))
    lines, summary = [], []
    for i, c in enumerate(calls):
        span = (c[-1][2] - c[0][1]) * 1e-6
        tot = {k: [0, 0] for k in KERNELS}
        for name, t0, t1 in c:
            k = next(k for k in KERNELS if k in name)
            tot[k][0] += t1 - t0
            tot[k][1] += 1
        busy = sum(a for a, _ in tot.values()) * 1e-6
        alloc = (tot["k_cost_jump"][0] + tot["k_cost_index"][0]) * 1e-6
        summary.append({"span_ms": round(span, 3), "kernel_ms": round(busy, 3), "allocation_ms": round(alloc, 3),
                        "allocation_share": round(alloc / busy, 4) if busy else 0.0,
                        "round_launches": tot["k_cost_round"][1]})
        lines.append("call %d  first launch to last end %.3f ms, kernels %.3f ms, allocation %.3f ms | %s" % (
            i, span, busy, alloc, " ".join("%s %.3f (%d)" % (k, a * 1e-6, n) for k, (a, n) in tot.items())))
    for tag, pat in (("nearest_river kernels (k_px_*)", "k_px_"), ("distance_down kernels (k_dd_*)", "k_dd_")):
        tot = sum(t1 - t0 for name, t0, t1 in ker if pat in name)
        lines.append("%s in all: %.3f ms" % (tag, tot * 1e-6))
        summary.append({"kernels": pat + "*", "kernel_ms": round(tot * 1e-6, 3)})
    text = "\n".join(lines) + "\n"
    if out_txt:
        with open(out_txt, "w") as fh:
            fh.write(text)
    print(text)
    return summary


def main(argv=None):
    ap = _bench.parser(steps=3, warmup=1)
    ap.add_argument("--profile-only", action="store_true", help="one call of each op and nothing else (for rocprofv3)")
    ap.add_argument("--trace", default=None, help="summarise the kernel trace under this directory and exit")
    ap.add_argument("--times", default=None, help="with --trace: the text file to write")
    a = ap.parse_args(argv)
    if a.trace:
        summary = summarise_trace(a.trace, a.times)
        if a.out and os.path.exists(a.out):
            res = json.loads(open(a.out).read())
            res["device_by_call"] = summary
            res["device_note"] = ("rocprofv3 --kernel-trace run of --profile-only: calls in the order uniform, slope "
                                  "friction; then the kernels of nearest_river and distance_down in all")
            _bench.emit(res, a.out, show=False)
        return

    import torch
    from descriptools_amd import _lib, cost, dinf, proximity

    H = W = a.size
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        dem_d, slope_d, river_d = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem", "slope", "river"), px).values()
        angle_d = torch.empty((H, W), dtype=torch.float32, device=dev)
        _lib.check(L.dt_dev_dinf_direction(ctx.h, dem_d.data_ptr(), None, H, W, px, angle_d.data_ptr(), None))
        ctx.sync()
        slope, river, angle = slope_d.cpu().numpy(), river_d.cpu().numpy(), angle_d.cpu().numpy()
    del dem_d, slope_d, river_d, angle_d
    ctx.close()
    torch.cuda.empty_cache()

    frictions = {"uniform": np.ones((H, W), np.float32),
                 "slope": (1 + 10 * np.clip(np.nan_to_num(slope, nan=0.0), 0, 5)).astype(np.float32)}
    del slope
    tiles = ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)
    modes = {}

    def run(kind):
        out = cost.cost_distance(frictions[kind], river, px)
        modes[kind] = dict(out.info, reached_fraction=round(out.info["reached"] / (H * W), 4),
                           visits_per_tile=round(out.info["tile_visits"] / tiles, 3))
        return out

    ops = (("cost_distance_uniform", lambda: run("uniform")),
           ("cost_distance_slope", lambda: run("slope")),
           ("nearest_river", lambda: proximity.nearest_river(river, px)),
           ("dinf_distance_down", lambda: dinf.distance_down(angle, river, px)))
    if a.profile_only:
        for _, fn in ops:
            fn()
        _bench.emit({"tool": "cost_distance_bench", "profile_only": True, "modes": modes}, None)
        return
    t = {name: _bench.timed(fn, a.steps, a.warmup) for name, fn in ops}
    res = {"tool": "cost_distance_bench", "size": [H, W], "seed": a.seed, "px": px, "connectivity": 8,
           "steps": a.steps, "warmup": a.warmup,
           "timing": "wall clock of the whole host-tier call (uploads, kernels, downloads), median",
           "river_cells": int(river.sum()),
           "ms": {k: round(_bench.median(v), 2) for k, v in t.items()},
           "ms_min_max": {k: _bench.summary(v, 2)[1] for k, v in t.items()},
           "modes": modes, "tile": [TILE, TILE], "tiles": tiles,
           "host_bytes_per_cell": {"cost_distance": [4 + 1, 8 + 8], "nearest_river": [1, 4 + 8],
                                   "dinf_distance_down": [4 + 1, 8]},
           "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)


if __name__ == "__main__":
    main()
