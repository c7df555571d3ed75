"""Harmonic interpolation on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by
default, px = 10) with its river network fac > N // 512, in one process:

* base_level -- the river cells' heights interpolated over the raster -- at tol = 1e-3, 1e-5 and 1e-7: the levels of the
  pyramid, the rounds per level (finest first), the tile visits per tile of the finest level, the wall clock of the
  library call dt_harmonic alone (uploads, kernels, the reads of the residual words, the download) and of the whole
  harmonic.base_level (the argument checks, regions.connected and the numpy passes around it);
* the difference between the tol = 1e-5 and the tol = 1e-7 field on a fixed sample (every 61st cell from (17, 17)): a
  SELF-COMPARISON of two iterates of the same solver, no parity with anything;
* fill_voids on the same terrain with 1 % of its cells knocked out in square blobs of 24 x 24 cells;
* cost.cost_distance with friction 1 over the same sources: the same kind of coloured tile relaxation, for scale;
* the ablation: dt_harmonic at tol = 1e-5 with the pyramid switched off (the environment variable DT_DBG_HARMONIC_LEVELS=1,
  read by the library per call) and the budget capped at --ablation-rounds: the residual it reaches.

Host-tier calls: each time is the median of --steps after --warmup.  The device time comes from a run of its own,
`rocprofv3 --kernel-trace --stats -- python tools/harmonic_bench.py --profile-only` (one base_level at 1e-5, one
fill_voids), summarised by `--trace DIR`: the dispatches are grouped into calls at each k_hm_init; per call the span from
the first launch to the last end and the kernel time split into pyramid (k_hm_init, k_hm_restrict, k_hm_flood, k_hm_start,
k_hm_prolong), smoothing (k_hm_round) and residual (k_hm_residual, k_hm_finish).  Prints one JSON line (and
writes it to --out)."""
import csv
import glob
import json
import os
import time

import numpy as np

import _bench

TILE = 64
GROUPS = {"pyramid": ("k_hm_init", "k_hm_restrict", "k_hm_flood", "k_hm_start", "k_hm_prolong"),
          "smoothing": ("k_hm_round",), "residual": ("k_hm_residual", "k_hm_finish")}


def summarise_trace(d, out_txt):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    calls = []
    for r in rows:
        name, t0, t1 = r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])
        if "k_hm_init" in name:
            calls.append([])
        if "k_hm_" in name and calls:
            calls[-1].append((name, t0, t1))
    lines, summary = [], []
    for i, c in enumerate(calls):
        span = (c[-1][2] - c[0][1]) * 1e-6
        tot = {g: [0, 0] for g in GROUPS}
        for name, t0, t1 in c:
            g = next(g for g, ks in GROUPS.items() if any(k in name for k in ks))
            tot[g][0] += t1 - t0
            tot[g][1] += 1
        summary.append(dict({"span_ms": round(span, 3)},
                            **{g + "_ms": round(a * 1e-6, 3) for g, (a, _) in tot.items()},
                            **{g + "_launches": n for g, (_, n) in tot.items()}))
        lines.append("call %d  first launch to last end %.3f ms | %s" % (
            i, span, " ".join("%s %.3f ms (%d launches)" % (g, a * 1e-6, n) for g, (a, n) in tot.items())))
    text = "\n".join(lines) + "\n"
    if out_txt:
        with open(out_txt, "w") as fh:
            fh.write(text)
    print(text)
    return summary


def knock_out(dem, share, blob, seed):
    """dem with about `share` of its cells set to -100 in blob x blob squares away from the border"""
    rng = np.random.default_rng(seed)
    H, W = dem.shape
    out = dem.copy()
    for _ in range(int(share * H * W / (blob * blob))):
        y, x = int(rng.integers(1, H - blob - 1)), int(rng.integers(1, W - blob - 1))
        out[y:y + blob, x:x + blob] = -100
    return out


def main(argv=None):
    ap = _bench.parser(steps=1, warmup=0)
    ap.add_argument("--profile-only", action="store_true", help="one base_level and one fill_voids (for rocprofv3)")
    ap.add_argument("--trace", default=None, help="summarise the kernel trace under this directory and exit")
    ap.add_argument("--times", default=None, help="with --trace: the text file to write")
    ap.add_argument("--tols", default="1e-3,1e-5,1e-7")
    ap.add_argument("--ablation-rounds", type=int, default=256)
    ap.add_argument("--skip", default="", help="comma-separated: cost, voids, ablation")
    a = ap.parse_args(argv)
    if a.trace:
        summary = summarise_trace(a.trace, a.times)
        if a.out and os.path.exists(a.out):
            res = json.loads(open(a.out).read())
            res["device_by_call"] = summary
            res["device_note"] = "rocprofv3 --kernel-trace run of --profile-only: base_level at 1e-5, then fill_voids"
            _bench.emit(res, a.out, show=False)
        return

    import torch
    from descriptools_amd import _lib, cost, harmonic
    from descriptools_amd._lib import c_f32p, c_f64p, c_i8p, c_i64p, ptr

    H = W = a.size
    px = 10.0
    skip = set(a.skip.split(","))
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        dem_d, river_d = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem", "river"), px).values()
        ctx.sync()
        dem, river = dem_d.cpu().numpy(), river_d.cpu().numpy()
    del dem_d, river_d
    ctx.close()
    torch.cuda.empty_cache()
    tiles = ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)
    holed = knock_out(dem, 0.01, 24, a.seed)
    if a.profile_only:
        harmonic.base_level(dem, river, 1e-5)
        harmonic.fill_voids(holed)
        _bench.emit({"tool": "harmonic_bench", "profile_only": True}, None)
        return

    L = _lib.lib()
    fixed = np.ascontiguousarray(river == 1, np.int8)

    def library(tol, rounds=4096):
        """dt_harmonic alone on prepared arrays (every cell of the terrain is valid and joined to the network)"""
        out = np.empty((H, W), np.float64)
        info = np.zeros(harmonic.INFO_WORDS, np.int64)
        t0 = time.perf_counter()
        _lib.check(L.dt_harmonic(ptr(dem, c_f32p), ptr(fixed, c_i8p), None, H, W, tol, rounds, ptr(out, c_f64p),
                                 ptr(info, c_i64p)))
        return (time.perf_counter() - t0) * 1e3, out, info

    base, sample = {}, {}
    for tol in [float(t) for t in a.tols.split(",")]:
        ms = []
        for i in range(a.warmup + a.steps):
            t, out, info = library(tol)
            if i >= a.warmup:
                ms.append(t)
        levels = int(info[0])
        sample[tol] = out[17::61, 17::61].copy()
        del out
        whole = None  # (harmonic.base_level raises when the budget of 4096 rounds per level runs out)
        if info[5]:
            whole = round(_bench.timed(lambda: harmonic.base_level(dem, river, tol), 1, 0)[0], 2)
        base["%g" % tol] = {"levels": levels, "rounds_per_level": [int(x) for x in info[8:8 + levels]],
                            "rounds_all": int(info[2]), "tile_visits": int(info[3]),
                            "visits_per_finest_tile": round(int(info[3]) / tiles, 3),
                            "residual": float(info[4:5].view(np.float64)[0]), "converged": bool(info[5]),
                            "library_call_ms": round(_bench.median(ms), 2), "base_level_ms": whole}
    res = {"tool": "harmonic_bench", "size": [H, W], "seed": a.seed, "steps": a.steps, "warmup": a.warmup,
           "river_cells": int(fixed.sum()), "tile": [TILE, TILE], "tiles": tiles, "sweeps_per_visit": 4,
           "timing": "wall clock of the whole host-tier call (uploads, kernels, downloads), median",
           "base_level": base, "host_bytes_per_cell": {"dt_harmonic": [4 + 1, 8]},
           "device": torch.cuda.get_device_name(0)}
    if 1e-5 in sample and 1e-7 in sample:
        d = np.abs(sample[1e-5] - sample[1e-7])
        res["self_comparison_1e-5_vs_1e-7"] = {"cells": int(d.size), "max": float(d.max()), "mean": float(d.mean()),
                                               "note": "two iterates of the same solver, not a parity claim"}
    if "voids" not in skip:
        nod = int((holed <= -100).sum())
        t = _bench.timed(lambda: harmonic.fill_voids(holed), a.steps, a.warmup)
        res["fill_voids"] = {"void_cells": nod, "share": round(nod / (H * W), 4), "blob": 24,
                             "ms": round(_bench.median(t), 2)}
    if "cost" not in skip:
        ones = np.ones((H, W), np.float32)
        t = _bench.timed(lambda: cost.cost_distance(ones, river, px), a.steps, a.warmup)
        res["cost_distance_uniform_ms"] = round(_bench.median(t), 2)
        del ones
    if "ablation" not in skip:
        os.environ["DT_DBG_HARMONIC_LEVELS"] = "1"
        try:
            t, out, info = library(1e-5, a.ablation_rounds)
        finally:
            del os.environ["DT_DBG_HARMONIC_LEVELS"]
        res["ablation_no_pyramid"] = {"budget": a.ablation_rounds, "rounds": int(info[1]),
                                      "residual": float(info[4:5].view(np.float64)[0]), "converged": bool(info[5]),
                                      "tile_visits": int(info[3]), "library_call_ms": round(t, 2)}
    _bench.emit(res, a.out)


if __name__ == "__main__":
    main()
