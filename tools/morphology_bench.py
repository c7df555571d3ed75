"""Geodesic reconstruction on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by
default), in one process: for fill, hminima(0.5), regional_minima and opening_by_reconstruction(16)

  - the whole host-tier call: wall clock, uploads and downloads included (4 B/cell up, 4 or 1 B/cell down), the median
    of --steps after --warmup, with the rounds, the changed cells and the tile visits per tile;
  - the device time of dt_dev_morph_reconstruct on resident rasters, between events (tools/_bench.events), with a budget
    of the host call's rounds + 1 (the quiet one);

and beside them, in the same run, a device copy of one float32 raster (4 B/cell read, 4 B/cell written: the algorithmic
bytes of an op that reads the DEM once and writes its result once) and dt_dev_condition_d8_async on the same DEM -- the
fill, D8 and flat phases of the conditioning together (the C ABI does not run its fill phase alone: the figure is an
upper bound of it), with the fill and flat rounds dt_dev_condition_d8 reports.  Prints one JSON line (and writes it to
--out)."""
import numpy as np

import _bench

TILE = 64
MARKER, SHIFT, STEP, OUTLETS, WINDOW = range(5)  # DT_MORPH_*


def main(argv=None):
    ap = _bench.parser(steps=3, warmup=1)
    a = ap.parse_args(argv)

    import torch
    from descriptools_amd import _lib, morphology

    H = W = a.size
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        dem_d = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem",), px)["dem"]
        ctx.sync()
        dem = dem_d.cpu().numpy()
    tiles = ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)
    # name -> (the host-tier call, (mode, erosion, h, radius, uint8 output))
    ops = {"fill": (lambda: morphology.fill(dem), (OUTLETS, 1, 0.0, 0, False)),
           "hminima_0.5": (lambda: morphology.hminima(dem, 0.5), (SHIFT, 1, 0.5, 0, False)),
           "regional_minima": (lambda: morphology.regional_minima(dem), (STEP, 1, 0.0, 0, True)),
           "opening_by_reconstruction_16": (lambda: morphology.opening_by_reconstruction(dem, 16),
                                            (WINDOW, 0, 0.0, 16, False))}
    res = {"tool": "morphology_bench", "size": [H, W], "seed": a.seed, "steps": a.steps, "warmup": a.warmup,
           "tile": [TILE, TILE], "tiles": tiles, "ops": {}, "device": torch.cuda.get_device_name(0)}
    valid = int((np.isfinite(dem) & (dem > -100)).sum())
    with torch.cuda.stream(st):
        out_d = torch.empty((H, W), dtype=torch.float32, device=dev)
        out8_d = torch.empty((H, W), dtype=torch.uint8, device=dev)
        copy_d = torch.empty((H, W), dtype=torch.float32, device=dev)
        fdr_d = torch.empty((H, W), dtype=torch.uint8, device=dev)
    infos, budgets, calls = {}, {}, {}
    for name, (host, (mode, erosion, h, radius, u8)) in ops.items():
        if name == "regional_minima":  # a plain ndarray: the counts come from the C entry
            info4 = np.zeros(4, np.int64)
            o8 = np.empty((H, W), np.uint8)
            _lib.check(L.dt_morph_reconstruct(mode, erosion, 8, _lib.ptr(dem, _lib.c_f32p), None, None, h, radius, H, W,
                                              0, None, _lib.ptr(o8, _lib.c_u8p), _lib.ptr(info4, _lib.c_i64p)))
            info = {"rounds": int(info4[0]), "changed": int(info4[1]), "tile_visits": int(info4[2]),
                    "minima_cells": int(o8.sum())}
            del o8
        else:
            r = host()
            info = dict(r.info)
            if name == "fill":
                info["raised_fraction"] = round(float((np.asarray(r) > dem).sum()) / max(valid, 1), 4)
            del r
        infos[name] = info
        budgets[name] = min(info["rounds"] + 1, 4096)
        t_host = _bench.timed(host, a.steps, a.warmup)
        info["host_call_ms"] = round(_bench.median(t_host), 2)
        info["host_call_ms_min_max"] = _bench.summary(t_host, 2)[1]

        def dev_call(mode=mode, erosion=erosion, h=h, radius=radius, u8=u8, budget=budgets[name]):
            _lib.check(L.dt_dev_morph_reconstruct(ctx.h, mode, erosion, 8, dem_d.data_ptr(), None, None, h, radius, H, W,
                                                  0, budget, None if u8 else out_d.data_ptr(),
                                                  out8_d.data_ptr() if u8 else None))
        calls[name] = dev_call
    info3 = np.zeros(3, np.int32)
    with torch.cuda.stream(st):
        _lib.check(L.dt_dev_condition_d8(ctx.h, dem_d.data_ptr(), H, W, px, out_d.data_ptr(), fdr_d.data_ptr(),
                                         info3.ctypes.data_as(_lib.c_i32p)))
        cond_budget = int(min(max(info3[1], info3[2]) + 1, 500))
        calls["condition_d8_async"] = lambda: _lib.check(L.dt_dev_condition_d8_async(
            ctx.h, dem_d.data_ptr(), H, W, px, out_d.data_ptr(), fdr_d.data_ptr(), cond_budget))
        calls["copy_f32"] = lambda: copy_d.copy_(dem_d)
        t_dev = _bench.events(ctx, st, calls, a.steps, a.warmup)
        status = ctx.status()
    for name in ops:
        ms, mm = _bench.summary(t_dev[name])
        res["ops"][name] = dict(infos[name], visits_per_tile=round(infos[name]["tile_visits"] / tiles, 3),
                                device_budget_rounds=budgets[name], device_ms=ms, device_ms_min_max=mm,
                                device_ms_per_round=round(ms / budgets[name], 4))
    ms_copy, mm_copy = _bench.summary(t_dev["copy_f32"])
    ms_cond, mm_cond = _bench.summary(t_dev["condition_d8_async"])
    res["copy_f32"] = {"device_ms": ms_copy, "device_ms_min_max": mm_copy,
                       "gb_s": round(8.0 * H * W / ms_copy * 1e-6, 1)}
    res["condition_d8_async"] = {"device_ms": ms_cond, "device_ms_min_max": mm_cond, "budget_rounds": cond_budget,
                                 "fill_rounds": int(info3[1]), "flat_rounds": int(info3[2]),
                                 "phases": "fill, D8 and flats together: an upper bound of the fill phase"}
    res["valid_cells"] = valid
    res["device_status"] = status
    res["timing"] = ("host_call_ms: wall clock of the whole host-tier call (uploads, kernels, downloads), median; "
                     "device_ms: between events on resident rasters, median")
    ctx.close()
    _bench.emit(res, a.out)


if __name__ == "__main__":
    main()
