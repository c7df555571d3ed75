"""SAGA wetness index on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by default,
px = 10), in one process: the slope in radians of dt_dev_slope_d8, the catchment area from D8 counts ((fac + 1) * px)
and from the multiple-flow-direction accumulation (mfd.specific_catchment_area), then for each area

  - the whole host-tier call wetness.saga_wetness_index: wall clock, uploads and downloads included (12 B/cell up, 4
    B/cell down), the median of --steps after --warmup, with the rounds, the raised cells and the tile visits per tile;
  - the device time of the three stages on resident rasters, between events (tools/_bench.events):
    dt_dev_wetness_suction, dt_dev_wetness_modified_area with a budget of the host call's rounds + 1 (the quiet one), and
    dt_dev_wetness_index;

and beside them, in the same run, cost.cost_distance with friction 1 from the river network fac > N // 512 (the (min, +)
twin on the same schedule) and a device copy of one float64 raster (8 B/cell read, 8 B/cell written) as the yardstick
of the memory system.  Prints one JSON line (and writes it to --out)."""
import numpy as np

import _bench

TILE = 64
# bytes per cell a stage reads + writes at least: suction 4 + 4; one round over every tile 8 + 4 read (M, s) and up to 8
# written; index 8 + 4 + 4
STAGE_BYTES = {"suction": 8, "round_all_tiles": 20, "index": 16, "copy_f64": 16}


def main(argv=None):
    ap = _bench.parser(steps=3, warmup=1)
    ap.add_argument("--no-mfd", action="store_true", help="skip the MFD area (its accumulation is a host-tier call)")
    a = ap.parse_args(argv)

    import torch
    from descriptools_amd import _lib, cost, mfd, wetness

    H = W = a.size
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        dem_d, fac_d, river_d = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem", "fac", "river"), px).values()
        rad_d = torch.empty((H, W), dtype=torch.float32, device=dev)
        _lib.check(L.dt_dev_slope_d8(ctx.h, dem_d.data_ptr(), H, W, px, None, None, rad_d.data_ptr()))
        ctx.sync()
        dem, river, rad = dem_d.cpu().numpy(), river_d.cpu().numpy(), rad_d.cpu().numpy()
        areas = {"d8": ((fac_d.to(torch.float64) + 1.0) * px).cpu().numpy()}
    del dem_d, fac_d, river_d
    if not a.no_mfd:
        areas["mfd"] = np.ascontiguousarray(mfd.specific_catchment_area(mfd.flow_shares(dem), px), np.float64)
    del dem
    tiles = ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)
    par = (10.0, 1.0, wetness.SLOPE_OFFSET, 0.0)

    res = {"tool": "wetness_bench", "size": [H, W], "seed": a.seed, "px": px, "steps": a.steps, "warmup": a.warmup,
           "parameters": {"t": par[0], "slope_weight": par[1], "slope_offset": par[2], "slope_min": par[3]},
           "tile": [TILE, TILE], "tiles": tiles, "stage_bytes_per_cell": STAGE_BYTES, "areas": {},
           "device": torch.cuda.get_device_name(0)}
    with torch.cuda.stream(st):
        s_d = torch.empty((H, W), dtype=torch.float32, device=dev)
        m_d = torch.empty((H, W), dtype=torch.float64, device=dev)
        w_d = torch.empty((H, W), dtype=torch.float32, device=dev)
        copy_d = torch.empty((H, W), dtype=torch.float64, device=dev)
    for name, area in areas.items():
        def host():
            return wetness.saga_wetness_index(area, rad)

        swi, M = wetness.saga_wetness_index(area, rad, modified=True)
        info = dict(M.info)
        valid = np.asarray(M) > 0
        stats = {"valid_fraction": round(float(valid.mean()), 4),
                 "raised_fraction": round(info["raised"] / max(int(valid.sum()), 1), 4),
                 "area_min_max": [float(area[valid].min()), float(area[valid].max())],
                 "swi_mean": round(float(swi[swi > -100].mean(dtype=np.float64)), 4)}
        del swi, M, valid
        t_host = _bench.timed(host, a.steps, a.warmup)
        budget = min(info["rounds"] + 1, 4096)
        with torch.cuda.stream(st):
            a_d = torch.from_numpy(area).to(dev)
            ctx.sync()
            calls = {
                "suction": lambda: _lib.check(L.dt_dev_wetness_suction(ctx.h, rad_d.data_ptr(), H, W, *par,
                                                                       s_d.data_ptr())),
                "modified_area": lambda: _lib.check(L.dt_dev_wetness_modified_area(
                    ctx.h, a_d.data_ptr(), s_d.data_ptr(), H, W, 0, budget, m_d.data_ptr())),
                "index": lambda: _lib.check(L.dt_dev_wetness_index(ctx.h, m_d.data_ptr(), rad_d.data_ptr(), H, W,
                                                                   par[2], par[3], w_d.data_ptr())),
                "copy_f64": lambda: copy_d.copy_(a_d),
            }
            t_dev = _bench.events(ctx, st, calls, a.steps, a.warmup)
            status = ctx.status()
            del a_d
        ms = {k: _bench.summary(v)[0] for k, v in t_dev.items()}
        res["areas"][name] = dict(
            info, visits_per_tile=round(info["tile_visits"] / tiles, 3), device_budget_rounds=budget,
            device_status=status, **stats,
            host_call_ms=round(_bench.median(t_host), 2), host_call_ms_min_max=_bench.summary(t_host, 2)[1],
            device_ms=ms, device_ms_min_max={k: _bench.summary(v)[1] for k, v in t_dev.items()},
            modified_area_ms_per_round=round(ms["modified_area"] / budget, 4),
            copy_f64_gb_s=round(16.0 * H * W / ms["copy_f64"] * 1e-6, 1))
    del s_d, m_d, w_d, copy_d, rad_d
    ctx.close()
    torch.cuda.empty_cache()

    friction = np.ones((H, W), np.float32)
    cd = {}

    def run_cost():
        out = cost.cost_distance(friction, river, px)
        cd.update(out.info)

    t_cost = _bench.timed(run_cost, a.steps, a.warmup)
    res["cost_distance_friction_1"] = dict(cd, host_call_ms=round(_bench.median(t_cost), 2),
                                           host_call_ms_min_max=_bench.summary(t_cost, 2)[1],
                                           visits_per_tile=round(cd["tile_visits"] / tiles, 3),
                                           host_bytes_per_cell=[4 + 1, 8 + 8])
    res["host_bytes_per_cell"] = {"saga_wetness_index": [8 + 4, 4]}
    res["timing"] = ("host_call_ms: wall clock of the whole host-tier call (uploads, kernels, downloads), "
                     "median; device_ms: between events on resident rasters, median")
    _bench.emit(res, a.out)


if __name__ == "__main__":
    main()
