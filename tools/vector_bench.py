"""Vector rasterisation on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by
default, px = 10), in one process, device time between events on resident arrays (tools/_bench.events):

  - hand_le3_runs    the extent hand <= 3 as one polygon: a rectangle per run of cells of a row, all of one id, so the
                     even-odd rule over millions of rings gives the mask back (checked: `exact`);
  - small_polygons   10^5 random hexagons of radius 2 to 40 cells, each its own id;
  - river_lines_8 / river_lines_4   the bench river network as polylines, a segment from every river cell's centre to
                     the centre of the cell its D8 code points at, at both connectivities (at 8 the label's extent is
                     the river raster again: `exact`);
  - points           10^6 random points.

Each case is timed beside a device copy of the label raster's 4 bytes per cell in the same run, the two alternating
inside a step: that copy is the yardstick, `ratio` = case / copy.  The phases (clear, count, scan, emit, sort, fill,
lines / points) come from dt_dev_rasterize_timed, which records an event between them; `info` is the call's own count
(crossings, the most on one row, rows sorted in global memory, overflow).

Polygonisation (--polygonize, a comma-separated list, empty to skip) takes label rasters off the grid
again with dt_dev_polygonize: `extent` (hand <= 3 as a mask), `landform` (horizon.geomorphons), `basins`
(zonal.compact(watershed.basins)) and `checkerboard` (two labels, every cell its own ring: 4 edges per cell, the most a
raster can have).  A first call with capacities 0 is the count; the timed calls get the exact capacities.  Each case
alternates with a device copy of the int32 label raster and with dt_dev_rasterize of the rings just produced, the round
trip's other half, whose label must equal the input (`exact`).  The phases (count, link, leaders, ranks, rings, emit,
shells) come from dt_dev_polygonize_timed; `info` holds the call's counts and rounds.  --skip-rasterize leaves the
rasterisation cases out.  Prints one JSON line (and writes it to --out)."""
import ctypes as C

import _bench

PHASES = ("clear", "count", "scan", "emit", "sort", "fill", "lines")
PG_PHASES = ("count", "link", "leaders", "ranks", "rings", "emit", "shells")
PG_INFO = ("edges", "vertices", "rings", "holes", "rounds", "overflow", "rank_rounds", "shell_rounds")
# dx, dy of the D8 codes 1 2 4 8 16 32 64 128 (E SE S SW W NW N NE)
D8_DX = (1, 1, 0, -1, -1, -1, 0, 1)
D8_DY = (0, 1, 1, 1, 0, -1, -1, -1)


def polygonize_case(ctx, st, dev, L, lab, steps, warmup):
    """one label raster (int32 on the device) through dt_dev_polygonize, beside its copy and the way back"""
    import torch
    from descriptools_amd import _lib
    H, W = lab.shape
    info = torch.zeros(8, dtype=torch.int64, device=dev)
    none = torch.zeros(2, dtype=torch.int64, device=dev)
    _lib.check(L.dt_dev_polygonize(ctx.h, lab.data_ptr(), H, W, 0, 0, 0, none.data_ptr(), none.data_ptr(),
                                   none.data_ptr(), none.data_ptr(), info.data_ptr()))     # capacities 0: the count
    ctx.sync()
    E, V = info[:2].tolist()
    if E >= 2 ** 31:
        return {"edges": E, "vertices": V, "skipped": "2^31 directed edges or more"}
    R = V // 4
    coords = torch.empty((max(V, 1), 2), dtype=torch.float64, device=dev)
    parts = torch.empty(R + 1, dtype=torch.int64, device=dev)
    ids, shell = (torch.empty(max(R, 1), dtype=torch.int32, device=dev) for _ in range(2))
    back, dst = torch.empty_like(lab), torch.empty_like(lab)
    rinfo = torch.zeros(4, dtype=torch.int64, device=dev)
    args = (ctx.h, lab.data_ptr(), H, W, E, V, R, coords.data_ptr(), parts.data_ptr(), ids.data_ptr(), shell.data_ptr(),
            info.data_ptr())
    _lib.check(L.dt_dev_polygonize(*args))
    ctx.sync()
    counts = dict(zip(PG_INFO, info.tolist()))
    P = counts["rings"]
    # every crossing of a row's centre line is one vertical unit edge: the edges bound the rasteriser's capacity
    rargs = (ctx.h, 0, coords.data_ptr(), parts.data_ptr(), ids.data_ptr(), P, V, H, W, 8, 0, E, back.data_ptr(),
             rinfo.data_ptr())
    calls = {"polygonize": lambda: _lib.check(L.dt_dev_polygonize(*args)), "copy": lambda: dst.copy_(lab),
             "rasterize": lambda: _lib.check(L.dt_dev_rasterize(*rargs))}
    tm = _bench.events(ctx, st, calls, steps, warmup)
    per_phase = []
    for _ in range(steps):
        out = (C.c_double * 7)()
        _lib.check(L.dt_dev_polygonize_timed(*args, out))
        per_phase.append(list(out))
    ctx.sync()
    ms, ms_copy, ms_back = (_bench.summary(tm[k]) for k in ("polygonize", "copy", "rasterize"))
    return {"info": counts, "ms": ms[0], "ms_min_max": ms[1], "copy_ms": ms_copy[0], "copy_ms_min_max": ms_copy[1],
            "ratio": round(ms[0] / ms_copy[0], 2), "rasterize_ms": ms_back[0], "rasterize_ms_min_max": ms_back[1],
            "rasterize_info": dict(zip(("crossings", "largest_row", "slow_rows", "overflow"), rinfo.tolist())),
            "exact": bool(torch.equal(back, torch.where(lab >= 0, lab, -1))),
            "scratch_bytes": int(L.dt_ctx_scratch_bytes(ctx.h)),
            "phase_ms": {p: round(_bench.median([s[k] for s in per_phase]), 3) for k, p in enumerate(PG_PHASES)}}


def main(argv=None):
    ap = _bench.parser(steps=5, warmup=2)
    ap.add_argument("--polygons", type=int, default=100000)
    ap.add_argument("--points", type=int, default=1000000)
    ap.add_argument("--polygonize", default="extent,landform,basins,checkerboard")
    ap.add_argument("--skip-rasterize", action="store_true")
    a = ap.parse_args(argv)

    import numpy as np
    import torch
    from descriptools_amd import _lib

    S = a.size
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    res = {"tool": "vector_bench", "size": [S, S], "seed": a.seed, "steps": a.steps, "warmup": a.warmup, "cases": {},
           "device": torch.cuda.get_device_name(0)}

    with torch.cuda.stream(st):
        pg_cases = [c for c in a.polygonize.split(",") if c]
        t = _bench.terrain(ctx, st, dev, S, a.seed, ("dem", "fdr", "river", "hand"))
        wet = (t["hand"] <= 3.0) & (t["hand"] > -100.0)
        river, fdr = t["river"] != 0, t["fdr"]
        dem_host = t["dem"].cpu().numpy() if "landform" in pg_cases else None
        del t

        # a rectangle per run of wet cells of a row, in row-major order
        first, last = wet.clone(), wet.clone()
        first[:, 1:] &= ~wet[:, :-1]
        last[:, :-1] &= ~wet[:, 1:]
        r0, c0 = first.nonzero(as_tuple=True)
        _, c1 = last.nonzero(as_tuple=True)
        del first, last
        x0, x1, y0 = c0.double(), (c1 + 1).double(), r0.double()
        runs = torch.stack((torch.stack((x0, y0), 1), torch.stack((x1, y0), 1), torch.stack((x1, y0 + 1), 1),
                            torch.stack((x0, y0 + 1), 1)), 1).reshape(-1, 2).contiguous()
        n_runs = int(r0.numel())
        del r0, c0, c1, x0, x1, y0
        run_parts = torch.arange(0, 4 * n_runs + 1, 4, dtype=torch.int64, device=dev)
        run_ids = torch.zeros(n_runs, dtype=torch.int32, device=dev)

        rng = np.random.default_rng(a.seed)
        ang = np.sort(rng.uniform(0.0, 2.0 * np.pi, (a.polygons, 6)), axis=1)
        rad = rng.uniform(2.0, 40.0, (a.polygons, 6))
        ctr = rng.uniform(0.0, S, (a.polygons, 1, 2))
        poly_host = (ctr + np.stack((rad * np.cos(ang), rad * np.sin(ang)), axis=2)).reshape(-1, 2)
        poly_parts_host = np.arange(0, 6 * a.polygons + 1, 6, dtype=np.int64)
        total, largest = C.c_int64(0), C.c_int64(0)
        _lib.check(L.dt_rasterize_count(0, _lib.ptr(poly_host, _lib.c_f64p), _lib.ptr(poly_parts_host, _lib.c_i64p),
                                        a.polygons, S, S, C.byref(total), C.byref(largest)))
        polys = torch.from_numpy(poly_host).to(dev)
        poly_parts = torch.from_numpy(poly_parts_host).to(dev)
        poly_ids = torch.arange(a.polygons, dtype=torch.int32, device=dev)

        rr, rc = river.nonzero(as_tuple=True)
        code = fdr[rr, rc].long()
        bit = torch.where(code > 0, torch.log2(code.double().clamp(min=1.0)).long(), torch.zeros_like(code))
        pow2 = (code > 0) & ((code & (code - 1)) == 0)
        dx = torch.tensor(D8_DX, device=dev)[bit] * pow2
        dy = torch.tensor(D8_DY, device=dev)[bit] * pow2
        a_xy = torch.stack((rc.double() + 0.5, rr.double() + 0.5), 1)
        b_xy = torch.stack(((rc + dx).double() + 0.5, (rr + dy).double() + 0.5), 1)
        segs = torch.stack((a_xy, b_xy), 1).reshape(-1, 2).contiguous()
        n_segs = int(rr.numel())
        seg_parts = torch.arange(0, 2 * n_segs + 1, 2, dtype=torch.int64, device=dev)
        seg_ids = torch.zeros(n_segs, dtype=torch.int32, device=dev)
        del rr, rc, code, bit, pow2, dx, dy, a_xy, b_xy

        pts = torch.from_numpy(rng.uniform(0.0, S, (a.points, 2))).to(dev)
        pt_parts = torch.tensor([0, a.points], dtype=torch.int64, device=dev)
        pt_ids = torch.zeros(1, dtype=torch.int32, device=dev)

        label = torch.empty((S, S), dtype=torch.int32, device=dev)
        c_src, c_dst = torch.zeros_like(label), torch.empty_like(label)
        info = torch.zeros(4, dtype=torch.int64, device=dev)
        ctx.sync()

        cases = [("hand_le3_runs", 0, runs, run_parts, run_ids, 8, 2 * n_runs, wet),
                 ("small_polygons", 0, polys, poly_parts, poly_ids, 8, total.value, None),
                 ("river_lines_8", 1, segs, seg_parts, seg_ids, 8, 0, river),
                 ("river_lines_4", 1, segs, seg_parts, seg_ids, 4, 0, None),
                 ("points", 2, pts, pt_parts, pt_ids, 8, 0, None)]
        for name, kind, xy, parts, ids, conn, capacity, truth in ([] if a.skip_rasterize else cases):
            args = (ctx.h, kind, xy.data_ptr(), parts.data_ptr(), ids.data_ptr(), ids.numel(), xy.shape[0], S, S, conn, 0,
                    capacity, label.data_ptr(), info.data_ptr())
            calls = {"case": lambda: _lib.check(L.dt_dev_rasterize(*args)), "copy": lambda: c_dst.copy_(c_src)}
            tm = _bench.events(ctx, st, calls, a.steps, a.warmup)
            ms, ms_copy = _bench.summary(tm["case"]), _bench.summary(tm["copy"])
            per_phase = []
            for _ in range(a.steps):
                out = (C.c_double * 7)()
                _lib.check(L.dt_dev_rasterize_timed(*args, out))
                per_phase.append(list(out))
            ctx.sync()
            c = {"kind": ("polygon", "line", "point")[kind], "connectivity": conn, "vertices": int(xy.shape[0]),
                 "parts": int(ids.numel()), "capacity": int(capacity),
                 "info": dict(zip(("crossings", "largest_row", "slow_rows", "overflow"), info.tolist())),
                 "burnt_cells": int((label >= 0).sum()), "ms": ms[0], "ms_min_max": ms[1], "copy_ms": ms_copy[0],
                 "copy_ms_min_max": ms_copy[1], "ratio": round(ms[0] / ms_copy[0], 2),
                 "phase_ms": {p: round(_bench.median([s[k] for s in per_phase]), 3) for k, p in enumerate(PHASES)}}
            if truth is not None:
                c["exact"] = bool(torch.equal(label >= 0, truth))
            res["cases"][name] = c
        del runs, run_parts, run_ids, polys, poly_parts, poly_ids, segs, seg_parts, seg_ids, pts, c_src, c_dst
        res["polygonize"] = {}
        for name in pg_cases:
            if name == "extent":
                lab = torch.where(wet, 1, -1).to(torch.int32)
            elif name == "checkerboard":
                k = torch.arange(S, device=dev, dtype=torch.int32)
                lab = ((k[:, None] + k[None, :]) & 1).contiguous()
            elif name == "landform":
                from descriptools_amd import horizon
                lab = torch.from_numpy(horizon.geomorphons(dem_host, 10.0).astype(np.int32)).to(dev)
            elif name == "basins":
                from descriptools_amd import watershed, zonal
                lab = torch.from_numpy(np.ascontiguousarray(zonal.compact(watershed.basins(fdr.cpu().numpy())).zones)).to(dev)
            else:
                raise SystemExit("unknown polygonize case %r" % name)
            res["polygonize"][name] = polygonize_case(ctx, st, dev, L, lab, a.steps, a.warmup)
            del lab
        status = ctx.status()
    res["device_status"] = status
    res["timing"] = ("device time between events on resident arrays, median of --steps after --warmup; copy: a device "
                     "copy of the label raster's 4 bytes per cell, timed alternately with the case; phase_ms: events "
                     "recorded between the phases of one call (dt_dev_rasterize_timed, dt_dev_polygonize_timed); "
                     "polygonize: rasterize_ms is dt_dev_rasterize of the rings just produced, timed in the same steps")
    ctx.close()
    _bench.emit(res, a.out)


if __name__ == "__main__":
    main()
