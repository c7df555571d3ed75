"""Zonal statistics (dt_dev_zonal_*) on the benchmark terrain (dt_dev_synth_dem with bench.py's seed,
16384^2 by default), on a resident chain's rasters, in one process, on one stream.  The values are the chain's HAND
(float32).  dt_dev_zonal_tables is timed with count + s1 alone and with every accumulator, on zones from four sources:
the landform classes of dt_dev_horizon (the direct LDS table), the chain's reach catchments, the drainage basins of
dt_dev_drainage made dense by dt_dev_zonal_compact, and a random zone per cell out of 2^20 (the worst case for the LDS
table).  Beside each: the same call without the LDS table (DT_DBG_RC_SLOTS = -1), and once a device copy of the same
algorithmic bytes (a 4-byte zone and a 4-byte value per cell).  dt_dev_zonal_compact is timed on the basins and on
dt_dev_regions_label of 0 <= hand <= 3 (both int64 flat indices) beside a copy of 12 bytes per cell (8 read, 4
written), dt_dev_zonal_counts at K = 64 and K = 1024 bins on the catchments, and dt_dev_zonal_paint of a float32 table
on the catchments (4 bytes read, 4 written per cell: the first copy's bytes).

The ops alternate, each bracketed by HIP events with a sync after it; medians of --steps are reported with the rate
their algorithmic bytes give.  Prints one JSON line (and writes it to --out when given)."""
import ctypes as C

import numpy as np
import torch

import _bench
from descriptools_amd import _lib, chain

DT_DBG_RC_SLOTS = 10
HEADS_CAP = 1 << 22
RANDOM_ZONES = 1 << 20


def main(argv=None):
    ap = _bench.parser(steps=10, warmup=2)
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        new = lambda dtype, n=None: torch.empty((H, W) if n is None else n, dtype=dtype, device=dev)
        dem = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem",))["dem"]
        ch = chain.Chain(H, W, ctx=ctx, px=px, overlap=False, tune_placement=False, river_threshold=N // 512)
        ch.run(dem.data_ptr())
        n_d = torch.zeros(1, dtype=torch.int64, device=dev)
        zones = {}
        # 1. landform classes (uint8 0..10 -> int32)
        lf = new(torch.uint8)
        _lib.check(L.dt_dev_horizon(ctx.h, dem.data_ptr(), H, W, px, 10, 0, float(np.tan(np.radians(1.0))),
                                    lf.data_ptr(), None, None, None, None))
        ctx.sync()
        zones["landform"] = (lf.to(torch.int32), 11)
        del lf
        # 2. the chain's reach catchments
        lk, so, cat = new(torch.int64), new(torch.int8), new(torch.int32)
        heads = new(torch.int64, HEADS_CAP)
        _lib.check(L.dt_dev_stream_order(ctx.h, ch.p("fdr"), ch.p("river"), H, W, so.data_ptr(), None, lk.data_ptr()))
        _lib.check(L.dt_dev_reach_catchments(ctx.h, lk.data_ptr(), ch.p("idx"), 4, H, W, None, cat.data_ptr(),
                                             heads.data_ptr(), HEADS_CAP, n_d.data_ptr()))
        ctx.sync()
        zones["catchments"] = (cat, int(n_d.item()))
        del so, heads
        # 3. the drainage basins (int64 flat indices), made dense
        basins, bz = lk, new(torch.int32)
        _lib.check(L.dt_dev_drainage(ctx.h, ch.p("fdr"), None, None, H, W, px, basins.data_ptr(), None, None))

        def compact_of(labels, out):
            def call():
                _lib.check(L.dt_dev_zonal_compact(ctx.h, labels.data_ptr(), 8, H, W, N, out.data_ptr(), None, 0,
                                                  n_d.data_ptr()))
            return call

        compact_of(basins, bz)()
        ctx.sync()
        zones["basins"] = (bz, int(n_d.item()))
        # 4. a random zone per cell
        zones["random_2^20"] = (torch.randint(0, RANDOM_ZONES, (H, W), dtype=torch.int32, device=dev), RANDOM_ZONES)
        # the values, in a tensor of this tool's own; the regions of 0 <= hand <= 3
        hand = torch.from_numpy(ch.buf["hand"].to_host(pinned=True)).to(dev)
        mask = ((hand >= 0) & (hand <= 3)).to(torch.uint8)
        regions, rz = new(torch.int64), new(torch.int32)
        _lib.check(L.dt_dev_regions_label(ctx.h, mask.data_ptr(), H, W, 8, regions.data_ptr(), None))
        compact_of(regions, rz)()
        ctx.sync()
        n_regions = int(n_d.item())
        ch.free()
        del mask, dem
        ok = torch.isfinite(hand) & (hand != -100)
        lo, hi = float(hand[ok].min().item()), float(hand[ok].max().item())
        del ok
        origin, s = float(np.floor(lo)), 16
        while s > 0 and (hi - origin) * 2.0 ** s > 2 ** 31 - 1:
            s -= 1

        zmax = max(n for _z, n in zones.values())
        tab = [new(torch.int64, zmax) for _ in range(4)] + [new(torch.float32, zmax) for _ in range(2)]

        def tables(z, n, all_acc, slots=0):
            ptrs = [t.data_ptr() for t in tab] if all_acc else [tab[0].data_ptr(), tab[1].data_ptr()] + [None] * 4

            def call():
                if slots:
                    _lib.check(L.dt_debug_set(DT_DBG_RC_SLOTS, slots))
                _lib.check(L.dt_dev_zonal_tables(ctx.h, z.data_ptr(), hand.data_ptr(), 4, H, W, n, origin, s, 1, -100.0,
                                                 *ptrs))
                if slots:
                    _lib.check(L.dt_debug_set(DT_DBG_RC_SLOTS, 0))
            return call

        src8, src12 = new(torch.uint8, N * 4), new(torch.uint8, N * 6)
        dst8, dst12 = torch.empty_like(src8), torch.empty_like(src12)
        ops = {"copy_8B_per_cell": (lambda: dst8.copy_(src8), 8), "copy_12B_per_cell": (lambda: dst12.copy_(src12), 12)}
        for k, (z, n) in zones.items():
            ops["tables_count_s1/%s" % k] = (tables(z, n, False), 8)
            ops["tables_all/%s" % k] = (tables(z, n, True), 8)
            ops["tables_count_s1_no_lds/%s" % k] = (tables(z, n, False, -1), 8)
            ops["tables_all_no_lds/%s" % k] = (tables(z, n, True, -1), 8)
        ops["compact/basins"] = (compact_of(basins, bz), 12)
        ops["compact/regions_hand_le_3"] = (compact_of(regions, rz), 12)
        cz, cn = zones["catchments"]
        for K in (64, 1024):
            edges = np.linspace(0.0, max(hi, 1.0), K + 1)
            counts = new(torch.int64, max(cn, 1) * K)

            def hist(edges=edges, K=K, counts=counts):
                _lib.check(L.dt_dev_zonal_counts(ctx.h, cz.data_ptr(), hand.data_ptr(), 4, H, W, cn,
                                                 edges.ctypes.data_as(_lib.c_f64p), K, 1, -100.0, counts.data_ptr()))
            ops["histogram_K%d/catchments" % K] = (hist, 8)
        painted = new(torch.float32)
        fill = np.array([np.nan], np.float32)
        ops["paint_f32/catchments"] = (lambda: _lib.check(L.dt_dev_zonal_paint(
            ctx.h, tab[4].data_ptr(), 4, cn, cz.data_ptr(), H, W, fill.ctypes.data_as(C.c_void_p), painted.data_ptr())), 8)
        t = _bench.events(ctx, st, {k: f for k, (f, _b) in ops.items()}, a.steps, a.warmup)
        status = ctx.status()
    out = {}
    for k, (_f, b) in ops.items():
        ms, mm = _bench.summary(t[k])
        out[k] = {"ms": ms, "ms_min_max": mm, "bytes_per_cell": b, "GBs": round(b * N / _bench.median(t[k]) / 1e6, 1)}
    res = {"tool": "zonal_bench", "size": [H, W], "seed": a.seed, "steps": a.steps, "warmup": a.warmup,
           "values": "the chain's HAND, float32", "origin": origin, "frac_bits": s, "value_range": [lo, hi],
           "n_zones": dict({k: n for k, (_z, n) in zones.items()}, regions_hand_le_3=n_regions),
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "ops": out, "status": status, "scratch_bytes": int(L.dt_ctx_scratch_bytes(ctx.h)),
           "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
