"""Reach catchments, channels, stage tables and inundation (dt_dev_reach_*, dt_dev_inundate) on the
benchmark terrain (dt_dev_synth_dem with bench.py's seed, 16384^2 by default), on a resident chain's own rasters: its
idx (int32), hand and slope (float32) and dt_dev_stream_order's link, at two thresholds in one process: the chain's
river = fac > N/512 and a dense one, fac > 1000.  K = 84 stages of one foot.  After --warmup runs, each entry is timed
--steps times, bracketed by HIP events on the context's stream with a sync after each; medians are reported with the
number of reaches R and the bytes each entry moves per cell.  The tables entry is timed four ways: with and without
the slope raster, and (--ab) without its LDS table, one global atomic per cell (DT_DBG_RC_SLOTS = -1), and with the
table capped at 4 slots.  Prints one JSON line (and writes it to --out when given)."""
import numpy as np
import torch

import _bench
from descriptools_amd import _args, _lib, chain
from descriptools_amd.reaches import bed_weight_max

DT_DBG_RC_SLOTS = 10
HEADS_CAP = 1 << 22


def main(argv=None):
    ap = _bench.parser(steps=20, warmup=3)
    ap.add_argument("--stages", type=int, default=84)
    ap.add_argument("--ab", action="store_true", help="also time the tables without and with a capped LDS table")
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    px = 10.0
    K = a.stages
    stages = np.arange(K) * 0.3048
    st_p = stages.ctypes.data_as(_lib.c_f64p)
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    thr = {"chain": N // 512, "dense": 1000}
    stats = {}
    with torch.cuda.stream(st):
        dem = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem",))["dem"]
        so = torch.empty((H, W), dtype=torch.int8, device=dev)
        lk = torch.empty((H, W), dtype=torch.int64, device=dev)
        reach = torch.empty((H, W), dtype=torch.int32, device=dev)
        cat = torch.empty((H, W), dtype=torch.int32, device=dev)
        depth = torch.empty((H, W), dtype=torch.float32, device=dev)
        heads = torch.empty(HEADS_CAP, dtype=torch.int64, device=dev)
        n_d = torch.zeros(1, dtype=torch.int64, device=dev)
        for k, v in thr.items():
            ch = chain.Chain(H, W, ctx=ctx, px=px, overlap=False, tune_placement=False, river_threshold=v)
            ch.run(dem.data_ptr())
            _lib.check(L.dt_dev_stream_order(ctx.h, ch.p("fdr"), ch.p("river"), H, W, so.data_ptr(), None,
                                             lk.data_ptr()))

            def catchments():
                _lib.check(L.dt_dev_reach_catchments(ctx.h, lk.data_ptr(), ch.p("idx"), 4, H, W, reach.data_ptr(),
                                                     cat.data_ptr(), heads.data_ptr(), HEADS_CAP, n_d.data_ptr()))

            catchments()
            ctx.sync()
            R = int(n_d.item())
            wmax = bed_weight_max(ch.buf["slope"].to_host(pinned=True))
            s = _args._default_frac_bits(N, max(float(stages[-1]), wmax))
            cha = [torch.empty(max(R, 1), dtype=torch.int64, device=dev) for _ in range(5)]
            tab = [torch.empty((max(R, 1), K), dtype=torch.int64, device=dev) for _ in range(3)]
            stage = torch.full((max(R, 1),), float(stages[K // 2]), dtype=torch.float64, device=dev)

            def channels():
                _lib.check(L.dt_dev_reach_channels(ctx.h, ch.p("fdr"), reach.data_ptr(), H, W, R,
                                                   *[t.data_ptr() for t in cha]))

            def tables(slope=True):
                _lib.check(L.dt_dev_reach_tables(ctx.h, cat.data_ptr(), ch.p("hand"), 4,
                                                 ch.p("slope") if slope else None, H, W, st_p, K, R, s,
                                                 *[t.data_ptr() for t in tab]))

            def inundate():
                _lib.check(L.dt_dev_inundate(ctx.h, cat.data_ptr(), ch.p("hand"), 4, stage.data_ptr(), H, W, R,
                                             depth.data_ptr()))

            def with_slots(n, slope):
                def f():
                    _lib.check(L.dt_debug_set(DT_DBG_RC_SLOTS, n))
                    tables(slope)
                    _lib.check(L.dt_debug_set(DT_DBG_RC_SLOTS, 0))
                return f

            # bytes per cell: what the entry reads and writes of full rasters (the per-reach arrays are noise)
            ops = {"catchments": (catchments, 8 + 4 + 4 + 4 + 8), "channels": (channels, 4),
                   "tables_slope": (tables, 12), "tables": (lambda: tables(False), 8), "inundate": (inundate, 12)}
            if a.ab:
                ops["tables_slope_no_lds"] = (with_slots(-1, True), 12)
                ops["tables_slope_4_slots"] = (with_slots(4, True), 12)
                ops["tables_no_lds"] = (with_slots(-1, False), 8)
            t = _bench.events(ctx, st, {o: f for o, (f, _b) in ops.items()}, a.steps, a.warmup)
            assert ctx.status() == 0  # the bits are sticky: the warm-up's too
            tables()
            ctx.sync()
            taking = int(tab[0][:R, K - 1].sum()) if R else 0
            stats[k] = {"threshold": v, "R": R, "frac_bits": s, "cells_in_tables": taking,
                        "network_cells": int((reach >= 0).sum()), "wet_cells": int((depth > 0).sum())}
            for o, (f, b) in ops.items():
                ms, ms_min_max = _bench.summary(t[o])
                stats[k][o] = {"ms": ms, "ms_min_max": ms_min_max, "bytes_per_cell": b,
                               "GBs": round(b * N / _bench.median(t[o]) / 1e6, 1)}
            del cha, tab, stage
            ch.free()
    res = {"tool": "reach_bench", "size": [H, W], "seed": a.seed, "px": px, "stages": K, "steps": a.steps,
           "warmup": a.warmup,
           "timing": "median of HIP events around each entry on its stream, entries alternating",
           "scratch_bytes": int(L.dt_ctx_scratch_bytes(ctx.h)), "runs": stats, "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
