"""D-infinity direction and contributing area beside their D8 counterparts, in one process, on one
stream: dt_dev_dinf_direction against dt_dev_slope_d8 (slope + codes), dt_dev_dinf_accumulate against
dt_dev_flowacc_weighted, on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by default, px = 10).

The four ops alternate, each bracketed by HIP events with a sync after it; the medians of --steps are reported with
the nominal bytes per cell of each entry (what it must read and write, scratch traffic left out), the queue rounds
that found work, the queue's high-water mark and the share of two-receiver cells.  Per-kernel times come from running
this tool under `rocprofv3 --kernel-trace --stats`.  Before timing, the accumulation of float32(k pi / 4) angles made
from the D8 codes is checked against dt_dev_flowacc, cell for cell.  Prints one JSON line (and writes it to --out)."""
import math

import numpy as np
import torch

import _bench
from descriptools_amd import _args, _lib

OCT_CODE = (1, 128, 64, 32, 16, 8, 4, 2)


def main(argv=None):
    ap = _bench.parser(steps=10, warmup=2)
    ap.add_argument("--rounds", type=int, default=0, help="budget of rounds; 0: 5/4 of what a first run needed, plus 16")
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        dem = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem",))["dem"]
        fdr = torch.empty((H, W), dtype=torch.uint8, device=dev)
        slope = torch.empty((H, W), dtype=torch.float32, device=dev)
        angle = torch.empty((H, W), dtype=torch.float32, device=dev)
        dslope = torch.empty((H, W), dtype=torch.float32, device=dev)
        acc = torch.empty((H, W), dtype=torch.float64, device=dev)
        ones = torch.ones((H, W), dtype=torch.float64, device=dev)
        s = _args._default_frac_bits(N, 1.0)

        def d8():
            _lib.check(L.dt_dev_slope_d8(ctx.h, dem.data_ptr(), H, W, px, slope.data_ptr(), fdr.data_ptr(), None))

        def dinf_dir():
            _lib.check(L.dt_dev_dinf_direction(ctx.h, dem.data_ptr(), None, H, W, px, angle.data_ptr(),
                                               dslope.data_ptr()))

        def fa_weighted():
            _lib.check(L.dt_dev_flowacc_weighted(ctx.h, fdr.data_ptr(), None, ones.data_ptr(), H, W, s, acc.data_ptr()))

        def dinf_acc():
            _lib.check(L.dt_dev_dinf_accumulate(ctx.h, angle.data_ptr(), ones.data_ptr(), H, W, s, a.rounds,
                                                acc.data_ptr()))

        # D8 angles reproduce the count
        d8()
        lut = torch.full((256,), -1.0, dtype=torch.float32, device=dev)
        for k, code in enumerate(OCT_CODE):
            lut[code] = float(np.float32(k * math.pi / 4))
        a8 = lut[fdr.long()]
        acc32 = torch.empty((H, W), dtype=torch.int32, device=dev)
        _lib.check(L.dt_dev_flowacc(ctx.h, fdr.data_ptr(), None, H, W, acc32.data_ptr()))
        _lib.check(L.dt_dev_dinf_accumulate(ctx.h, a8.data_ptr(), ones.data_ptr(), H, W, 0, 4096, acc.data_ptr()))
        while ctx.status() & 2:
            _lib.check(L.dt_dev_dinf_accumulate(ctx.h, a8.data_ptr(), ones.data_ptr(), H, W, 0, -4096, acc.data_ptr()))
        same = bool(torch.equal(acc32.to(torch.float64), acc))
        assert same, "accumulate(D8 angles) != flowacc"
        del a8, acc32, lut

        # size the budget of rounds once, as a caller would
        dinf_dir()
        info = np.zeros(4, np.int64)
        if a.rounds <= 0:
            a.rounds = 4096
            dinf_acc()
            while ctx.status() & 2:
                _lib.check(L.dt_dev_dinf_accumulate(ctx.h, angle.data_ptr(), ones.data_ptr(), H, W, s, -4096,
                                                    acc.data_ptr()))
            _lib.check(L.dt_dev_dinf_accumulate_info(ctx.h, info.ctypes.data_as(_lib.c_i64p)))
            a.rounds = int(info[0]) * 5 // 4 + 16  # which lane completes a cell varies run to run: so do the rounds
        ops = {"slope_d8": d8, "dinf_direction": dinf_dir, "flowacc_weighted": fa_weighted,
               "dinf_accumulate": dinf_acc}
        _bench.events(ctx, st, ops, 0, a.warmup)  # the queue's figures are those of the last warm-up call
        _lib.check(L.dt_dev_dinf_accumulate_info(ctx.h, info.ctypes.data_as(_lib.c_i64p)))
        status = ctx.status()
        t = _bench.events(ctx, st, ops, a.steps, 0)
        status |= ctx.status()
        no_flow = float((angle == -1).double().mean())
    med = {k: _bench.median(v) for k, v in t.items()}
    bytes_per_cell = {"slope_d8": 4 + 4 + 1, "dinf_direction": 4 + 4 + 4, "flowacc_weighted": 1 + 8 + 8,
                      "dinf_accumulate": 4 + 8 + 8}
    res = {"tool": "dinf_bench", "size": [H, W], "seed": a.seed, "px": px, "frac_bits": s, "steps": a.steps,
           "warmup": a.warmup, "rounds_budget": a.rounds,
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: _bench.summary(v)[1] for k, v in t.items()},
           "nominal_bytes_per_cell": bytes_per_cell,
           "nominal_GBps": {k: round(bytes_per_cell[k] * N / (med[k] * 1e-3) / 1e9, 1) for k in med},
           "direction_over_slope_d8": round(med["dinf_direction"] / med["slope_d8"], 3),
           "accumulate_over_flowacc_weighted": round(med["dinf_accumulate"] / med["flowacc_weighted"], 3),
           "queue_rounds_with_work": int(info[0]), "queue_high_water_cells": int(info[1]),
           "cells_queued": int(info[2]), "two_receiver_share": round(float(info[3]) / N, 4),
           "no_flow_share": round(no_flow, 6), "status": status, "d8_angles_equal_flowacc": same,
           "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
