"""D-infinity direction and contributing area beside their D8 counterparts, in one process, on one
stream: dt_dev_dinf_direction against dt_dev_slope_d8 (slope + codes), dt_dev_dinf_accumulate against
dt_dev_flowacc_weighted, on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by default, px = 10).

The four ops alternate, each bracketed by HIP events with a sync after it; the medians of --steps are reported with
the nominal bytes per cell of each entry (what it must read and write, scratch traffic left out), the queue rounds
that found work, the queue's high-water mark and the share of two-receiver cells.  Per-kernel times come from running
this tool under `rocprofv3 --kernel-trace --stats`.  Before timing, the accumulation of float32(k pi / 4) angles made
from the D8 codes is checked against dt_dev_flowacc, cell for cell.  Prints one JSON line (and writes it to --out)."""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from descriptools_amd import _lib, flowacc  # noqa: E402
from descriptools_amd.device import Context  # noqa: E402

OCT_CODE = (1, 128, 64, 32, 16, 8, 4, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=0, help="budget of rounds; 0: 5/4 of what a first run needed, plus 16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    st = torch.cuda.Stream()
    ctx = Context(0, st.cuda_stream)
    dev = torch.device("cuda", 0)
    with torch.cuda.stream(st):
        dem = torch.empty((H, W), dtype=torch.float32, device=dev)
        fdr = torch.empty((H, W), dtype=torch.uint8, device=dev)
        slope = torch.empty((H, W), dtype=torch.float32, device=dev)
        angle = torch.empty((H, W), dtype=torch.float32, device=dev)
        dslope = torch.empty((H, W), dtype=torch.float32, device=dev)
        acc = torch.empty((H, W), dtype=torch.float64, device=dev)
        ones = torch.ones((H, W), dtype=torch.float64, device=dev)
        s = flowacc._default_frac_bits(N, 1.0)
        _lib.check(L.dt_dev_synth_dem(ctx.h, a.seed, H, W, 0, 0, H, W, 0, dem.data_ptr()))

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
        ops = (("slope_d8", d8), ("dinf_direction", dinf_dir), ("flowacc_weighted", fa_weighted),
               ("dinf_accumulate", dinf_acc))
        for _ in range(a.warmup):
            for _, fn in ops:
                fn()
        ctx.sync()
        _lib.check(L.dt_dev_dinf_accumulate_info(ctx.h, info.ctypes.data_as(_lib.c_i64p)))
        status = ctx.status()
        t = {name: [] for name, _ in ops}
        for _ in range(a.steps):
            for name, fn in ops:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                ctx.sync()
                t[name].append(e0.elapsed_time(e1))
        status |= ctx.status()
        no_flow = float((angle == -1).double().mean())
    med = {k: float(np.median(v)) for k, v in t.items()}
    bytes_per_cell = {"slope_d8": 4 + 4 + 1, "dinf_direction": 4 + 4 + 4, "flowacc_weighted": 1 + 8 + 8,
                      "dinf_accumulate": 4 + 8 + 8}
    res = {"tool": "dinf_bench", "size": [H, W], "seed": a.seed, "px": px, "frac_bits": s, "steps": a.steps,
           "warmup": a.warmup, "rounds_budget": a.rounds,
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: [round(min(v), 3), round(max(v), 3)] for k, v in t.items()},
           "nominal_bytes_per_cell": bytes_per_cell,
           "nominal_GBps": {k: round(bytes_per_cell[k] * N / (med[k] * 1e-3) / 1e9, 1) for k in med},
           "direction_over_slope_d8": round(med["dinf_direction"] / med["slope_d8"], 3),
           "accumulate_over_flowacc_weighted": round(med["dinf_accumulate"] / med["flowacc_weighted"], 3),
           "queue_rounds_with_work": int(info[0]), "queue_high_water_cells": int(info[1]),
           "cells_queued": int(info[2]), "two_receiver_share": round(float(info[3]) / N, 4),
           "no_flow_share": round(no_flow, 6), "status": status, "d8_angles_equal_flowacc": same,
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
