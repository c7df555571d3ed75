"""Multiple-flow-direction shares and contributing area beside their D-infinity and D8 counterparts, in
one process, on one stream: dt_dev_mfd_shares (exponent 1.1: the pow instance; exponent 1: the integer instance)
against dt_dev_dinf_direction, dt_dev_mfd_accumulate against dt_dev_dinf_accumulate and dt_dev_flowacc_weighted, on the
benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by default, px = 10).

The ops alternate, each bracketed by HIP events with a sync after it; the medians of --steps are reported with the
nominal bytes per cell of each entry (what it must read and write, scratch traffic left out), each MFD figure as a
ratio to its D-infinity counterpart of the same run, the queue rounds that found work, the queue's high-water mark,
the cells queued and the share of cells with two or more receivers.  Per-kernel times come from running this tool under
`rocprofv3 --kernel-trace --stats`.  Before timing, the accumulation of the single-receiver shares made from the D8
codes is checked against dt_dev_flowacc, cell for cell.  Prints one JSON line (and writes it to --out)."""
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
        shares = torch.empty((H, W, 8), dtype=torch.int16, device=dev)  # the bits of uint16
        shares1 = torch.empty((H, W, 8), dtype=torch.int16, device=dev)
        acc = torch.empty((H, W), dtype=torch.float64, device=dev)
        ones = torch.ones((H, W), dtype=torch.float64, device=dev)
        s = _args._default_frac_bits(N, 1.0)
        budget = {"dinf": a.rounds, "mfd": a.rounds}

        def dinf_dir():
            _lib.check(L.dt_dev_dinf_direction(ctx.h, dem.data_ptr(), None, H, W, px, angle.data_ptr(),
                                               slope.data_ptr()))

        def mfd_shares():
            _lib.check(L.dt_dev_mfd_shares(ctx.h, dem.data_ptr(), None, H, W, 1.1, 0, shares.data_ptr()))

        def mfd_shares_p1():
            _lib.check(L.dt_dev_mfd_shares(ctx.h, dem.data_ptr(), None, H, W, 1.0, 0, shares1.data_ptr()))

        def fa_weighted():
            _lib.check(L.dt_dev_flowacc_weighted(ctx.h, fdr.data_ptr(), None, ones.data_ptr(), H, W, s, acc.data_ptr()))

        def budgeted(call, rounds):
            """`rounds` rounds as a caller enqueues them: a call takes 4096 at most, continuations take the rest"""
            call(min(rounds, 4096))
            for left in range(rounds - 4096, 0, -4096):
                call(-min(left, 4096))

        def dinf_acc(rounds=None):
            if rounds is None:
                return budgeted(dinf_acc, budget["dinf"])
            _lib.check(L.dt_dev_dinf_accumulate(ctx.h, angle.data_ptr(), ones.data_ptr(), H, W, s, rounds,
                                                acc.data_ptr()))

        def mfd_acc(rounds=None, sh=shares, fb=s):
            if rounds is None:
                return budgeted(mfd_acc, budget["mfd"])
            _lib.check(L.dt_dev_mfd_accumulate(ctx.h, sh.data_ptr(), ones.data_ptr(), H, W, fb, rounds, acc.data_ptr()))

        def finish(call, **kw):
            """a first call with the largest budget, continued until nothing is queued"""
            call(4096, **kw)
            while ctx.status() & 2:
                call(-4096, **kw)

        # single-receiver shares made from the D8 codes reproduce the count
        _lib.check(L.dt_dev_slope_d8(ctx.h, dem.data_ptr(), H, W, px, slope.data_ptr(), fdr.data_ptr(), None))
        lut = torch.zeros((256, 8), dtype=torch.int16, device=dev)
        for k, code in enumerate(OCT_CODE):
            lut[code, k] = -32768  # 0x8000
        for y in range(0, H, 1024):  # in slabs: the index tensor is int64
            shares1[y:y + 1024] = lut[fdr[y:y + 1024].long()]
        acc32 = torch.empty((H, W), dtype=torch.int32, device=dev)
        _lib.check(L.dt_dev_flowacc(ctx.h, fdr.data_ptr(), None, H, W, acc32.data_ptr()))
        finish(mfd_acc, sh=shares1, fb=0)
        same = bool(torch.equal(acc32.to(torch.float64), acc))
        assert same, "accumulate(d8_shares) != flowacc"
        del acc32, lut

        # size the budgets of rounds once, as a caller would
        dinf_dir()
        mfd_shares()
        info = np.zeros(4, np.int64)
        if a.rounds <= 0:
            finish(dinf_acc)
            _lib.check(L.dt_dev_dinf_accumulate_info(ctx.h, info.ctypes.data_as(_lib.c_i64p)))
            # which lane completes a cell varies run to run: so do the rounds
            budget["dinf"] = int(info[0]) * 5 // 4 + 16
            finish(mfd_acc)
            _lib.check(L.dt_dev_mfd_accumulate_info(ctx.h, info.ctypes.data_as(_lib.c_i64p)))
            budget["mfd"] = int(info[0]) * 5 // 4 + 16
        ops = {"dinf_direction": dinf_dir, "mfd_shares": mfd_shares, "mfd_shares_p1": mfd_shares_p1,
               "flowacc_weighted": fa_weighted, "dinf_accumulate": dinf_acc, "mfd_accumulate": mfd_acc}
        _bench.events(ctx, st, ops, 0, a.warmup)  # the queue's figures are those of the last warm-up call
        _lib.check(L.dt_dev_mfd_accumulate_info(ctx.h, info.ctypes.data_as(_lib.c_i64p)))
        status = ctx.status()
        t = _bench.events(ctx, st, ops, a.steps, 0)
        status |= ctx.status()
        # the first call of a budget above 4096 rounds leaves work queued and raises DT_STATUS_NOT_CONVERGED before its
        # continuation finishes it: whether the last timed accumulation finished is asked with one more round
        mfd_acc(-1)
        converged = not ctx.status() & 2
        receivers = int((shares != 0).sum().item()) / N
    med = {k: _bench.median(v) for k, v in t.items()}
    bytes_per_cell = {"dinf_direction": 4 + 4 + 4, "mfd_shares": 4 + 16, "mfd_shares_p1": 4 + 16,
                      "flowacc_weighted": 1 + 8 + 8, "dinf_accumulate": 4 + 8 + 8, "mfd_accumulate": 16 + 8 + 8}
    res = {"tool": "mfd_bench", "size": [H, W], "seed": a.seed, "px": px, "frac_bits": s, "steps": a.steps,
           "warmup": a.warmup, "rounds_budget": budget,
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: _bench.summary(v)[1] for k, v in t.items()},
           "nominal_bytes_per_cell": bytes_per_cell,
           "nominal_GBps": {k: round(bytes_per_cell[k] * N / (med[k] * 1e-3) / 1e9, 1) for k in med},
           "shares_over_dinf_direction": round(med["mfd_shares"] / med["dinf_direction"], 3),
           "shares_p1_over_dinf_direction": round(med["mfd_shares_p1"] / med["dinf_direction"], 3),
           "accumulate_over_dinf_accumulate": round(med["mfd_accumulate"] / med["dinf_accumulate"], 3),
           "accumulate_over_flowacc_weighted": round(med["mfd_accumulate"] / med["flowacc_weighted"], 3),
           "queue_rounds_with_work": int(info[0]), "queue_high_water_cells": int(info[1]),
           "cells_queued": int(info[2]), "multi_receiver_share": round(float(info[3]) / N, 4),
           "mean_receivers": round(receivers, 4), "status": status, "mfd_converged": converged,
           "d8_shares_equal_flowacc": same, "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
