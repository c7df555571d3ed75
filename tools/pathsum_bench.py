"""Weighted flow-path sums (dt_dev_flowpath_downstream_sum, dt_dev_flowpath_upslope_longest) at 16384^2
on flowpath_bench.py's two inputs: the benchmark terrain's D8 (weights px / (0.1 + sqrt(slope)), a travel time, and its
river as the stop mask) and a white-noise DEM conditioned on the device, whose paths run to the raster edge (uniform
random weights).  Beside them, in the same run, the ops they are siblings of (dt_dev_drainage, dt_dev_upslope_length,
dt_dev_flowpath_downstream, dt_dev_flowpath_upslope), the longest fold with unit weights (what upslope_length computes
on cardinal moves) and a device copy of the ops' algorithmic bytes.  After --warmup runs, each op is timed --steps times
per input, bracketed by HIP events on the context's stream with a sync after each; medians are reported.  Prints one
JSON line (and writes it to --out when given)."""
import numpy as np
import torch

import _bench
from descriptools_amd import _args, _lib


def main(argv=None):
    a = _bench.parser(steps=10, warmup=2).parse_args(argv)
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        ter = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem", "fdr", "slope", "river"), px)
        rng = np.random.default_rng(a.seed)
        rough = torch.from_numpy(np.ascontiguousarray(rng.random((H, W), dtype=np.float32) * 100.0)).to(dev)
        filled = torch.empty((H, W), dtype=torch.float32, device=dev)
        fdr_c = torch.empty((H, W), dtype=torch.uint8, device=dev)
        info = np.zeros(3, np.int32)
        _lib.check(L.dt_dev_condition_d8(ctx.h, rough.data_ptr(), H, W, px, filled.data_ptr(), fdr_c.data_ptr(),
                                         info.ctypes.data_as(_lib.c_i32p)))
        del filled
        w_t = (px / (0.1 + torch.sqrt(torch.clamp(ter["slope"], min=0.0)))).to(torch.float64)
        del ter["slope"]
        w_c = torch.from_numpy(rng.random((H, W)) * 10.0).to(dev)
        one = torch.ones((H, W), dtype=torch.float64, device=dev)
        # fdr, values of the extremes, weights, stop mask, frac_bits of the weights
        inputs = {"terrain": (ter["fdr"], ter["dem"], w_t, (ter["river"] != 0).to(torch.uint8)),
                  "conditioned": (fdr_c, rough, w_c, None)}
        bits = {k: _args._default_frac_bits(N, float(v[2].max())) for k, v in inputs.items()}
        val = torch.empty((H, W), dtype=torch.float32, device=dev)
        f64 = torch.empty((H, W), dtype=torch.float64, device=dev)
        i64 = torch.empty((H, W), dtype=torch.int64, device=dev)

        def down_sum(k, stopped):
            f, _, w, s = inputs[k]
            _lib.check(L.dt_dev_flowpath_downstream_sum(ctx.h, f.data_ptr(), None, w.data_ptr(),
                                                        s.data_ptr() if stopped else None, H, W, bits[k],
                                                        f64.data_ptr()))

        def longest(k, unit):
            f, _, w, _ = inputs[k]
            _lib.check(L.dt_dev_flowpath_upslope_longest(ctx.h, f.data_ptr(), None, (one if unit else w).data_ptr(), H,
                                                         W, 0 if unit else bits[k], f64.data_ptr()))

        def up_extreme(k):
            f, v, _, _ = inputs[k]
            _lib.check(L.dt_dev_flowpath_upslope(ctx.h, f.data_ptr(), None, v.data_ptr(), H, W, 1, val.data_ptr(), None))

        def down_extreme(k):
            f, v, _, _ = inputs[k]
            _lib.check(L.dt_dev_flowpath_downstream(ctx.h, f.data_ptr(), None, v.data_ptr(), None, H, W, 0,
                                                    val.data_ptr(), None))

        def upslope_length(k):
            _lib.check(L.dt_dev_upslope_length(ctx.h, inputs[k][0].data_ptr(), None, H, W, px, f64.data_ptr()))

        def drainage(k):
            _lib.check(L.dt_dev_drainage(ctx.h, inputs[k][0].data_ptr(), None, None, H, W, px, i64.data_ptr(),
                                         f64.data_ptr(), None))

        def copy_floats(bytes_per_cell):  # a float copy moves 8 bytes per element, in patches of 65536 floats
            return max(65536, N * bytes_per_cell // 8 // 65536 * 65536)

        src = torch.zeros(copy_floats(17), dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)

        def copy():  # codes and float64 weights in, a float64 raster out
            _lib.check(L.dt_dev_membench_copy(ctx.h, src.data_ptr(), dst.data_ptr(), copy_floats(17), -1))

        calls = {}
        for k in inputs:
            calls[k, "downstream_sum"] = lambda k=k: down_sum(k, False)
            if inputs[k][3] is not None:
                calls[k, "downstream_sum_to_river"] = lambda k=k: down_sum(k, True)
            calls[k, "upslope_longest"] = lambda k=k: longest(k, False)
            calls[k, "upslope_longest_unit_weights"] = lambda k=k: longest(k, True)
            calls[k, "downstream_extreme_max"] = lambda k=k: down_extreme(k)
            calls[k, "upslope_extreme_min"] = lambda k=k: up_extreme(k)
            calls[k, "upslope_length"] = lambda k=k: upslope_length(k)
            calls[k, "drainage"] = lambda k=k: drainage(k)
        calls["copy", "copy_17B_per_cell"] = copy
        t = _bench.events(ctx, st, calls, a.steps, a.warmup)
        # what the timed calls computed, on the terrain: how much of the raster has a value, and the largest
        down_sum("terrain", True)
        ctx.sync()
        defined_to_river = int((f64 >= 0).sum())
        longest("terrain", False)
        ctx.sync()
        defined = int((f64 >= 0).sum())
        tc_max = float(f64.max())
    runs = {}
    for (k, o), v in t.items():
        runs.setdefault(k, {})[o + "_ms"], runs[k][o + "_ms_min_max"] = _bench.summary(v)
    runs["terrain"].update({"frac_bits": bits["terrain"], "cells_with_a_path_to_the_river": defined_to_river,
                            "cells_with_a_longest_path": defined, "largest_longest_path": tc_max})
    runs["conditioned"].update({"frac_bits": bits["conditioned"], "fill_rounds": int(info[1]),
                                "flat_rounds": int(info[2])})
    res = {"tool": "pathsum_bench", "size": [H, W], "seed": a.seed, "px": px, "steps": a.steps, "warmup": a.warmup,
           "timing": "median of HIP events around each call on its stream, inputs and ops alternating",
           "scratch_bytes": int(L.dt_ctx_scratch_bytes(ctx.h)), "runs": runs, "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
