"""Flow-path extremes and depression carving (dt_dev_flowpath_upslope, dt_dev_flowpath_downstream, dt_dev_carve_blend;
DESIGN.md 4.23) at 16384^2 on watershed_bench.py's two inputs: the benchmark terrain's D8 (with its DEM as the values
and its river as the stop mask) and a rough DEM conditioned on the device, whose paths run to the raster edge.  Beside
them, in the same run, the two yardsticks they are siblings of (dt_dev_upslope_length, dt_dev_drainage) and a device
copy of each op's algorithmic bytes.  After --warmup runs, each op is timed --steps times per input, bracketed by HIP
events on the context's stream with a sync after each; medians are reported.  Prints one JSON line (and writes it to
--out when given)."""
import numpy as np
import torch

import _bench
from descriptools_amd import _lib


def main(argv=None):
    a = _bench.parser(steps=10, warmup=2).parse_args(argv)
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        ter = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem", "fdr", "river"), px)
        rng = np.random.default_rng(a.seed)
        rough = torch.from_numpy(np.ascontiguousarray(rng.random((H, W), dtype=np.float32) * 100.0)).to(dev)
        filled = torch.empty((H, W), dtype=torch.float32, device=dev)
        fdr_c = torch.empty((H, W), dtype=torch.uint8, device=dev)
        info = np.zeros(3, np.int32)

        def condition():
            _lib.check(L.dt_dev_condition_d8(ctx.h, rough.data_ptr(), H, W, px, filled.data_ptr(), fdr_c.data_ptr(),
                                             info.ctypes.data_as(_lib.c_i32p)))

        condition()
        inputs = {"terrain": (ter["fdr"], ter["dem"], (ter["river"] != 0).to(torch.uint8)),
                  "conditioned": (fdr_c, rough, None)}
        val = torch.empty((H, W), dtype=torch.float32, device=dev)
        whr = torch.empty((H, W), dtype=torch.int64, device=dev)
        f64 = torch.empty((H, W), dtype=torch.float64, device=dev)
        i64 = torch.empty((H, W), dtype=torch.int64, device=dev)

        def up(k, where):
            f, v, _ = inputs[k]
            _lib.check(L.dt_dev_flowpath_upslope(ctx.h, f.data_ptr(), None, v.data_ptr(), H, W, 1, val.data_ptr(),
                                                 whr.data_ptr() if where else None))

        def down(k, stopped):
            f, v, s = inputs[k]
            _lib.check(L.dt_dev_flowpath_downstream(ctx.h, f.data_ptr(), None, v.data_ptr(),
                                                    s.data_ptr() if stopped else None, H, W, 0, val.data_ptr(), None))

        def upslope_length(k):
            _lib.check(L.dt_dev_upslope_length(ctx.h, inputs[k][0].data_ptr(), None, H, W, px, f64.data_ptr()))

        def drainage(k):
            _lib.check(L.dt_dev_drainage(ctx.h, inputs[k][0].data_ptr(), None, None, H, W, px, i64.data_ptr(),
                                         f64.data_ptr(), None))

        def copy_floats(bytes_per_cell):  # a float copy moves 8 bytes per element, in patches of 65536 floats
            return max(65536, N * bytes_per_cell // 8 // 65536 * 65536)

        # buffers of the copies' own, as long as the longest of them
        src = torch.zeros(copy_floats(17), dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)

        def copy(bytes_per_cell):
            n = copy_floats(bytes_per_cell)
            assert n <= src.numel() and n % 65536 == 0
            return lambda: _lib.check(L.dt_dev_membench_copy(ctx.h, src.data_ptr(), dst.data_ptr(), n, -1))

        def lowest():  # d8_carved's second part: the DEM is its own nodata raster
            _lib.check(L.dt_dev_flowpath_upslope(ctx.h, fdr_c.data_ptr(), rough.data_ptr(), rough.data_ptr(), H, W, 1,
                                                 val.data_ptr(), None))

        def blend():
            _lib.check(L.dt_dev_carve_blend(ctx.h, rough.data_ptr(), filled.data_ptr(), val.data_ptr(), H, W, 0.5,
                                            val.data_ptr()))

        calls = {}
        for k in inputs:
            calls[k, "upslope_min"] = lambda k=k: up(k, False)
            calls[k, "upslope_min_where"] = lambda k=k: up(k, True)
            calls[k, "downstream_max"] = lambda k=k: down(k, False)
            if inputs[k][2] is not None:
                calls[k, "downstream_max_to_river"] = lambda k=k: down(k, True)
            calls[k, "upslope_length"] = lambda k=k: upslope_length(k)
            calls[k, "drainage"] = lambda k=k: drainage(k)
        calls["copy", "copy_9B_per_cell"] = copy(9)    # fdr, values in; value out
        calls["copy", "copy_17B_per_cell"] = copy(17)  # ... and where
        calls["copy", "copy_12B_per_cell"] = copy(12)  # the blend: dem, filled, lowest in; carved out
        calls["carve", "condition_d8"] = condition
        calls["carve", "lowest"] = lowest
        calls["carve", "blend"] = blend
        t = _bench.events(ctx, st, calls, a.steps, a.warmup)
        lowest()
        ctx.sync()
        cut = int((val < rough).sum())
        raised = int((filled > rough).sum())
    runs = {}
    for (k, o), v in t.items():
        runs.setdefault(k, {})[o + "_ms"], runs[k][o + "_ms_min_max"] = _bench.summary(v)
    runs["carve"].update({"cells_cut": cut, "cells_the_fill_raises": raised, "fill_rounds": int(info[1]),
                          "flat_rounds": int(info[2])})
    res = {"tool": "flowpath_bench", "size": [H, W], "seed": a.seed, "px": px, "steps": a.steps, "warmup": a.warmup,
           "timing": "median of HIP events around each call on its stream, inputs and ops alternating",
           "scratch_bytes": int(L.dt_ctx_scratch_bytes(ctx.h)), "runs": runs, "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
