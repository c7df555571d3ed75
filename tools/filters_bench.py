"""DEM filters on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by default), in one
process, on one stream: dt_dev_filter_extremes (minimum and maximum) at radius 4, 64 and 1024 beside dt_dev_focal's tpi
at the same radii; dt_dev_filter_rank (the median) at radius 1, 2, 5 and 16 beside dt_dev_percentile (MRVBF's elevation
percentile) at 3, 6 and 16; dt_dev_filter_denoise at radius 5 with one and with three steps beside dt_dev_terrain at
radius 5 with one output; and a device copy of 8 bytes per cell (a raster read, a raster written).

The ops alternate, each bracketed by HIP events with a sync after it; the medians of --steps are reported.  The
denoising has one entry: a Jacobi step is (three steps - one step) / 2 and the normals with the window sum are the rest
of the one-step call; the two are told apart by k_fd_normals and k_fd_smooth when this tool runs under `rocprofv3
--kernel-trace --stats`.  Prints one JSON line (and writes it to --out)."""
import ctypes as C
import math

import numpy as np
import torch

import _bench
from descriptools_amd import _lib, filters, focal, terrain

COPY_BYTES_PER_CELL = 8


def main(argv=None):
    ap = _bench.parser(steps=5, warmup=1)
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    radii, rank_radii, ep_radii = (4, 64, 1024), (1, 2, 5, 16), (3, 6, 16)
    with torch.cuda.stream(st):
        dem = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem",))["dem"]
        ok = torch.isfinite(dem) & (dem > -100)
        lo, hi = float(dem[ok].min().item()), float(dem[ok].max().item())
        del ok
        origin = float(math.floor(lo))
        s = focal.default_frac_bits(np.array([[lo, hi]], np.float32), max(radii))
        o1 = torch.empty((H, W), dtype=torch.float32, device=dev)
        o2 = torch.empty((H, W), dtype=torch.float32, device=dev)
        src = torch.empty(N * (COPY_BYTES_PER_CELL // 2), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        t = math.cos(math.radians(15.0))

        def extremes(radius):
            def call():
                _lib.check(L.dt_dev_filter_extremes(ctx.h, dem.data_ptr(), H, W, radius, o1.data_ptr(), o2.data_ptr(),
                                                    None, None, None))
            return call

        def tpi(radius):
            rs = (C.c_int32 * 1)(radius)

            def call():
                _lib.check(L.dt_dev_focal(ctx.h, dem.data_ptr(), H, W, origin, s, rs, 1, None, None, None, o1.data_ptr(),
                                          None, None))
            return call

        def rank(radius):
            table = filters.rank_table(radius, 50.0)
            tp = table.ctypes.data_as(C.POINTER(C.c_uint16))

            def call(table=table):
                _lib.check(L.dt_dev_filter_rank(ctx.h, dem.data_ptr(), H, W, radius, tp, table.size, o1.data_ptr()))
            return call

        def ep(radius):
            def call():
                _lib.check(L.dt_dev_percentile(ctx.h, dem.data_ptr(), H, W, radius, o1.data_ptr(), None))
            return call

        def denoise(steps):
            def call():
                _lib.check(L.dt_dev_filter_denoise(ctx.h, dem.data_ptr(), H, W, 10.0, 5, t, steps, 0.5, o1.data_ptr()))
            return call

        def copy():
            dst.copy_(src)

        def terrain5():
            _lib.check(L.dt_dev_terrain(ctx.h, dem.data_ptr(), H, W, 10.0, 5, *terrain.sun_vector(), o1.data_ptr(),
                                        *[None] * 7))

        ops = {"copy_8B_per_cell": copy}
        for r in radii:
            ops["extremes_r%d" % r] = extremes(r)
            ops["tpi_r%d" % r] = tpi(r)
        for r in rank_radii:
            ops["percentile_r%d" % r] = rank(r)
        for r in ep_radii:
            ops["ep_r%d" % r] = ep(r)
        ops["denoise_r5_1_step"] = denoise(1)
        ops["denoise_r5_3_steps"] = denoise(3)
        ops["terrain_r5_gradient"] = terrain5
        tm = _bench.events(ctx, st, ops, a.steps, a.warmup)
        status = ctx.status()
        scratch = int(L.dt_ctx_scratch_bytes(ctx.h))
    med = {k: _bench.median(v) for k, v in tm.items()}
    step = (med["denoise_r5_3_steps"] - med["denoise_r5_1_step"]) / 2
    res = {"tool": "filters_bench", "size": [H, W], "seed": a.seed, "steps": a.steps, "warmup": a.warmup,
           "radii": {"extremes": radii, "percentile": rank_radii, "ep": ep_radii}, "height_range": [lo, hi],
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: _bench.summary(v)[1] for k, v in tm.items()},
           "denoise_ms": {"per_step": round(step, 3),
                          "normals_and_window_sum": round(med["denoise_r5_1_step"] - step, 3)},
           "copy_GBps": round(COPY_BYTES_PER_CELL * N / (med["copy_8B_per_cell"] * 1e-3) / 1e9, 1),
           "scratch_bytes_per_cell": round(scratch / N, 3), "status": status,
           "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
