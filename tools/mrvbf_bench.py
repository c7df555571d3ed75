"""MRVBF / MRRTF and their building blocks on the benchmark terrain (dt_dev_synth_dem, bench.py's seed,
16384^2 by default), in one process, on one stream: dt_dev_percentile at radius 3, 6 and 16 (one output), dt_dev_coarsen
once, dt_dev_mrvbf with one and with both outputs at the default levels and -- the same kernel without a pyramid -- at
levels = 2, beside the two yardsticks this op stands next to: dt_dev_focal (tpi at radius 64, whose cost does not depend
on the radius) and dt_dev_horizon (the landform at radius 10, the other LDS-tile kernel).

The ops alternate, each bracketed by HIP events with a sync after it; the medians of --steps are reported.  What the
levels >= 3 cost together is the difference between a call at the default levels and one at levels = 2: the launches
that build the pyramid and the walk over the levels inside the final launch.  The launches alone are the sum of
k_coarsen and k_percentile when this tool runs under `rocprofv3 --kernel-trace --stats`.  Prints one JSON line (and
writes it to --out)."""
import ctypes as C
import math

import numpy as np
import torch

import _bench
from descriptools_amd import _lib, focal, mrvbf

PX = 10.0


def main(argv=None):
    ap = _bench.parser(steps=5, warmup=1)
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    levels = mrvbf.default_levels((H, W))
    t1 = mrvbf.slope_threshold(PX)
    with torch.cuda.stream(st):
        dem = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem",))["dem"]
        ok = torch.isfinite(dem) & (dem > -100)
        lo, hi = float(dem[ok].min().item()), float(dem[ok].max().item())
        del ok
        origin = float(math.floor(lo))
        s = focal.default_frac_bits(np.array([[lo, hi]], np.float32), 64)
        out = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in range(2)]
        form = torch.empty((H, W), dtype=torch.uint8, device=dev)
        Hc, Wc = -(-H // 3), -(-W // 3)
        out3 = [torch.empty((Hc, Wc), dtype=torch.float32, device=dev) for _ in range(2)]
        g = (C.c_double * 6)(*mrvbf._gauss_weights())

        def percentile(radius):
            def call():
                _lib.check(L.dt_dev_percentile(ctx.h, dem.data_ptr(), H, W, radius, out[0].data_ptr(), None))
            return call

        def coarsen():
            _lib.check(L.dt_dev_coarsen(ctx.h, dem.data_ptr(), H, W, PX, g, out3[0].data_ptr(), out3[1].data_ptr()))

        def indices(n_levels, both):
            p = (C.c_double * (n_levels - 1))(*mrvbf._exponents(n_levels))

            def call():
                _lib.check(L.dt_dev_mrvbf(ctx.h, dem.data_ptr(), H, W, PX, t1, n_levels, 0.4, 0.35, p,
                                          out[0].data_ptr(), out[1].data_ptr() if both else None))
            return call

        def focal_tpi():
            rs = (C.c_int32 * 1)(64)
            _lib.check(L.dt_dev_focal(ctx.h, dem.data_ptr(), H, W, origin, s, rs, 1, None, None, None,
                                      out[0].data_ptr(), None, None))

        def horizon():
            _lib.check(L.dt_dev_horizon(ctx.h, dem.data_ptr(), H, W, PX, 10, 0, math.tan(math.radians(1.0)),
                                        form.data_ptr(), None, None, None, None))

        ops = {"percentile_r3": percentile(3), "percentile_r6": percentile(6), "percentile_r16": percentile(16),
               "coarsen": coarsen, "indices_mrvbf": indices(levels, False), "indices_both": indices(levels, True),
               "indices_mrvbf_levels2": indices(2, False), "indices_both_levels2": indices(2, True),
               "focal_r64_tpi": focal_tpi, "horizon_r10_landform": horizon}
        t = _bench.events(ctx, st, ops, a.steps, a.warmup)
        status = ctx.status()
    med = {k: _bench.median(v) for k, v in t.items()}
    res = {"tool": "mrvbf_bench", "size": [H, W], "seed": a.seed, "steps": a.steps, "warmup": a.warmup, "px": PX,
           "levels": levels, "slope_threshold": t1,
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: _bench.summary(v)[1] for k, v in t.items()},
           "levels_ge3_share": {k: round(1.0 - med[k + "_levels2"] / med[k], 4)
                                for k in ("indices_mrvbf", "indices_both")},
           "pyramid_bytes_per_cell": round(pyramid_bytes(H, W, levels) / N, 3), "status": status,
           "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


def pyramid_bytes(H, W, levels):
    """16 bytes per cell of the levels 3 .. levels, each raster rounded up to 256 bytes as the library carves them"""
    total = 0
    for _ in range(3, levels + 1):
        H, W = -(-H // 3), -(-W // 3)
        total += 4 * ((4 * H * W + 255) // 256 * 256)
    return total


if __name__ == "__main__":
    main()
