"""Line-of-sight attributes on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by
default, px = 10), in one process, on one stream: dt_dev_horizon at radius 3 with the landform alone, at radius 3 with
all five outputs and at the radii of --radii (10, 32 and 64 by default) with all five, beside dt_dev_terrain at radius 1
with all eight outputs, the row DESIGN.md 4.16 carries.

The ops alternate, each bracketed by HIP events with a sync after it; the medians of --steps are reported with the
algorithmic bytes per cell of each call (4 B read + the bytes of its outputs; the kernel has no scratch traffic), the
rate that gives and its share of the 8 TB/s HBM figure the README uses, and the samples per second (8 radius samples
per cell).  Per-kernel times come from running this tool under `rocprofv3 --kernel-trace --stats`.  Prints one JSON
line (and writes it to --out)."""
import torch

import _bench
from descriptools_amd import _lib, horizon, terrain

HBM_GBPS = 8000.0
OUT_BYTES = {"landform": 1, "pattern": 2, "positive": 4, "negative": 4, "sky_view": 4}
DTYPES = {"landform": torch.uint8, "pattern": torch.int16, "positive": torch.float32, "negative": torch.float32,
          "sky_view": torch.float32}


def main(argv=None):
    ap = _bench.parser(steps=10, warmup=2)
    ap.add_argument("--radii", type=int, nargs="*", default=[10, 32, 64], help="radii timed with all five outputs")
    ap.add_argument("--flat", type=float, default=1.0, help="the flatness threshold in degrees")
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    sun = terrain.sun_vector()
    T = horizon.flat_tangent(a.flat)
    with torch.cuda.stream(st):
        dem = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem",))["dem"]
        out = {n: torch.empty((H, W), dtype=DTYPES[n], device=dev) for n in horizon.OUTPUTS}
        tout = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in terrain.OUTPUTS]

        def run(radius, names):
            ptrs = [out[n].data_ptr() if n in names else None for n in horizon.OUTPUTS]

            def call():
                _lib.check(L.dt_dev_horizon(ctx.h, dem.data_ptr(), H, W, px, radius, 0, T, *ptrs))
            return call

        def terrain_r1():
            _lib.check(L.dt_dev_terrain(ctx.h, dem.data_ptr(), H, W, px, 1, *sun, *[o.data_ptr() for o in tout]))

        ops = {"terrain_r1_all": terrain_r1, "r3_landform": run(3, ("landform",)), "r3_all": run(3, horizon.OUTPUTS)}
        radius = {"r3_landform": 3, "r3_all": 3}
        bytes_per_cell = {"terrain_r1_all": 4 + 4 * len(terrain.OUTPUTS), "r3_landform": 4 + OUT_BYTES["landform"],
                          "r3_all": 4 + sum(OUT_BYTES.values())}
        for r in a.radii:
            ops["r%d_all" % r] = run(r, horizon.OUTPUTS)
            radius["r%d_all" % r] = r
            bytes_per_cell["r%d_all" % r] = 4 + sum(OUT_BYTES.values())
        t = _bench.events(ctx, st, ops, a.steps, a.warmup)
        status = ctx.status()
        valued = float((out["landform"] != 0).sum().item()) / N  # of the last call
    med = {k: _bench.median(v) for k, v in t.items()}
    gbps = {k: bytes_per_cell[k] * N / (med[k] * 1e-3) / 1e9 for k in med}
    res = {"tool": "horizon_bench", "size": [H, W], "seed": a.seed, "px": px, "steps": a.steps, "warmup": a.warmup,
           "radii": a.radii, "flat": a.flat,
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: _bench.summary(v)[1] for k, v in t.items()},
           "algorithmic_bytes_per_cell": bytes_per_cell,
           "algorithmic_GBps": {k: round(v, 1) for k, v in gbps.items()},
           "share_of_8TBps": {k: round(v / HBM_GBPS, 4) for k, v in gbps.items()},
           "gigasamples_per_s": {k: round(8 * r * N / (med[k] * 1e-3) / 1e9, 1) for k, r in radius.items()},
           "ms_over_terrain_r1_all": {k: round(med[k] / med["terrain_r1_all"], 3) for k in med},
           "cells_with_a_value_last_call": round(valued, 4), "status": status,
           "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
