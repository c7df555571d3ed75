"""Local terrain attributes on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by
default, px = 10), in one process, on one stream: dt_dev_terrain at radius 1 with gradient + aspect, at radius 1 with all
eight outputs and at the radii of --radii (4 and 16 by default) with all eight, beside dt_dev_dinf_direction, the
sibling float64 3 x 3 stencil.

The ops alternate, each bracketed by HIP events with a sync after it; the medians of --steps are reported with the
algorithmic bytes per cell of each call (4 B read + 4 B per output; the fused radius > 1 kernel has no scratch traffic),
the rate that gives and its share of the 8 TB/s HBM figure the README uses, and each time as a ratio to
dinf_direction's.  Per-kernel times come from running this tool under `rocprofv3 --kernel-trace --stats`.  Prints one
JSON line (and writes it to --out)."""
import torch

import _bench
from descriptools_amd import _lib, terrain

HBM_GBPS = 8000.0


def main(argv=None):
    ap = _bench.parser(steps=10, warmup=2)
    ap.add_argument("--radii", type=int, nargs="*", default=[4, 16], help="radii > 1 timed with all eight outputs")
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    sun = terrain.sun_vector()
    with torch.cuda.stream(st):
        dem = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem",))["dem"]
        out = [torch.empty((H, W), dtype=torch.float32, device=dev) for _ in terrain.OUTPUTS]
        angle, slope = out[0], out[1]  # dinf_direction's two outputs: the calls alternate, nothing is compared

        def run(radius, names):
            ptrs = [o.data_ptr() if n in names else None for n, o in zip(terrain.OUTPUTS, out)]

            def call():
                _lib.check(L.dt_dev_terrain(ctx.h, dem.data_ptr(), H, W, px, radius, *sun, *ptrs))
            return call

        def dinf_dir():
            _lib.check(L.dt_dev_dinf_direction(ctx.h, dem.data_ptr(), None, H, W, px, angle.data_ptr(),
                                               slope.data_ptr()))

        ops = {"dinf_direction": dinf_dir, "r1_gradient_aspect": run(1, ("gradient", "aspect")),
               "r1_all": run(1, terrain.OUTPUTS)}
        nout = {"dinf_direction": 2, "r1_gradient_aspect": 2, "r1_all": 8}
        for r in a.radii:
            ops["r%d_all" % r] = run(r, terrain.OUTPUTS)
            nout["r%d_all" % r] = 8
        t = _bench.events(ctx, st, ops, a.steps, a.warmup)
        status = ctx.status()
        valued = float((out[0] != -100).sum().item()) / N  # of the last call
    med = {k: _bench.median(v) for k, v in t.items()}
    bytes_per_cell = {k: 4 + 4 * n for k, n in nout.items()}
    gbps = {k: bytes_per_cell[k] * N / (med[k] * 1e-3) / 1e9 for k in med}
    res = {"tool": "terrain_bench", "size": [H, W], "seed": a.seed, "px": px, "steps": a.steps, "warmup": a.warmup,
           "radii": a.radii,
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: _bench.summary(v)[1] for k, v in t.items()},
           "algorithmic_bytes_per_cell": bytes_per_cell,
           "algorithmic_GBps": {k: round(v, 1) for k, v in gbps.items()},
           "share_of_8TBps": {k: round(v / HBM_GBPS, 4) for k, v in gbps.items()},
           "ms_over_dinf_direction": {k: round(med[k] / med["dinf_direction"], 3) for k in med},
           "cells_with_a_value_last_call": round(valued, 4), "status": status,
           "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
