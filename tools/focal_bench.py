"""Focal statistics on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by default),
in one process, on one stream: dt_dev_focal at the radii of --radii (4, 64 and 1024 by default) with tpi alone and with
all five outputs, DEVmax over 8 and over 32 radii, beside a device copy that moves the scan's algorithmic bytes (28 per
cell: the heights read twice, the three planes written once) and dt_dev_terrain at radius 32 with one output, the
O(radius) window kernel this op stands next to.

The ops alternate, each bracketed by HIP events with a sync after it; the medians of --steps are reported.  A call is
the scan (three launches) and one evaluation launch, and the C ABI has no entry for the scan alone: the scan's own time
is the sum of k_fc_band_sums, k_fc_band_scan and k_fc_scan when this tool runs under `rocprofv3 --kernel-trace --stats`
(the same in every call, whatever the radius), and a call's evaluation is the rest.  DEVmax's time is NOT linear in the
number of radii alone -- it depends on how many rows of the tables the radii keep in flight -- so the
tool reports its time per radius and no split by difference.  origin and frac_bits are focal's defaults for the largest
radius timed.  Prints one JSON line (and writes it to --out)."""
import ctypes as C
import math

import numpy as np
import torch

import _bench
from descriptools_amd import _lib, focal, terrain

HBM_GBPS = 8000.0
SCAN_BYTES_PER_CELL = 28


def main(argv=None):
    ap = _bench.parser(steps=5, warmup=1)
    ap.add_argument("--radii", type=int, nargs="*", default=[4, 64, 1024], help="radii timed with one and five outputs")
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    top = max(a.radii + [32 * 32])
    with torch.cuda.stream(st):
        dem = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem",))["dem"]
        ok = torch.isfinite(dem) & (dem > -100)
        lo, hi = float(dem[ok].min().item()), float(dem[ok].max().item())
        del ok
        origin = float(math.floor(lo))
        s = focal.default_frac_bits(np.array([[lo, hi]], np.float32), top)
        out = {n: torch.empty((H, W), dtype=torch.int32 if n == "count" else torch.float32, device=dev)
               for n in focal.OUTPUTS}
        scale = torch.empty((H, W), dtype=torch.int16, device=dev)  # uint16 bits
        src = torch.empty(N * (SCAN_BYTES_PER_CELL // 2), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)

        def stats(radius, names):
            ptrs = [out[n].data_ptr() if n in names else None for n in focal.OUTPUTS]
            rs = (C.c_int32 * 1)(radius)

            def call():
                _lib.check(L.dt_dev_focal(ctx.h, dem.data_ptr(), H, W, origin, s, rs, 1, *ptrs, None))
            return call

        def dev_max(radii):
            rs = (C.c_int32 * len(radii))(*radii)

            def call():
                _lib.check(L.dt_dev_focal(ctx.h, dem.data_ptr(), H, W, origin, s, rs, len(radii), None, None, None, None,
                                          out["dev"].data_ptr(), scale.data_ptr()))
            return call

        def copy():
            dst.copy_(src)

        def terrain32():
            _lib.check(L.dt_dev_terrain(ctx.h, dem.data_ptr(), H, W, 10.0, 32, *terrain.sun_vector(),
                                        out["mean"].data_ptr(), *[None] * 7))

        ops = {"copy_28B_per_cell": copy}
        for r in a.radii:
            ops["r%d_tpi" % r] = stats(r, ("tpi",))
            ops["r%d_all" % r] = stats(r, focal.OUTPUTS)
        radii8, radii32 = [2 ** k for k in range(1, 9)], [32 * k for k in range(1, 33)]
        ops["dev_max_8"] = dev_max(radii8)
        ops["dev_max_32"] = dev_max(radii32)
        ops["terrain_r32_gradient"] = terrain32
        t = _bench.events(ctx, st, ops, a.steps, a.warmup)
        status = ctx.status()
        scratch = int(L.dt_ctx_scratch_bytes(ctx.h))
    med = {k: _bench.median(v) for k, v in t.items()}
    res = {"tool": "focal_bench", "size": [H, W], "seed": a.seed, "steps": a.steps, "warmup": a.warmup,
           "radii": a.radii, "dev_max_radii": {"8": radii8, "32": radii32},
           "origin": origin, "frac_bits": s, "height_range": [lo, hi],
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: _bench.summary(v)[1] for k, v in t.items()},
           "dev_max_ms_per_radius": {"8": round(med["dev_max_8"] / 8, 3), "32": round(med["dev_max_32"] / 32, 3)},
           "copy_GBps": round(SCAN_BYTES_PER_CELL * N / (med["copy_28B_per_cell"] * 1e-3) / 1e9, 1),
           "copy_share_of_8TBps": round(SCAN_BYTES_PER_CELL * N / (med["copy_28B_per_cell"] * 1e-3) / 1e9 / HBM_GBPS, 4),
           "scratch_bytes_per_cell": round(scratch / N, 3), "status": status,
           "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
