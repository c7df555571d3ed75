"""Resampling on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by default, px =
10), in one process, device time between events on resident rasters (tools/_bench.events):

  - average and nearest  size^2 -> (size/4)^2 and -> (size/16)^2;
  - bilinear, cubic and nearest  (size/4)^2 -> size^2 (the source is the average above);
  - mode  size^2 -> (size/4)^2 on the landform raster of dt_dev_horizon (radius 8);
  - average at factor 256, size^2 -> (size/256)^2: the footprint cap;
  - bilinear  size^2 -> size^2 turned by 30 degrees about the centre.

Each case is timed beside a device copy of the same algorithmic bytes -- the source read once and the destination
written once, as one flat uint8 copy of (source bytes + destination bytes) / 2 -- in the same run, the two alternating
inside a step: that copy is the yardstick, `ratio` = case / copy.  Prints one JSON line (and writes it to --out)."""
import ctypes as C
import math

import _bench

METHODS = ("nearest", "bilinear", "cubic", "average", "sum", "min", "max", "mode")


def main(argv=None):
    ap = _bench.parser(steps=5, warmup=2)
    a = ap.parse_args(argv)

    import torch
    from descriptools_amd import _lib

    S = a.size
    if S % 256:
        raise SystemExit("--size must be a multiple of 256")
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    f32_fill = int.from_bytes(torch.tensor(-100.0).numpy().tobytes(), "little")

    def resample(src, code, method, matrix, dst, nodata=-1, fill=0):
        m = (C.c_double * 6)(*matrix)
        _lib.check(L.dt_dev_resample(ctx.h, src.data_ptr(), code, src.shape[0], src.shape[1], m, METHODS.index(method),
                                     nodata, fill, dst.data_ptr(), dst.shape[0], dst.shape[1]))

    def zoom(k):
        return (0.0, float(k), 0.0, 0.0, 0.0, float(k))

    res = {"tool": "resample_bench", "size": [S, S], "seed": a.seed, "steps": a.steps, "warmup": a.warmup, "cases": {},
           "device": torch.cuda.get_device_name(0)}
    with torch.cuda.stream(st):
        dem = _bench.terrain(ctx, st, dev, S, a.seed, ("dem",), px)["dem"]
        landform = torch.empty((S, S), dtype=torch.uint8, device=dev)
        _lib.check(L.dt_dev_horizon(ctx.h, dem.data_ptr(), S, S, px, 8, 0, math.tan(math.radians(1.0)),
                                    landform.data_ptr(), None, None, None, None))
        q = torch.empty((S // 4, S // 4), dtype=torch.float32, device=dev)
        resample(dem, 32, "average", zoom(4), q)
        ctx.sync()

        def f32(n):
            return torch.empty((n, n), dtype=torch.float32, device=dev)

        c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
        h = S / 2
        turn = (h - c * h + s * h, c, -s, h - s * h - c * h, s, c)
        cases = [
            ("average_down4", dem, 32, "average", zoom(4), f32(S // 4), {}),
            ("nearest_down4", dem, 4, "nearest", zoom(4), f32(S // 4), {"fill": f32_fill}),
            ("average_down16", dem, 32, "average", zoom(16), f32(S // 16), {}),
            ("nearest_down16", dem, 4, "nearest", zoom(16), f32(S // 16), {"fill": f32_fill}),
            ("bilinear_up4", q, 32, "bilinear", zoom(0.25), f32(S), {}),
            ("cubic_up4", q, 32, "cubic", zoom(0.25), f32(S), {}),
            ("nearest_up4", q, 4, "nearest", zoom(0.25), f32(S), {"fill": f32_fill}),
            ("mode_down4", landform, 1, "mode", zoom(4), torch.empty((S // 4, S // 4), dtype=torch.uint8, device=dev), {}),
            ("average_down256", dem, 32, "average", zoom(256), f32(S // 256), {}),
            ("bilinear_turn30", dem, 32, "bilinear", turn, f32(S), {}),
        ]
        for name, src, code, method, matrix, dst, kw in cases:
            nbytes = src.numel() * src.element_size() + dst.numel() * dst.element_size()
            half = (nbytes // 2 + 15) // 16 * 16
            c_src = torch.empty(half, dtype=torch.uint8, device=dev)
            c_dst = torch.empty(half, dtype=torch.uint8, device=dev)
            calls = {"case": lambda: resample(src, code, method, matrix, dst, **kw), "copy": lambda: c_dst.copy_(c_src)}
            t = _bench.events(ctx, st, calls, a.steps, a.warmup)
            ms, ms_copy = _bench.summary(t["case"]), _bench.summary(t["copy"])
            res["cases"][name] = {"method": method, "src": list(src.shape), "dst": list(dst.shape),
                                  "dtype": str(src.dtype).replace("torch.", ""), "bytes": nbytes,
                                  "ms": ms[0], "ms_min_max": ms[1], "copy_ms": ms_copy[0], "copy_ms_min_max": ms_copy[1],
                                  "ratio": round(ms[0] / ms_copy[0], 2),
                                  "gb_s": round(nbytes / ms[0] * 1e-6, 1), "copy_gb_s": round(nbytes / ms_copy[0] * 1e-6, 1)}
            del c_src, c_dst, dst
        status = ctx.status()
    res["device_status"] = status
    res["timing"] = ("device time between events on resident rasters, median of --steps after --warmup; copy: a device "
                     "copy of (source + destination) / 2 bytes, timed alternately with the case")
    ctx.close()
    _bench.emit(res, a.out)


if __name__ == "__main__":
    main()
