"""Flood inundation on the benchmark terrain (dt_dev_synth_dem, bench.py's seed, px = 10) under
uniform rain, at --sizes (4096 and 16384 by default), in one process:

* the device time per step: dt_dev_inundation with max_steps = --batch on resident rasters between two timing events
  (so 2 * batch + 3 launches and no host synchronisation in between), divided by the batch.  The state it starts from
  is a film of --film metres on every cell after --spinup steps of the same rain, so that every face is wet and the
  flux arithmetic runs everywhere; "dry" is the same measurement from a dry start (no face wet: no cube root taken);
* a device copy of the same algorithmic bytes, in the same run and alternating with the steps: 52 B per cell and step
  (h, qx, qy read and written, the float32 heights read), so a copy of 26 B per cell read and 26 B written
  (dt_dev_membench_copy); the achieved rate of a step is 52 B * cells / its time, and the ratio to the copy's is the
  figure to explain;
* a whole inundation.simulate call (host tier: the argument checks, uploads, --sim-steps steps, downloads, the volume),
  wall clock.

Prints one JSON line (and writes it to --out).  `rocprofv3 --kernel-trace --stats -- python tools/inundation_bench.py
--profile-only --sizes 4096` runs one batch for a kernel trace of its own."""
import numpy as np

import _bench

BYTES_PER_CELL = 52


def main(argv=None):
    ap = _bench.parser(steps=5, warmup=1)
    ap.add_argument("--sizes", default="4096,16384")
    ap.add_argument("--batch", type=int, default=50, help="steps per timed call")
    ap.add_argument("--spinup", type=int, default=20)
    ap.add_argument("--film", type=float, default=0.05)
    ap.add_argument("--rain", type=float, default=50e-3 / 3600.0, help="m/s")
    ap.add_argument("--sim-steps", type=int, default=100)
    ap.add_argument("--skip", default="", help="comma-separated: simulate, dry")
    ap.add_argument("--profile-only", action="store_true", help="one batch per size (for rocprofv3)")
    a = ap.parse_args(argv)

    import torch
    from descriptools_amd import _lib, inundation
    from descriptools_amd._lib import c_f64p, ptr

    L = _lib.lib()
    px = 10.0
    skip = set(a.skip.split(","))
    res = {"tool": "inundation_bench", "seed": a.seed, "steps": a.steps, "warmup": a.warmup, "batch": a.batch,
           "rain_m_per_s": a.rain, "film_m": a.film, "bytes_per_cell_and_step": BYTES_PER_CELL,
           "timing": "HIP events around a batch of steps on the context's stream, median over --steps batches",
           "device": torch.cuda.get_device_name(0), "sizes": {}}
    for size in [int(s) for s in a.sizes.split(",")]:
        H = W = size
        n = H * W
        ctx, st, dev = _bench.device()
        with torch.cuda.stream(st):
            dem = _bench.terrain(ctx, st, dev, size, a.seed, ("dem",), px)["dem"]
            h, qx, qy = (torch.zeros((H, W), dtype=torch.float64, device=dev) for _ in range(3))
            n_copy = (BYTES_PER_CELL * n) // 8  # floats: 4 B read + 4 B written each
            src = torch.zeros(n_copy, dtype=torch.float32, device=dev)
            dst = torch.empty(n_copy, dtype=torch.float32, device=dev)
            info = torch.zeros(inundation.INFO_WORDS, dtype=torch.int64, device=dev)
            par = np.array([px, 0.0, 1e9, 0.05, a.rain, 0.7, 60.0, 1e-3, 1e-3, 0.05], np.float64)

            def steps(count):
                _lib.check(L.dt_dev_inundation(ctx.h, dem.data_ptr(), None, None, H, W, ptr(par, c_f64p), 0, None, None,
                                               None, 0, 0, 0, count, h.data_ptr(), qx.data_ptr(), qy.data_ptr(), None,
                                               None, info.data_ptr()))

            def copy():
                _lib.check(L.dt_dev_membench_copy(ctx.h, src.data_ptr(), dst.data_ptr(), n_copy, -1))

            out = {}
            if a.profile_only:
                h.fill_(a.film)
                steps(a.batch)
                ctx.sync()
            else:
                for name in ("dry", "wet"):
                    if name in skip:
                        continue
                    h.fill_(a.film if name == "wet" else 0.0)
                    qx.zero_()
                    qy.zero_()
                    par[4] = a.rain if name == "wet" else 0.0
                    steps(a.spinup)
                    ctx.sync()
                    t = _bench.events(ctx, st, {"steps": lambda: steps(a.batch), "copy": copy}, a.steps, a.warmup)
                    ctx.sync()
                    step_ms = _bench.median(t["steps"]) / a.batch
                    copy_ms = _bench.median(t["copy"])
                    got = info.cpu().numpy()
                    out[name] = {"step_ms": round(step_ms, 4), "step_ms_range": [round(min(t["steps"]) / a.batch, 4),
                                                                               round(max(t["steps"]) / a.batch, 4)],
                                 "copy_same_bytes_ms": round(copy_ms, 4),
                                 "step_GBs": round(BYTES_PER_CELL * n / (step_ms * 1e-3) / 1e9, 1),
                                 "copy_GBs": round(BYTES_PER_CELL * n / (copy_ms * 1e-3) / 1e9, 1),
                                 "step_over_copy": round(step_ms / copy_ms, 3),
                                 "hmax_m": float(got[5:6].view(np.float64)[0]),
                                 "dt_last_s": float(got[4:5].view(np.float64)[0]),
                                 "wet_share": round(float((h > 1e-3).double().mean().item()), 4)}
            del src, dst, h, qx, qy
            if "simulate" not in skip and not a.profile_only:
                z = dem.cpu().numpy()
        del dem
        ctx.close()
        torch.cuda.empty_cache()
        if "simulate" not in skip and not a.profile_only:
            ms = _bench.timed(lambda: inundation.simulate(z, px, 1e9, rain=a.rain, max_steps=a.sim_steps), 1, 0)
            out["simulate"] = {"steps": a.sim_steps, "ms": round(ms[0], 1), "outputs": ["depth"]}
            del z
        res["sizes"][str(size)] = out
    _bench.emit(res, a.out)


if __name__ == "__main__":
    main()
