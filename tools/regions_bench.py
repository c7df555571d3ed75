"""Connected regions at three masks, in one process, 16384^2 by default: regions.label,
regions.connected and reaches.inundate_connected on (a) the wet mask hand <= h of the benchmark terrain
(dt_dev_synth_dem, bench.py's seed and threshold, px = 10; the chain's river network as seeds), (b) a 50 % random mask --
near the 8-connectivity percolation threshold, the longest find chains -- and (c) an all-foreground mask.

Two times per op and mask.  "host": the wall clock of the whole host-tier call, uploads and downloads included (1 B/cell
up and 8 B/cell down for label).  "device": the device-tier entry (dt_dev_regions_label / dt_dev_regions_select /
dt_dev_inundate_connected) on rasters that are already on the device, between two events on the context's stream --
the kernels alone.  Both are the median of --steps after --warmup.  The algorithmic bytes of the op stand beside them:
1 B read + 8 B label written per cell, plus what the union-find plane costs (4 B written by the local pass, 4 B read by
the flatten pass, the seam pass's reads aside).  (c) is checked against its closed form, (a) and (b) against each other
between the tiers.  Nothing is gated.  Prints one JSON line (and writes it to --out)."""
import numpy as np
import torch

import _bench
from descriptools_amd import _lib, reaches, regions


def main(argv=None):
    ap = _bench.parser(steps=5, warmup=1)
    ap.add_argument("--level", type=float, default=3.0, help="the wet mask is hand <= level (and hand >= 0)")
    ap.add_argument("--no-host", action="store_true", help="device-tier times only")
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    res = {"tool": "regions_bench", "size": [H, W], "seed": a.seed, "level": a.level, "steps": a.steps,
           "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "scratch_bytes_per_cell": 12,
           "algorithmic_bytes_per_cell": {"label": 1 + 8, "plane_P": 4 + 4}}
    with torch.cuda.stream(st):
        # the benchmark terrain, its river network, the flow-path HAND and one catchment for the whole raster
        river, hand = _bench.terrain(ctx, st, dev, a.size, a.seed, ("river", "hand"), px).values()
        gen = torch.Generator(device=dev)
        gen.manual_seed(a.seed)
        masks = {"wet": ((hand >= 0) & (hand <= a.level)).to(torch.uint8),
                 "random50": (torch.rand((H, W), device=dev, generator=gen) < 0.5).to(torch.uint8),
                 "all": torch.ones((H, W), dtype=torch.uint8, device=dev)}
        seeds = (river == 1).to(torch.uint8)
        cat = torch.zeros((H, W), dtype=torch.int32, device=dev)
        stage = torch.tensor([a.level], dtype=torch.float64, device=dev)
        label = torch.empty((H, W), dtype=torch.int64, device=dev)
        keep = torch.empty((H, W), dtype=torch.uint8, device=dev)
        depth = torch.empty((H, W), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        res["foreground_cells"] = {k: int(m.sum().item()) for k, m in masks.items()}
        res["seed_cells"] = int(seeds.sum().item())

        def device_ms(call):  # one entry at a time: its warm-up, then its steps
            return _bench.events(ctx, st, {"call": lambda: _lib.check(call())}, a.steps, a.warmup)["call"]

        dev_t = {}
        for name, m in masks.items():
            for cn in (8, 4):
                dev_t["label_%s_%d" % (name, cn)] = device_ms(
                    lambda: L.dt_dev_regions_label(ctx.h, m.data_ptr(), H, W, cn, label.data_ptr(), None))
            dev_t["connected_%s_8" % name] = device_ms(
                lambda: L.dt_dev_regions_select(ctx.h, m.data_ptr(), seeds.data_ptr(), H, W, 8, 1, keep.data_ptr()))
        dev_t["inundate_connected_wet_8"] = device_ms(
            lambda: L.dt_dev_inundate_connected(ctx.h, cat.data_ptr(), hand.data_ptr(), 4, stage.data_ptr(),
                                                river.data_ptr(), H, W, 1, 8, depth.data_ptr()))
        dev_t["inundate_wet"] = device_ms(
            lambda: L.dt_dev_inundate(ctx.h, cat.data_ptr(), hand.data_ptr(), 4, stage.data_ptr(), H, W, 1,
                                      depth.data_ptr()))
        # closed form of (c), and the regions of (a): how many, how many seeded
        _lib.check(L.dt_dev_regions_label(ctx.h, masks["all"].data_ptr(), H, W, 8, label.data_ptr(), None))
        ctx.sync()
        assert int(label.max().item()) == 0 and int(label.min().item()) == 0
        _lib.check(L.dt_dev_regions_label(ctx.h, masks["wet"].data_ptr(), H, W, 8, label.data_ptr(), None))
        _lib.check(L.dt_dev_regions_select(ctx.h, masks["wet"].data_ptr(), seeds.data_ptr(), H, W, 8, 1, keep.data_ptr()))
        ctx.sync()
        flat = torch.arange(N, device=dev, dtype=torch.int64).reshape(H, W)
        res["wet_regions"] = int((label == flat).sum().item())
        res["wet_cells_kept"] = int(keep.sum().item())
        host = {k: m.cpu().numpy() for k, m in masks.items()}
        host_seeds, host_hand, host_river = seeds.cpu().numpy(), hand.cpu().numpy(), river.cpu().numpy()
        dev_label_wet, dev_keep_wet = label.cpu().numpy(), keep.cpu().numpy()
    ctx.close()
    res["device_ms"] = {k: _bench.summary(v)[0] for k, v in dev_t.items()}
    res["device_ms_min_max"] = {k: _bench.summary(v)[1] for k, v in dev_t.items()}
    res["device_GBps_algorithmic_label"] = {
        k: round(N * 9 / (_bench.median(v) * 1e-3) / 1e9, 1) for k, v in dev_t.items() if k.startswith("label_")}
    del masks, seeds, hand, river, label, keep, depth, cat
    torch.cuda.empty_cache()
    if not a.no_host:
        got = regions.label(host["wet"])
        assert got.tobytes() == dev_label_wet.tobytes()
        assert regions.connected(host["wet"], host_seeds).tobytes() == dev_keep_wet.tobytes()
        del got
        cat_h = np.zeros((H, W), np.int32)
        ops = [("label_%s_8" % k, (lambda m: lambda: regions.label(m))(m)) for k, m in host.items()]
        ops += [("connected_%s_8" % k, (lambda m: lambda: regions.connected(m, host_seeds))(m)) for k, m in host.items()]
        ops += [("inundate_connected_wet_8",
                 lambda: reaches.inundate_connected(cat_h, host_hand, [a.level], host_river)),
                ("inundate_wet", lambda: reaches.inundate(cat_h, host_hand, [a.level]))]
        t = {name: _bench.timed(fn, a.steps, a.warmup) for name, fn in ops}
        res["host_ms"] = {k: _bench.summary(v, 2)[0] for k, v in t.items()}
        res["host_ms_min_max"] = {k: _bench.summary(v, 2)[1] for k, v in t.items()}
        res["host_timing"] = "wall clock of the whole host-tier call (mask != 0, uploads, kernels, downloads), median"
    _bench.emit(res, a.out)


if __name__ == "__main__":
    main()
