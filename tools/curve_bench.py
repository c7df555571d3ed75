"""The one-pass threshold histogram on 16384^2 rasters (--size), in one process, on one stream:
dt_dev_threshold_hist at K = 61, 1001, 10001 and 65535 thresholds (--ks) of the lattice k / (K - 1), beside the way to
the same counts without it -- ceil(K / 24) launches of dt_dev_confusion_multi on the resident rasters, which is the loop
of the host tier's dt_confusion_multi without its upload -- one such launch alone, and a float4 copy that moves 9 bytes
per cell (dt_dev_membench_copy, 4.5 read and 4.5 written), the byte floor of a pass that reads a float64 and an int8.

Three descriptors: "hand", the benchmark terrain's flow-path HAND scaled as evaluate_resident scales it (float32
arithmetic, thresholds rounded to float32; a benchmark map of the cells within --wet metres of their river cell), with its
nodata cells and its cells of exactly 0; "one_value", every cell 0.5, where every lane of every wave adds to the same
bin; "uniform", float64 uniform in [0, 1), where no two neighbours share a bin.

The ops alternate, each bracketed by HIP events with a sync after it; medians of --steps with min-max.  Per-kernel
counters come from running this tool under rocprofv3.  Prints one JSON line (and writes it to --out)."""
import numpy as np
import torch

import _bench
from descriptools_amd import _lib, evaluation

HBM_GBPS = 8000.0
BYTES_PER_CELL = 9


def main(argv=None):
    ap = _bench.parser(steps=10, warmup=2)
    ap.add_argument("--ks", type=int, nargs="*", default=[61, 1001, 10001, 65535])
    ap.add_argument("--old-max", type=int, default=10001,
                    help="largest K at which the 24-way launches are timed too (a launch costs milliseconds at any size: "
                         "its 96 same-address atomics per wave; 65535 thresholds are 2731 of them per call)")
    ap.add_argument("--wet", type=float, default=5.0, help="HAND below which the benchmark map is flooded")
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    res = {"tool": "curve_bench", "size": [H, W], "seed": a.seed, "steps": a.steps, "warmup": a.warmup, "ks": a.ks,
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "bytes_per_cell": BYTES_PER_CELL, "rasters": {}}
    with torch.cuda.stream(st):
        desc = torch.empty(N, dtype=torch.float64, device=dev)
        flood = torch.empty(N, dtype=torch.int8, device=dev)
        counts = torch.empty(24 * 4, dtype=torch.int64, device=dev)
        hist = torch.empty(2 * (max(a.ks) + 1) + 1, dtype=torch.int64, device=dev)
        n_copy = (N * BYTES_PER_CELL // 8) // 65536 * 65536  # floats: 4.5 B read + 4.5 B written per cell
        src = torch.zeros(n_copy, dtype=torch.float32, device=dev)
        dst = torch.empty(n_copy, dtype=torch.float32, device=dev)

        def fill(name):
            """-> (round thresholds to float32, extra facts)"""
            if name == "hand":
                hand = _bench.terrain(ctx, st, dev, a.size, a.seed, ("hand",))["hand"].reshape(-1)
                flood.copy_(((hand >= 0) & (hand <= a.wet)).to(torch.int8))
                ctx.sync()
                r = evaluation.evaluate_resident(ctx, hand.data_ptr(), flood.data_ptr(), N, desc_ptr=desc.data_ptr())
                return True, {"searched_threshold": r["threshold"], "searched_fit": float(r["fit"]),
                              "nodata_share": float((hand == -100).sum().item()) / N,
                              "zero_share": float((hand == 0).sum().item()) / N}
            if name == "one_value":
                desc.fill_(0.5)
            else:
                desc.copy_(torch.rand(N, dtype=torch.float64, device=dev))
            flood.copy_((torch.rand(N, device=dev) < 0.35).to(torch.int8))
            return False, {}

        for name in ("hand", "one_value", "uniform"):
            as_f32, facts = fill(name)
            ctx.sync()
            nodata = float(desc[0].item())
            ops, tables = {}, {}
            for K in a.ks:
                th = np.arange(K) / max(K - 1, 1)
                if as_f32:
                    th = th.astype(np.float32).astype(np.float64)
                th = np.ascontiguousarray(th)
                tables[K] = (th, torch.from_numpy(th).to(dev))

                def new(K=K):
                    _lib.check(L.dt_dev_threshold_hist(ctx.h, desc.data_ptr(), flood.data_ptr(), N, nodata,
                                                       tables[K][1].data_ptr(), K, 1, hist.data_ptr()))

                def old(K=K):
                    t = tables[K][0]
                    for k0 in range(0, K, 24):
                        k = min(24, K - k0)
                        _lib.check(L.dt_dev_confusion_multi(ctx.h, desc.data_ptr(), flood.data_ptr(), N, nodata,
                                                            _lib.ptr(t[k0:k0 + k], _lib.c_f64p), k, 1, counts.data_ptr()))
                ops["hist_%d" % K] = new
                if K <= a.old_max:
                    ops["passes24_%d" % K] = old

            def one_pass():
                _lib.check(L.dt_dev_confusion_multi(ctx.h, desc.data_ptr(), flood.data_ptr(), N, nodata,
                                                    _lib.ptr(tables[a.ks[0]][0][:24], _lib.c_f64p),
                                                    min(24, a.ks[0]), 1, counts.data_ptr()))

            def copy():
                _lib.check(L.dt_dev_membench_copy(ctx.h, src.data_ptr(), dst.data_ptr(), n_copy, -1))
            ops["confusion_one_pass"] = one_pass
            ops["copy_9B_per_cell"] = copy
            t = _bench.events(ctx, st, ops, a.steps, a.warmup)
            med = {k: _bench.median(v) for k, v in t.items()}
            # the last histogram against the last 24-way counts is checked by the tests; here only that all cells arrived
            K = a.ks[-1]
            ops["hist_%d" % K]()
            ctx.sync()
            h = hist[:2 * K + 3].cpu().numpy()
            c = evaluation._curve_of(tables[K][0], h, True)
            best = int(np.nanargmax(c.fit)) if not np.isnan(c.fit).all() else -1
            facts.update({"cells_in_histogram": int(h.sum()), "auc": c.auc,
                          "best_fit": float(c.fit[best]) if best >= 0 else None,
                          "best_fit_threshold": float(tables[K][0][best]) if best >= 0 else None})
            gbps = {k: BYTES_PER_CELL * N / (v * 1e-3) / 1e9 for k, v in med.items()
                    if k.startswith("hist_") or k in ("confusion_one_pass", "copy_9B_per_cell")}
            res["rasters"][name] = {
                "ms": {k: round(v, 3) for k, v in med.items()},
                "ms_min_max": {k: _bench.summary(v)[1] for k, v in t.items()},
                "algorithmic_GBps": {k: round(v, 1) for k, v in gbps.items()},
                "share_of_8TBps": {k: round(v / HBM_GBPS, 4) for k, v in gbps.items()},
                "ms_over_confusion_one_pass": {k: round(v / med["confusion_one_pass"], 2) for k, v in med.items()},
                "launches_24_way": {str(K): -(-K // 24) for K in a.ks},
                "facts": facts}
    res["status"] = ctx.status()
    res["device"] = torch.cuda.get_device_name(0)
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
