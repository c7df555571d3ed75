"""Weighted flow accumulation against the count it generalises: dt_dev_flowacc_weighted and
dt_dev_flowacc on the same D8 field, in one process, on one stream.

The field is D8 of the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by default); the weights are
seeded uniform [0, 10) float64, quantised at flowacc.weight_frac_bits' scale.  The two ops alternate, each bracketed
by HIP events with a sync after it; the medians of --steps are reported.  Before timing, the weighted op with unit
weights is checked against the count, cell for cell.  Prints one JSON line (and writes it to --out when given)."""
import torch

import _bench
from descriptools_amd import _args, _lib


def main(argv=None):
    a = _bench.parser(steps=20, warmup=3).parse_args(argv)
    H = W = a.size
    N = H * W
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        dem, fdr = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem", "fdr")).values()
        g = torch.Generator(device=dev)
        g.manual_seed(a.seed)
        w = torch.rand((H, W), dtype=torch.float64, device=dev, generator=g) * 10.0
        s = _args._default_frac_bits(N, float(w.max()))
        acc32 = torch.empty((H, W), dtype=torch.int32, device=dev)
        accw = torch.empty((H, W), dtype=torch.float64, device=dev)

        def count():
            _lib.check(L.dt_dev_flowacc(ctx.h, fdr.data_ptr(), dem.data_ptr(), H, W, acc32.data_ptr()))

        def weighted(wt=w, frac=s):
            _lib.check(L.dt_dev_flowacc_weighted(ctx.h, fdr.data_ptr(), dem.data_ptr(), wt.data_ptr(), H, W, frac,
                                                 accw.data_ptr()))

        # unit weights reproduce the count
        ones = torch.ones((H, W), dtype=torch.float64, device=dev)
        count()
        weighted(ones, _args._default_frac_bits(N, 1.0))
        ctx.sync()
        same = bool(torch.equal(acc32.to(torch.float64), accw))
        del ones
        assert same, "weighted(ones) != count"
        t = _bench.events(ctx, st, {"count": count, "weighted": weighted}, a.steps, a.warmup)
        assert ctx.status() == 0  # the bits are sticky: the warm-up's too
    med = {k: _bench.median(v) for k, v in t.items()}
    (count_ms, count_mm), (weighted_ms, weighted_mm) = _bench.summary(t["count"]), _bench.summary(t["weighted"])
    res = {"tool": "fa_weighted_bench", "size": [H, W], "seed": a.seed, "frac_bits": s, "steps": a.steps,
           "warmup": a.warmup, "timing": "median of HIP events around each op on its stream, ops alternating",
           "count_ms": count_ms, "weighted_ms": weighted_ms,
           "ratio": round(med["weighted"] / med["count"], 3),
           "count_ms_min_max": count_mm, "weighted_ms_min_max": weighted_mm,
           "ones_equal_count": same, "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
