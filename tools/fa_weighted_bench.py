"""Weighted flow accumulation against the count it generalises: dt_dev_flowacc_weighted and
dt_dev_flowacc on the same D8 field, in one process, on one stream.

The field is D8 of the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by default); the weights are
seeded uniform [0, 10) float64, quantised at flowacc.weight_frac_bits' scale.  The two ops alternate, each bracketed
by HIP events with a sync after it; the medians of --steps are reported.  Before timing, the weighted op with unit
weights is checked against the count, cell for cell.  Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from descriptools_amd import _lib, flowacc  # noqa: E402
from descriptools_amd.device import Context  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    H = W = a.size
    N = H * W
    L = _lib.lib()
    st = torch.cuda.Stream()
    ctx = Context(0, st.cuda_stream)
    dev = torch.device("cuda", 0)
    with torch.cuda.stream(st):
        dem = torch.empty((H, W), dtype=torch.float32, device=dev)
        fdr = torch.empty((H, W), dtype=torch.uint8, device=dev)
        slope = torch.empty((H, W), dtype=torch.float32, device=dev)
        _lib.check(L.dt_dev_synth_dem(ctx.h, a.seed, H, W, 0, 0, H, W, 0, dem.data_ptr()))
        _lib.check(L.dt_dev_slope_d8(ctx.h, dem.data_ptr(), H, W, 10.0, slope.data_ptr(), fdr.data_ptr(), None))
        del slope
        g = torch.Generator(device=dev)
        g.manual_seed(a.seed)
        w = torch.rand((H, W), dtype=torch.float64, device=dev, generator=g) * 10.0
        s = flowacc._default_frac_bits(N, float(w.max()))
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
        weighted(ones, flowacc._default_frac_bits(N, 1.0))
        ctx.sync()
        same = bool(torch.equal(acc32.to(torch.float64), accw))
        del ones
        assert same, "weighted(ones) != count"
        for _ in range(a.warmup):
            count()
            weighted()
        ctx.sync()
        assert ctx.status() == 0
        t = {"count": [], "weighted": []}
        for _ in range(a.steps):
            for name, fn in (("count", count), ("weighted", weighted)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(st)
                fn()
                e1.record(st)
                ctx.sync()
                t[name].append(e0.elapsed_time(e1))
        assert ctx.status() == 0
    med = {k: float(np.median(v)) for k, v in t.items()}
    res = {"tool": "fa_weighted_bench", "size": [H, W], "seed": a.seed, "frac_bits": s, "steps": a.steps,
           "warmup": a.warmup, "timing": "median of HIP events around each op on its stream, ops alternating",
           "count_ms": round(med["count"], 3), "weighted_ms": round(med["weighted"], 3),
           "ratio": round(med["weighted"] / med["count"], 3),
           "count_ms_min_max": [round(min(t["count"]), 3), round(max(t["count"]), 3)],
           "weighted_ms_min_max": [round(min(t["weighted"]), 3), round(max(t["weighted"]), 3)],
           "ones_equal_count": same, "device": torch.cuda.get_device_name(0)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
