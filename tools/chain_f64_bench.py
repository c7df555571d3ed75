"""The resident chain's step on float32 and on float64 heights, same terrain, same process.

The float64 DEM is the benchmark terrain (oracle.synth_dem, seed 1) plus sub-float32 structure, as in
tests/test_dem_dtype.py::test_wide_dems_against_the_float64_oracle; the float32 chain runs on that terrain's float32
heights.  Each chain runs its ops(serial=True) on one stream: HIP events around every op and around the whole step.
Prints one JSON line (and writes it to --out when given)."""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import oracle  # noqa: E402
from descriptools_amd import _lib, chain  # noqa: E402
from descriptools_amd.device import Context  # noqa: E402


def dem64_of(d32):
    """float64 heights with structure below float32's resolution; nodata stays -100 (row blocks: no full-size
    temporaries beyond the result)"""
    H, W = d32.shape
    out = np.empty((H, W), np.float64)
    xx = np.arange(W, dtype=np.float64)
    for y0 in range(0, H, 1024):
        blk = d32[y0:y0 + 1024].astype(np.float64)
        yy = np.arange(y0, y0 + blk.shape[0], dtype=np.float64)[:, None]
        v = blk + 1e-3 * np.sin(0.3 * yy + 0.2 * xx) + 1e-7 * xx
        out[y0:y0 + 1024] = np.where(blk == -100, -100.0, v)
    return out


def time_chain(dem, heights, px, steps, warmup):
    H, W = dem.shape
    st = torch.cuda.Stream()
    ctx = Context(0, st.cuda_stream)
    with torch.cuda.stream(st):
        d = ctx.to_device(dem)
        ch = chain.Chain(H, W, ctx=ctx, px=px, overlap=False, tune_placement=False, want_slope_rad=False,
                         heights=heights)
        ops = ch.ops(d.ptr, want_a_river=False, serial=True)
        for _ in range(warmup):
            for _, _, fn in ops:
                _lib.check(fn())
        ctx.sync()
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(len(ops) + 1)]
              for _ in range(steps)]
        for k in range(steps):
            ev[k][-1][0].record(st)
            for i, (_, _, fn) in enumerate(ops):
                ev[k][i][0].record(st)
                _lib.check(fn())
                ev[k][i][1].record(st)
            ev[k][-1][1].record(st)
        ctx.sync()
        ctx.raise_on_status()

        def ms(i):
            return round(float(np.median([ev[k][i][0].elapsed_time(ev[k][i][1]) for k in range(steps)])), 4)
        res = {"ms_per_step": ms(len(ops)), "per_op_ms": {n: ms(i) for i, (n, _, _) in enumerate(ops)}}
        ch.free()
        d.free()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, px = a.n, 10.0
    t0 = time.perf_counter()
    d32 = oracle.synth_dem(1, n, n)
    d64 = dem64_of(d32)
    t_gen = time.perf_counter() - t0
    r32 = time_chain(d32, "float32", px, a.steps, a.warmup)
    r64 = time_chain(d64, "float64", px, a.steps, a.warmup)
    N = n * n
    bpc = {name: b for name, b, _ in chain.OPS_F64}
    for r, ops in ((r32, chain.OPS), (r64, chain.OPS_F64)):
        r["GB_s_per_op"] = {name: round(N * b / (r["per_op_ms"][name] * 1e-3) / 1e9, 1)
                            for name, b, _ in ops if r["per_op_ms"].get(name)}
    out = {
        "tool": "chain_f64_bench", "raster": "%dx%d synthetic (oracle.synth_dem seed 1)" % (n, n), "cells": N,
        "steps": a.steps, "warmup": a.warmup, "timing": "median of HIP events on the launch stream, ops(serial=True)",
        "float32": r32, "float64": r64, "f64_over_f32": round(r64["ms_per_step"] / r32["ms_per_step"], 3),
        "bytes_per_cell_f64_ops": bpc, "dem_gen_s": round(t_gen, 1),
        "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
