"""D-infinity distance down to the stream beside the D-infinity accumulation and the D8 flow-path
HAND on the same rasters, in one process: the benchmark terrain (dt_dev_synth_dem, bench.py's seed, 16384^2 by
default, px = 10), angles from dt_dev_dinf_direction, the river network fac > N / 512 with fac = dinf.accumulate of
those angles, then dinf.distance_down (stat 'ave', heights given) under both edge rules, dinf.accumulate and
flowhand.flow_hand_index.

These are host-tier calls: each time is the wall clock of the whole call, uploads and downloads included (9 B/cell up
and 24 B/cell down for distance_down with heights), the median of --steps after --warmup; every call synchronises
before it returns.  For each edge rule the tool records the rounds that settled something, the cells that reach, are
dead or stay unsettled, the tile visits per tile and the bytes a visit moves, computed from the shapes.

The device time comes from a second run of its own, `rocprofv3 --kernel-trace --stats -- python
tools/dinf_distance_bench.py --profile-only` (one call of each op), summarised by `--trace DIR`: the dispatches are
grouped into calls at each k_dd_init, per call the span from the first launch to the last end, the three kernels'
totals and the rounds one by one (four launches, one per colour, each); the accumulation's k_di_* with the countdown's
k_cd_mark (no other op of this tool's run launches it) and the flow-path kernels of flow_hand_index beside them.
Prints one JSON line (and writes it to --out)."""
import ctypes
import csv
import glob
import json
import os

import numpy as np

import _bench

TILE = 32
# what one tile visit moves: the state and the height of tile and halo always; beside them at most the three values of
# every staged cell, the angle and state of the tile's own cells, and state and values of every cell written back
VISIT_BYTES_MIN = (TILE + 2) ** 2 * (1 + 4) + TILE * TILE
VISIT_BYTES_MAX = (TILE + 2) ** 2 * (1 + 4 + 24) + TILE * TILE * (1 + 4) + TILE * TILE * (1 + 24)


def summarise_trace(d, out_txt):
    f = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)[0]
    rows = sorted(csv.DictReader(open(f)), key=lambda r: int(r["Start_Timestamp"]))
    ker = [(r["Kernel_Name"], int(r["Start_Timestamp"]), int(r["End_Timestamp"])) for r in rows]
    calls, other = [], {}
    for name, t0, t1 in ker:
        if "k_dd_init" in name:
            calls.append([])
        if "k_dd_" in name:
            calls[-1].append((name, t0, t1))
        else:
            key = name.split("(")[0][:60]
            tot, n = other.get(key, (0, 0))
            other[key] = (tot + (t1 - t0), n + 1)
    lines, spans = [], []
    for i, c in enumerate(calls):
        span = (c[-1][2] - c[0][1]) * 1e-6
        spans.append(round(span, 3))
        tot = {}
        for name, t0, t1 in c:
            k = "k_dd_init" if "k_dd_init" in name else ("k_dd_final" if "k_dd_final" in name else "k_dd_round")
            a, n = tot.get(k, (0, 0))
            tot[k] = (a + (t1 - t0), n + 1)
        rounds = [t1 - t0 for name, t0, t1 in c if "k_dd_round" in name]
        per_round = [sum(rounds[j:j + 4]) * 1e-6 for j in range(0, len(rounds), 4)]
        lines.append("call %d  first launch to last end %.3f ms | %s | rounds (4 launches each), ms: %s" % (
            i, span, " ".join("%s %.3f (%d)" % (k, a * 1e-6, n) for k, (a, n) in sorted(tot.items())),
            " ".join("%.3f" % x for x in per_round)))
    lines.append("other kernels: total ms, launches")
    for k, (tot, n) in sorted(other.items(), key=lambda kv: -kv[1][0])[:24]:
        lines.append("%9.3f %4d %s" % (tot * 1e-6, n, k))
    for tag, pat in (("dinf.accumulate kernels (k_di_*, k_cd_mark)", ("k_di_", "k_cd_mark")),
                     ("flow_hand_index kernels (k_fh_*, k_i32_to_i64)", ("k_fh_", "k_i32_to_i64"))):
        pats = (pat,) if isinstance(pat, str) else pat
        tot = sum(t1 - t0 for name, t0, t1 in ker if any(p in name for p in pats))
        lines.append("%s in all: %.3f ms" % (tag, tot * 1e-6))
    text = "\n".join(lines) + "\n"
    if out_txt:
        with open(out_txt, "w") as fh:
            fh.write(text)
    print(text)
    return spans


def main(argv=None):
    ap = _bench.parser(steps=5, warmup=1)
    ap.add_argument("--profile-only", action="store_true", help="one call of each op and nothing else (for rocprofv3)")
    ap.add_argument("--trace", default=None, help="summarise the kernel trace under this directory and exit")
    ap.add_argument("--times", default=None, help="with --trace: the text file to write")
    a = ap.parse_args(argv)
    if a.trace:
        spans = summarise_trace(a.trace, a.times)
        if a.out and os.path.exists(a.out):
            res = json.loads(open(a.out).read())
            res["device_span_ms_by_call"] = spans
            res["device_span_note"] = ("rocprofv3 --kernel-trace run of --profile-only: first k_dd_init launch to "
                                       "k_dd_final end, calls in the order check_edges True, False")
            _bench.emit(res, a.out, show=False)
        return

    import torch
    from descriptools_amd import _lib, dinf, flowhand

    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        dem_d, fdr_d = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem", "fdr"), px).values()
        angle_d = torch.empty((H, W), dtype=torch.float32, device=dev)
        _lib.check(L.dt_dev_dinf_direction(ctx.h, dem_d.data_ptr(), None, H, W, px, angle_d.data_ptr(), None))
        ctx.sync()
        dem, fdr, angle = dem_d.cpu().numpy(), fdr_d.cpu().numpy(), angle_d.cpu().numpy()
    del dem_d, fdr_d, angle_d
    ctx.close()
    torch.cuda.empty_cache()

    fac = dinf.accumulate(angle)
    river = (fac > N / 512).astype(np.int8)
    del fac
    tiles = ((H + TILE - 1) // TILE) * ((W + TILE - 1) // TILE)
    visits = L.dt_dinf_distance_visits_  # the library's private diagnostic: this thread's last call
    visits.restype, visits.argtypes = ctypes.c_int64, []
    modes = {}

    def dist(check_edges):
        out, info = dinf._distance_down(angle, river, px, dem, "ave", check_edges, 0)
        info["tile_visits"] = int(visits())
        info["visits_per_tile"] = round(info["tile_visits"] / tiles, 3)
        modes["check_edges_%s" % check_edges] = info
        return out

    ops = (("distance_down_check_edges", lambda: dist(True)),
           ("distance_down_no_check_edges", lambda: dist(False)),
           ("dinf_accumulate", lambda: dinf.accumulate(angle)),
           ("flow_hand_index", lambda: flowhand.flow_hand_index(dem, fdr, river, px)))
    if a.profile_only:
        for _, fn in ops:
            fn()
        _bench.emit({"tool": "dinf_distance_bench", "profile_only": True, "modes": modes}, None)
        return
    t = {name: _bench.timed(fn, a.steps, a.warmup) for name, fn in ops}
    med = {k: _bench.median(v) for k, v in t.items()}
    res = {"tool": "dinf_distance_bench", "size": [H, W], "seed": a.seed, "px": px, "stat": "ave", "steps": a.steps,
           "warmup": a.warmup,
           "timing": "wall clock of the whole host-tier call (uploads, kernels, downloads), median",
           "river_cells": int(river.sum()), "non_nodata_cells": int((angle != -100).sum()),
           "ms": {k: round(v, 2) for k, v in med.items()},
           "ms_min_max": {k: _bench.summary(v, 2)[1] for k, v in t.items()},
           "modes": modes, "tile": [TILE, TILE], "tiles": tiles,
           "bytes_per_tile_visit_min_max": [VISIT_BYTES_MIN, VISIT_BYTES_MAX],
           "host_bytes_per_cell": {"distance_down": [4 + 1 + 4, 24], "dinf_accumulate": [4, 8],
                                   "flow_hand_index": [4 + 1 + 1, 4 + 8 + 4]},
           "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)


if __name__ == "__main__":
    main()
