"""Euclidean nearest-river distance and allocation at three source patterns, beside the flow-path
HAND on the same raster, in one process: proximity.nearest_river on (a) the chain's river network of the benchmark
terrain (dt_dev_synth_dem, bench.py's seed and threshold, 16384^2 by default, px = 10), (b) a single source in one
corner, (c) every cell a source; then proximity.euclidean_hand and flowhand.flow_hand_index on (a), the user-facing
comparison.  The work bound of the op says (b) and (c) cost no more than a small factor over (a).

These are host-tier calls: each time is the wall clock of the whole call, uploads and downloads included (1 B/cell up,
12 B/cell down for nearest_river), the median of --steps after --warmup.  The device time of the passes alone comes
from running this tool under `rocprofv3 --kernel-trace --stats` (k_px_mark / k_px_carry / k_px_row: the row pass,
k_px_col: the column pass, one launch per level).  (b) and (c) are checked against their closed forms.  Prints one JSON
line (and writes it to --out)."""
import numpy as np
import torch

import _bench
from descriptools_amd import flowhand, proximity


def main(argv=None):
    a = _bench.parser(steps=5, warmup=1).parse_args(argv)
    H = W = a.size
    px = 10.0
    # the benchmark terrain as host arrays: dem float32, fdr uint8, river int8
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        ter = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem", "fdr", "river"), px)
        dem, fdr, network = (r.cpu().numpy() for r in ter.values())
    del ter
    ctx.close()
    corner = np.zeros((H, W), np.int8)
    corner[0, 0] = 1
    every = np.ones((H, W), np.int8)

    # the closed forms of (b) and (c)
    got = proximity.nearest_river(corner, px)
    rows = np.unique(np.linspace(0, H - 1, 9).astype(np.int64))
    xx = np.arange(W, dtype=np.int64)
    for y in rows:
        assert not got.indices[y].any()
        assert np.array_equal(got.distance[y], (px * np.sqrt((y * y + xx * xx).astype(np.float64))).astype(np.float32))
    got = proximity.nearest_river(every, px)
    for y in rows:
        assert np.array_equal(got.indices[y], y * W + xx) and not got.distance[y].any()
    del got

    ops = (("nearest_river_network", lambda: proximity.nearest_river(network, px)),
           ("nearest_river_one_corner", lambda: proximity.nearest_river(corner, px)),
           ("nearest_river_every_cell", lambda: proximity.nearest_river(every, px)),
           ("euclidean_hand_network", lambda: proximity.euclidean_hand(dem, network, px)),
           ("flow_hand_index_network", lambda: flowhand.flow_hand_index(dem, fdr, network, px)))
    t = {name: _bench.timed(fn, a.steps, a.warmup) for name, fn in ops}
    med = {k: _bench.median(v) for k, v in t.items()}
    res = {"tool": "proximity_bench", "size": [H, W], "seed": a.seed, "px": px, "steps": a.steps, "warmup": a.warmup,
           "timing": "wall clock of the whole host-tier call (uploads, kernels, downloads), median",
           "network_cells": int(network.sum()), "ms": {k: round(v, 2) for k, v in med.items()},
           "ms_min_max": {k: _bench.summary(v, 2)[1] for k, v in t.items()},
           "one_corner_over_network": round(med["nearest_river_one_corner"] / med["nearest_river_network"], 3),
           "every_cell_over_network": round(med["nearest_river_every_cell"] / med["nearest_river_network"], 3),
           "euclidean_hand_over_flow_hand_index": round(med["euclidean_hand_network"] / med["flow_hand_index_network"],
                                                        3),
           "scratch_bytes_per_cell": 8, "closed_forms_checked": True, "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)


if __name__ == "__main__":
    main()
