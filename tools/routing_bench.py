"""Decayed, retention-limited and transport-limited accumulation beside the accumulations they are built on (DESIGN.md
4.30), in one process, on one stream: dt_dev_mfd_route and dt_dev_dinf_route in each mode against dt_dev_mfd_accumulate
and dt_dev_dinf_accumulate on the same share and angle rasters of the benchmark terrain (dt_dev_synth_dem, bench.py's
seed, 16384^2 by default, px = 10, unit weights).

Each mode runs three ways: with its identity parameter (decay 1, retain 0, limit +inf) and `inflow` as the only output
-- the accumulation's own result, so what it costs more is the parameter raster, read when a cell completes and again
in the out step: 16 bytes per cell; with the identity parameter and all four outputs, 24 bytes per cell more written;
and with a parameter that holds something back, all four outputs.  Beside them: a device copy that moves 16 bytes per
cell and one that moves 40 (dt_dev_membench_copy), what those extra bytes cost as a plain stream.

The ops alternate, each bracketed by HIP events with a sync after it; the medians of --steps are reported with the
min-max spread of each, every routing figure as a ratio to its accumulation of the same run, and `over_copy`: (routing
- accumulation) / the copy of its extra bytes.  The budget of rounds is sized once from a finished accumulation, as a
caller would.  Before timing, the identity runs are checked against the accumulation, cell for cell.  Prints one JSON
line (and writes it to --out)."""
import numpy as np
import torch

import _bench
from descriptools_amd import _args, _lib

MODES = {"decay": 1, "retain": 2, "limit": 3}
IDENTITY = {"decay": 1.0, "retain": 0.0, "limit": float("inf")}


def main(argv=None):
    ap = _bench.parser(steps=5, warmup=1)
    ap.add_argument("--rounds", type=int, default=0, help="budget of rounds; 0: 5/4 of what a first run needed, plus 16")
    a = ap.parse_args(argv)
    H = W = a.size
    N = H * W
    px = 10.0
    L = _lib.lib()
    ctx, st, dev = _bench.device()
    with torch.cuda.stream(st):
        dem = _bench.terrain(ctx, st, dev, a.size, a.seed, ("dem",))["dem"]
        angle = torch.empty((H, W), dtype=torch.float32, device=dev)
        shares = torch.empty((H, W, 8), dtype=torch.int16, device=dev)  # the bits of uint16
        _lib.check(L.dt_dev_dinf_direction(ctx.h, dem.data_ptr(), None, H, W, px, angle.data_ptr(), None))
        _lib.check(L.dt_dev_mfd_shares(ctx.h, dem.data_ptr(), None, H, W, 1.1, 0, shares.data_ptr()))
        ctx.sync()
        del dem
        ones = torch.ones((H, W), dtype=torch.float64, device=dev)
        acc = torch.empty((H, W), dtype=torch.float64, device=dev)
        outs = torch.empty((4, H, W), dtype=torch.float64, device=dev)
        gen = torch.Generator(device=dev).manual_seed(a.seed)
        u = torch.rand((H, W), dtype=torch.float64, device=dev, generator=gen)
        ident = {m: torch.full((H, W), v, dtype=torch.float64, device=dev) for m, v in IDENTITY.items()}
        active = {"decay": 0.5 + 0.5 * u, "retain": 4.0 * u, "limit": 1.0 + 100.0 * u}
        del u
        s = _args._default_frac_bits(N, 1.0)
        flows = {"mfd": (L.dt_dev_mfd_accumulate, L.dt_dev_mfd_route, L.dt_dev_mfd_accumulate_info, shares),
                 "dinf": (L.dt_dev_dinf_accumulate, L.dt_dev_dinf_route, L.dt_dev_dinf_accumulate_info, angle)}
        budget = {k: a.rounds for k in flows}

        def budgeted(call, rounds):
            """`rounds` rounds as a caller enqueues them: a call takes 4096 at most, continuations take the rest"""
            call(min(rounds, 4096))
            for left in range(rounds - 4096, 0, -4096):
                call(-min(left, 4096))

        def accumulate(kind):
            entry, _, _, flow = flows[kind]

            def call(rounds=None):
                if rounds is None:
                    return budgeted(call, budget[kind])
                _lib.check(entry(ctx.h, flow.data_ptr(), ones.data_ptr(), H, W, s, rounds, acc.data_ptr()))
            return call

        def route(kind, mode, param, four):
            _, entry, _, flow = flows[kind]
            o = [outs[i].data_ptr() for i in range(4)] if four else [outs[0].data_ptr(), None, None, None]

            def call(rounds=None):
                if rounds is None:
                    return budgeted(call, budget[kind])
                _lib.check(entry(ctx.h, flow.data_ptr(), ones.data_ptr(), param.data_ptr(), H, W, s, MODES[mode],
                                 rounds, *o))
            return call

        def finish(call):
            """a first call with the largest budget, continued until nothing is queued"""
            call(4096)
            while ctx.status() & 2:
                call(-4096)

        def copy(floats, src, dst):
            blocks = -1 if floats % 65536 == 0 else 2048
            _lib.check(L.dt_dev_membench_copy(ctx.h, src.data_ptr(), dst.data_ptr(), floats, blocks))

        # the identity parameters reproduce the accumulation, and the budgets are sized from it
        info = np.zeros(4, np.int64)
        same, queue = {}, {}
        for kind in flows:
            finish(accumulate(kind))
            _lib.check(flows[kind][2](ctx.h, info.ctypes.data_as(_lib.c_i64p)))
            queue[kind] = [int(v) for v in info]
            if a.rounds <= 0:
                # which lane completes a cell varies run to run: so do the rounds
                budget[kind] = int(info[0]) * 5 // 4 + 16
            for mode in MODES:
                finish(route(kind, mode, ident[mode], True))
                same[kind + "_" + mode] = bool(torch.equal(outs[0], acc) and torch.equal(outs[1], outs[2]))
        assert all(same.values()), same

        ops = {}
        for kind in flows:
            ops[kind + "_accumulate"] = accumulate(kind)
            for mode in MODES:
                ops["%s_%s_identity_1" % (kind, mode)] = route(kind, mode, ident[mode], False)
                ops["%s_%s_identity_4" % (kind, mode)] = route(kind, mode, ident[mode], True)
                ops["%s_%s_active_4" % (kind, mode)] = route(kind, mode, active[mode], True)
        # 16 B per cell: 2N floats read and written; 40 B per cell: 5N floats, in two pieces
        ops["copy_16B"] = lambda: copy(2 * N, ones, outs[0])
        ops["copy_40B"] = lambda: (copy(4 * N, shares, outs), copy(N, ones, acc))
        _bench.events(ctx, st, ops, 0, a.warmup)
        status = ctx.status()
        t = _bench.events(ctx, st, ops, a.steps, 0)
        status |= ctx.status()
        converged = {}
        # the first call of a budget above 4096 rounds leaves work queued and raises DT_STATUS_NOT_CONVERGED before its
        # continuation finishes it: whether a run of the timed budget finishes is asked with one more round
        for kind in flows:
            last = route(kind, "limit", active["limit"], True)
            last()
            ctx.status()
            last(-1)
            converged[kind] = not ctx.status() & 2
    med = {k: _bench.median(v) for k, v in t.items()}
    ratios, over_copy = {}, {}
    for kind in flows:
        base = med[kind + "_accumulate"]
        for mode in MODES:
            for form, extra in (("identity_1", "copy_16B"), ("identity_4", "copy_40B"), ("active_4", "copy_40B")):
                k = "%s_%s_%s" % (kind, mode, form)
                ratios[k] = round(med[k] / base, 3)
                over_copy[k] = round((med[k] - base) / med[extra], 2)
    res = {"tool": "routing_bench", "size": [H, W], "seed": a.seed, "px": px, "frac_bits": s, "steps": a.steps,
           "warmup": a.warmup, "rounds_budget": budget,
           "timing": "median of HIP events around each op on its stream, ops alternating",
           "ms": {k: round(v, 3) for k, v in med.items()},
           "ms_min_max": {k: _bench.summary(v)[1] for k, v in t.items()},
           "over_accumulate": ratios, "over_copy": over_copy,
           "accumulate_spread_ms": {k: round(max(t[k + "_accumulate"]) - min(t[k + "_accumulate"]), 3) for k in flows},
           "queue_info4": queue, "status": status, "converged": converged, "identity_equals_accumulate": same,
           "device": torch.cuda.get_device_name(0)}
    _bench.emit(res, a.out)
    ctx.close()


if __name__ == "__main__":
    main()
