"""GPU (-m gpu): decayed, retention-limited and transport-limited accumulation (descriptools_amd.routing, dt_mfd_route,
dt_dinf_route and the device tier; the MODE instances of k_mf_* / k_di_* and cd_transfer in dt_countdown.h) against
the integer reference (tests/_routing_ref.py).  Every comparison is on bytes, and on all four outputs."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
from descriptools_amd import dinf, mfd, routing

import _dinf_ref as D
import _mfd_ref as M
import _routing_ref as R
from test_routing_host import chain_inputs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PX = 10.0
INF = float("inf")
MODES = ("decay", "retain", "limit")
IDENTITY = {"decay": 1.0, "retain": 0.0, "limit": INF}
MODE_ID = routing.TRANSFERS
NOT_CONVERGED, BAD_PARAM = 2, 512


def _bits_equal(name, g, r):
    assert g.dtype == r.dtype and g.shape == r.shape, name
    if g.dtype.kind == "f":
        g, r = g.view(np.int64), r.view(np.int64)
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        i = tuple(bad[0])
        raise AssertionError("%s: %d values differ, first at %s: got %r, reference %r"
                             % (name, len(bad), i, g[i], r[i]))


def _all_equal(name, got, ref):
    for k in R.OUTPUTS:
        assert got[k].dtype == np.float64
        _bits_equal("%s, %s" % (name, k), got[k], ref[k])


def ref_flow(flow):
    """the raster the reference takes: D8 codes go through the single-receiver shares"""
    return M.d8_shares(flow) if flow.ndim == 2 and flow.dtype == np.uint8 else flow


def check_route(name, flow, param, transfer, w=None, fb=None):
    """all four outputs of the host tier against the reference -> (the reference's outputs, its bookkeeping)"""
    got = routing.route(flow, param, transfer, w, fb, outputs=R.OUTPUTS)
    ref, x = R.route(ref_flow(flow), param, transfer, w, fb, full=True)
    assert list(got) == list(R.OUTPUTS) and set(got.info) >= {"rounds", "queue_high", "queued"}
    _all_equal(name, got, ref)
    return ref, x


# ---- the hand-worked chains -----------------------------------------------------------------------------------------
def _dev_route(entry, flow, w, p, fb, mode, rounds=64):
    from descriptools_amd import _lib, device
    H, W = flow.shape[:2]
    ctx = device.Context()
    bufs = [ctx.to_device(flow), ctx.to_device(w), ctx.to_device(p)] + [ctx.empty((H, W), np.float64) for _ in range(4)]
    try:
        _lib.check(getattr(_lib.lib(), entry)(ctx.h, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, H, W, fb, mode, rounds,
                                              *(b.ptr for b in bufs[3:])))
        status = ctx.status()
        return status, dict(zip(R.OUTPUTS, (b.to_host() for b in bufs[3:])))
    finally:
        for b in bufs:
            b.free()
        ctx.close()


@pytest.mark.parametrize("transfer", MODES)
def test_hand_worked_chains_on_both_tiers(transfer):
    fdr, w, p, want = chain_inputs(transfer)
    shares, angle = mfd.d8_shares(fdr), D.d8_angles(fdr)
    for name, flow in (("codes", fdr), ("shares", shares), ("angles", angle)):
        _all_equal(name, routing.route(flow, p, transfer, w, 0, outputs=R.OUTPUTS), want)
    for entry, flow in (("dt_dev_mfd_route", shares), ("dt_dev_dinf_route", angle)):
        status, got = _dev_route(entry, flow, w, p, 0, MODE_ID[transfer])
        assert status == 0
        _all_equal(entry, got, want)
    if transfer == "decay":
        assert np.array_equal(routing.decayed_accumulation(fdr, p, w, 0), want["load"])
    if transfer == "retain":
        out, kept = routing.retention_limited(angle, p, w, 0)
        assert np.array_equal(out, want["outflow"]) and np.array_equal(kept, want["retained"])
    if transfer == "limit":
        tla, tdep = routing.transport_limited(shares, w, p, 0)
        assert np.array_equal(tla, want["outflow"]) and np.array_equal(tdep, want["retained"])


# ---- terrain ---------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def terrain_flow(kind, H, W, nodata_pct):
    """MFD shares (exponent 1: the reference's shares are exact), D-infinity angles or D8 codes of a terrain"""
    dem = oracle.synth_dem(11, H, W, nodata_pct=nodata_pct)
    if kind == "mfd":
        f = M.flow_shares(dem, 1)
    elif kind == "dinf":
        f = D.flow_direction(dem, PX)[0]
    else:
        f = np.ascontiguousarray(oracle.slope_d8(dem, PX)[1], np.uint8)
    f.setflags(write=False)
    return f


@functools.lru_cache(maxsize=None)
def terrain_weights(H, W):
    w = np.random.default_rng(H + W).uniform(0, 4, (H, W))
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def identity_load(kind, H, W, nodata_pct):
    """the load of the reference when nothing is held back, and its median over the cells that complete"""
    load = R.route(ref_flow(terrain_flow(kind, H, W, nodata_pct)), np.ones((H, W)), "decay",
                   terrain_weights(H, W))["load"]
    return load, float(np.median(load[load != -100]))


def terrain_param(kind, H, W, nodata_pct, transfer):
    """a tenth exact 0, a tenth the other exact end (1, +inf), the rest decays in [0.5, 1) or capacities around the
    median load"""
    rng = np.random.default_rng(17 + len(transfer))
    pick = rng.random((H, W))
    if transfer == "decay":
        p = rng.uniform(0.5, 1.0, (H, W))
        p[pick < 0.1], p[pick > 0.9] = 0.0, 1.0
        return p
    med = identity_load(kind, H, W, nodata_pct)[1]
    p = med * rng.uniform(0.0, 1.0, (H, W)) ** 2 * 2.0
    p[pick < 0.1], p[pick > 0.9] = 0.0, INF
    return p


@pytest.mark.parametrize("H,W,nodata_pct", [(200, 333, 0), (200, 333, 2), (600, 1000, 0)])
@pytest.mark.parametrize("transfer", MODES)
@pytest.mark.parametrize("kind", ["mfd", "dinf", "d8"])
def test_terrain(kind, transfer, H, W, nodata_pct):
    flow, w = terrain_flow(kind, H, W, nodata_pct), terrain_weights(H, W)
    p = terrain_param(kind, H, W, nodata_pct, transfer)
    assert (p == 0).mean() > 0.05 and (p == IDENTITY["decay" if transfer == "decay" else "limit"]).mean() > 0.05
    ref, x = check_route("%s %s %dx%d" % (kind, transfer, H, W), flow, p, transfer, w)
    done = x["done"]
    assert done.sum() == (~x["nodata"]).sum(), "a terrain has no cycle"
    if kind != "d8":
        assert x["nodata"].any() == (nodata_pct > 0)
    T, O = x["T"][done], x["O"][done]
    if transfer == "decay":
        assert (O < T).mean() > 0.5 and (O == T).mean() > 0.05
    else:  # both branches of the capacity, each on a tenth of the valid cells at least
        first = (O > 0) if transfer == "retain" else (O < T)   # above the capacity: spills / is cut
        share = float(first.mean())
        print("%s %s %dx%d: %.1f %% of the cells above their capacity" % (kind, transfer, H, W, 100 * share))
        assert 0.1 <= share <= 0.9


# ---- identities ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", MODES)
def test_identity_parameters_give_the_accumulations(transfer):
    H, W = 200, 333
    w = terrain_weights(H, W)
    p = np.full((H, W), IDENTITY[transfer])
    s, a = terrain_flow("mfd", H, W, 2), terrain_flow("dinf", H, W, 2)
    for flow, acc in ((s, mfd.accumulate(s, w)), (a, dinf.accumulate(a, w))):
        got = routing.route(flow, p, transfer, w, outputs=R.OUTPUTS)
        _bits_equal("inflow", got["inflow"], acc)
        _bits_equal("outflow is the load", got["outflow"], got["load"])
        assert (got["retained"][acc != -100] == 0).all() and (got["retained"][acc == -100] == -100).all()
    from descriptools_amd import flowacc
    fdr = terrain_flow("d8", 600, 1000, 0)
    got = routing.route(fdr, np.full(fdr.shape, IDENTITY[transfer]), transfer, frac_bits=0, outputs=("inflow",))
    acc = flowacc.accumulate(fdr)
    _bits_equal("D8 codes against flowacc", got["inflow"], acc.astype(np.float64))


# ---- depth -----------------------------------------------------------------------------------------------------------
def _serpentine(H=257, W=256):
    fdr = np.empty((H, W), np.uint8)
    fdr[0::2, :], fdr[1::2, :] = 1, 16
    fdr[0::2, -1] = fdr[1::2, 0] = 4
    fdr[-1, -1] = 0
    order = np.arange(H * W).reshape(H, W)
    order[1::2] = order[1::2, ::-1]
    return fdr, order.reshape(-1)   # order[c] = the position of cell c along the chain


def _chain_recurrence(transfer, q, Q):
    """Python integers down one chain: -> (T, O) lists by position"""
    T, O, carry = [], [], 0
    for qi, Qi in zip(q, Q):
        t = int(qi) + carry
        carry = R.transfer_exact(transfer, t, Qi)
        T.append(t)
        O.append(carry)
    return T, O


def _along(order, values, fb):
    """values by position -> float64 raster"""
    by_pos = np.ldexp(np.array(values, np.float64), -fb)
    return by_pos[order]


@pytest.mark.parametrize("transfer", ["decay", "retain"])
def test_serpentine_depth(transfer):
    """one chain through every cell of 257 x 256 (65,791 moves) against a Python-integer recurrence: a constant decay
    of 0.5 on integer weights, and capacities that empty the chain (+inf every 997th cell) and let it refill"""
    fdr, order = _serpentine()
    H, W = fdr.shape
    fb = 20
    rng = np.random.default_rng(4)
    w = rng.integers(0, 1000, (H, W))
    if transfer == "decay":
        p = np.full((H, W), 0.5)
    else:
        p = rng.uniform(0, 1200, (H, W))
        p.reshape(-1)[np.flatnonzero(order % 997 == 996)] = INF
    pos = np.argsort(order)  # pos[i] = the cell at position i
    q = (w.reshape(-1)[pos].astype(np.int64) << fb)
    Q = R.quantise_param(transfer, p.reshape(-1)[pos], fb)[0]
    T, O = _chain_recurrence(transfer, q, Q)
    if transfer == "retain":
        assert sum(1 for o in O if o == 0) > 66 and sum(1 for o in O if o > 0) > H * W // 4
    want = {"inflow": _along(order, [t - int(qi) for t, qi in zip(T, q)], fb).reshape(H, W),
            "load": _along(order, T, fb).reshape(H, W), "outflow": _along(order, O, fb).reshape(H, W),
            "retained": _along(order, [t - o for t, o in zip(T, O)], fb).reshape(H, W)}
    for flow in (fdr, D.d8_angles(fdr)):
        _all_equal("serpentine", routing.route(flow, p, transfer, w, fb, outputs=R.OUTPUTS), want)


# ---- the width of the decay product ---------------------------------------------------------------------------------
def test_decay_product_needs_more_than_64_bits():
    """1 x 64, every weight quantises to 2^52 / 64 and D = 2^30 - 1: the loads pass 2^34, from where T * D no longer
    fits 64 bits; the split product of the definition is exact"""
    n, fb = 64, 46
    fdr = np.full((1, n), 1, np.uint8)
    w = np.ones((1, n))
    d = (2.0 ** 30 - 1) / 2.0 ** 30
    p = np.full((1, n), d)
    q = [1 << 46] * n
    T, O = _chain_recurrence("decay", q, [(1 << 30) - 1] * n)
    assert T[-1] * ((1 << 30) - 1) >= 1 << 64 and max(T) <= 1 << 52
    assert any(((t * ((1 << 30) - 1)) & ((1 << 64) - 1)) >> 30 != o for t, o in zip(T, O)), "a wrapped product differs"
    ident = np.arange(n)
    want = {"inflow": _along(ident, [t - (1 << 46) for t in T], fb).reshape(1, n),
            "load": _along(ident, T, fb).reshape(1, n), "outflow": _along(ident, O, fb).reshape(1, n),
            "retained": _along(ident, [t - o for t, o in zip(T, O)], fb).reshape(1, n)}
    for flow in (fdr, mfd.d8_shares(fdr), D.d8_angles(fdr)):
        _all_equal("wide product", routing.route(flow, p, "decay", w, fb, outputs=R.OUTPUTS), want)
        _all_equal("wide product, the reference", R.route(ref_flow(flow), p, "decay", w, fb), want)


# ---- forced spill ----------------------------------------------------------------------------------------------------
_CHILD = """
import sys
import numpy as np
sys.path.insert(0, %r)
from descriptools_amd import routing
z = np.load(sys.argv[1])
out = {}
for t in ("decay", "retain", "limit"):
    r = routing.route(z["flow"], z[t], t, z["w"], outputs=("inflow", "load", "outflow", "retained"))
    for k, v in r.items():
        out[t + "_" + k] = v
    print("INFO", t, r.info["rounds"], r.info["queued"], r.info["queue_high"])
np.savez(sys.argv[2], **out)
"""


def _spill_params(H, W, med):
    rng = np.random.default_rng(21)
    return {"decay": rng.uniform(0.6, 1.0, (H, W)), "retain": med * rng.uniform(0, 1.5, (H, W)),
            "limit": med * rng.uniform(0.5, 4.0, (H, W))}


@pytest.mark.parametrize("kind", ["mfd", "dinf"])
def test_forced_spill_gives_the_same_bytes(kind, tmp_path):
    """three receivers per cell (the plane's shares) / two (a constant angle between E and NE): a fresh process with
    the lane's stack capped at one cell runs the spill queue and several rounds"""
    H, W = 300, 500
    if kind == "mfd":
        yy, xx = np.mgrid[0:H, 0:W]
        flow = M.flow_shares((3000 - yy - xx).astype(np.float32), 1)
        assert ((flow[1:-1, 1:-1] > 0).sum(axis=2) == 3).all()
    else:
        flow = np.full((H, W), 0.3, np.float32)
        assert (D.decode(flow)[0] == 2).all()
    w = np.random.default_rng(5).uniform(0, 2, (H, W))
    base = R.route(flow, np.ones((H, W)), "decay", w)["load"]
    params = _spill_params(H, W, float(np.median(base)))
    default = {t: routing.route(flow, params[t], t, w, outputs=R.OUTPUTS) for t in MODES}
    for t in MODES:
        _all_equal("default run, " + t, default[t], R.route(flow, params[t], t, w))
    np.savez(tmp_path / "in.npz", flow=flow, w=w, **params)
    env = dict(os.environ, **{"DT_DBG_MFD_STACK" if kind == "mfd" else "DT_DBG_DINF_STACK": "1"})
    out = subprocess.run([sys.executable, "-c", _CHILD % ROOT, str(tmp_path / "in.npz"), str(tmp_path / "out.npz")],
                         env=env, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    got = np.load(tmp_path / "out.npz")
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("INFO")]
    assert [ln[1] for ln in lines] == list(MODES)
    for ln in lines:
        rounds, queued = int(ln[2]), int(ln[3])
        print("forced spill %s %s: %d rounds, %d cells queued" % (kind, ln[1], rounds, queued))
        assert queued > 0 and rounds >= 2, "the spill path did not run"
        _all_equal("forced spill, " + ln[1], {k: got[ln[1] + "_" + k] for k in R.OUTPUTS}, default[ln[1]])


# ---- cycles ----------------------------------------------------------------------------------------------------------
CYCLES = ((10, 10), (63, 127), (150, 300), (127, 63))   # the second and the fourth lie across tile borders


@pytest.mark.parametrize("transfer", MODES)
def test_cycles_give_minus_100_in_all_four_outputs(transfer):
    U = 32768
    s = terrain_flow("mfd", 200, 333, 2).copy()
    for y, x in CYCLES:
        s[y:y + 2, x:x + 2] = 0
        s[y, x, 0] = s[y + 1, x + 1, 4] = s[y + 1, x, 2] = s[y, x + 1, 6] = U   # E, S, W, N: clockwise
    y, x = CYCLES[1]
    s[y, x + 1, 6], s[y, x + 1, 0] = U - 9000, 9000   # part of this one leaks out to the east
    p = terrain_param("mfd", 200, 333, 2, transfer)
    w = terrain_weights(200, 333)
    got = routing.route(s, p, transfer, w, outputs=R.OUTPUTS)
    ref, xr = R.route(s, p, transfer, w, full=True)
    _all_equal("cycles", got, ref)
    base = R.route(terrain_flow("mfd", 200, 333, 2), p, transfer, w)
    for k in R.OUTPUTS:
        for y, x in CYCLES:
            assert (got[k][y:y + 2, x:x + 2] == -100).all(), k
        y, x = CYCLES[1]
        assert got[k][y, x + 2] == -100, "the cell the leak feeds never completes"
        assert np.array_equal(got[k] == -100, got["load"] == -100)
    lost = (got["load"] == -100) & (base["load"] != -100)
    assert lost.sum() > 16 and (got["load"] != -100).sum() > 0.5 * got["load"].size


# ---- mass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transfer", MODES)
@pytest.mark.parametrize("kind", ["mfd", "dinf"])
def test_mass_is_conserved_with_nodata_holes(kind, transfer):
    """the sum of q = what the cells keep + what leaves the domain, in integers, the right side from the device's
    rasters: R from `retained`, and the split of the device's `outflow` along the shares that point off the raster or
    into nodata (a cell without a receiver sends all of it)"""
    flow = terrain_flow(kind, 200, 333, 2)[20:180, 30:300].copy()   # cut out: shares along the rim point off it
    flow[70:90, 100:140] = 0xFFFF if kind == "mfd" else -100        # a lake: shares around it point into nodata
    H, W = flow.shape[:2]
    w = np.random.default_rng(9).uniform(0, 5, (H, W))
    med = float(np.median(R.route(flow, np.ones((H, W)), "decay", w)["load"]))
    p = _spill_params(H, W, max(med, 1.0))[transfer]
    fb = D.default_frac_bits(H * W, float(w.max()))
    got = routing.route(flow, p, transfer, w, fb, outputs=R.OUTPUTS)
    live = (got["load"] != -100).reshape(-1)
    q = D.quantise(w, (H, W), fb)

    def ints(name):
        return np.where(live, np.rint(np.ldexp(got[name].reshape(-1), fb)).astype(np.int64), 0)

    O, kept = ints("outflow"), ints("retained")
    if kind == "mfd":
        P, nod, _, edge, gone = M.graph(flow)
        sent = M.split(O, P)
        left = int(sent[gone].sum()) + int(O[~(P > 0).any(axis=1)].sum())
    else:
        r0, r1, p2, gone0, gone1 = D.receivers(flow)
        nod = (flow == np.float32(-100)).reshape(-1)
        m2 = D.share(O, p2)
        m1 = O - m2
        left = int(m1[r0 < 0].sum()) + int(m2[gone1].sum())   # no first edge: the share, or all of O, leaves
    assert np.array_equal(live, ~nod), "no cycle: every cell that is not nodata completes"
    assert left > 0 and int(kept.sum()) > 0
    assert int(q[live].sum()) == int(kept.sum()) + left
    assert np.array_equal(ints("load"), kept + O)
    assert np.array_equal(ints("inflow"), np.where(live, ints("load") - q, 0))


# ---- the device tier -------------------------------------------------------------------------------------------------
def test_device_tier_on_a_chain():
    """dt_dev_mfd_route / dt_dev_dinf_route on the shares and angles made from a conditioning Chain's filled surface
    and codes, nothing synchronising in between: equal to the host tier; *_accumulate_info reports the run"""
    from descriptools_amd import _lib, chain, device
    H, W = 320, 448
    dem = oracle.synth_dem(9, H, W, nodata_pct=1).copy()
    dem[100:140, 200:260][dem[100:140, 200:260] > -100] -= 30
    dem = np.ascontiguousarray(dem, np.float32)
    rng = np.random.default_rng(2)
    w = rng.uniform(0, 3, (H, W))
    params = {"decay": rng.uniform(0.3, 1.0, (H, W)), "retain": rng.uniform(0, 40, (H, W)),
              "limit": rng.uniform(0, 400, (H, W))}
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=PX, overlap=False, tune_placement=False, river_threshold=200, condition=True,
                     condition_rounds=500)
    L = _lib.lib()
    bufs = {"dem": ctx.to_device(dem), "w": ctx.to_device(w), "shr": ctx.empty((H, W, 8), np.uint16),
            "ang": ctx.empty((H, W), np.float32)}
    for t in MODES:
        bufs[t] = ctx.to_device(params[t])
    for k in R.OUTPUTS:
        bufs[k] = ctx.empty((H, W), np.float64)
    outs = [bufs[k].ptr for k in R.OUTPUTS]
    got, info = {}, np.zeros(4, np.int64)
    try:
        ch.run(bufs["dem"].ptr)
        _lib.check(L.dt_dev_mfd_shares(ctx.h, ch.p("filled"), ch.p("fdr"), H, W, 1.0, 0, bufs["shr"].ptr))
        _lib.check(L.dt_dev_dinf_direction(ctx.h, ch.p("filled"), ch.p("fdr"), H, W, PX, bufs["ang"].ptr, None))
        for entry, flow, info_entry in (("dt_dev_mfd_route", "shr", "dt_dev_mfd_accumulate_info"),
                                        ("dt_dev_dinf_route", "ang", "dt_dev_dinf_accumulate_info")):
            for t in MODES:
                _lib.check(getattr(L, entry)(ctx.h, bufs[flow].ptr, bufs["w"].ptr, bufs[t].ptr, H, W, 24, MODE_ID[t],
                                             512, *outs))
                assert ctx.status() == 0
                _lib.check(getattr(L, info_entry)(ctx.h, info.ctypes.data_as(_lib.c_i64p)))
                assert info[3] > 0 and info[2] >= info[1] >= 0 and info[0] < 512
                got[flow, t] = {k: bufs[k].to_host() for k in R.OUTPUTS}
        # a subset of the outputs
        _lib.check(L.dt_dev_mfd_route(ctx.h, bufs["shr"].ptr, bufs["w"].ptr, bufs["limit"].ptr, H, W, 24, 3, 512,
                                      None, None, None, bufs["retained"].ptr))
        only = bufs["retained"].to_host()
        shares, angle = bufs["shr"].to_host(), bufs["ang"].to_host()
    finally:
        for b in bufs.values():
            b.free()
        ch.free()
        ctx.close()
    _bits_equal("one output", only, got["shr", "limit"]["retained"])
    for flow, raster in (("shr", shares), ("ang", angle)):
        for t in MODES:
            host = routing.route(raster, params[t], t, w, 24, outputs=R.OUTPUTS)
            _all_equal("%s %s against the host tier" % (flow, t), got[flow, t], host)
            assert (host["load"] != -100).sum() > 0.9 * H * W


def test_device_tier_budget_bad_parameter_and_refusals():
    from descriptools_amd import _lib, device
    H, W = 65, 64
    fdr, _ = _serpentine(H, W)
    s, a = mfd.d8_shares(fdr), D.d8_angles(fdr)
    rng = np.random.default_rng(6)
    w = rng.uniform(0, 2, (H, W))
    p = rng.uniform(0.5, 1.0, (H, W))
    ref = R.route(s, p, "decay", w, 30)
    ctx = device.Context()
    L = _lib.lib()
    ds, da, dw, dp = ctx.to_device(s), ctx.to_device(a), ctx.to_device(w), ctx.to_device(p)
    o = [ctx.empty((H, W), np.float64) for _ in range(4)]
    ptrs = [b.ptr for b in o]
    try:
        for entry, flow in (("dt_dev_mfd_route", ds), ("dt_dev_dinf_route", da)):
            call = getattr(L, entry)
            # a budget of two rounds leaves queued work on the serpentine; negative budgets carry on to the same bytes
            _lib.check(call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 30, 1, 2, *ptrs))
            assert ctx.status() & NOT_CONVERGED
            part = o[1].to_host()
            assert (part == -100).any() and ((part == ref["load"]) | (part == -100)).all()
            calls = 0
            while True:
                _lib.check(call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 30, 1, -8, *ptrs))
                calls += 1
                if not ctx.status() & NOT_CONVERGED:
                    break
                assert calls < 100
            assert calls >= 2
            # a continuation names what it was started with, the parameter raster and the mode included
            assert call(ctx.h, flow.ptr, dw.ptr, dw.ptr, H, W, 30, 1, -1, *ptrs) != 0
            assert call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 30, 2, -1, *ptrs) != 0
            assert call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 29, 1, -1, *ptrs) != 0
            acc = L.dt_dev_mfd_accumulate if entry == "dt_dev_mfd_route" else L.dt_dev_dinf_accumulate
            assert acc(ctx.h, flow.ptr, dw.ptr, H, W, 30, -1, ptrs[0]) != 0, "an accumulation does not continue a run"
            assert call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 30, 1, -1, *ptrs) == 0
            _all_equal(entry + " continued", dict(zip(R.OUTPUTS, (b.to_host() for b in o))), ref)
            _lib.check(acc(ctx.h, flow.ptr, dw.ptr, H, W, 30, 2, ptrs[0]))
            assert call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 30, 1, -1, *ptrs) != 0, "nor a run an accumulation"
            ctx.status()
            # the refusals
            assert call(ctx.h, flow.ptr, dw.ptr, None, H, W, 30, 1, 64, *ptrs) != 0                 # NULL param
            assert b"param is NULL" in L.dt_last_error()
            for mode in (0, 4, -1):
                assert call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 30, mode, 64, *ptrs) != 0       # unknown mode
            assert call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 30, 1, 64, None, None, None, None) != 0
            assert b"all four outputs are NULL" in L.dt_last_error()
            for alias in (flow, dw, dp):                                                       # an output is an input
                for slot in range(4):
                    args = list(ptrs)
                    args[slot] = alias.ptr
                    assert call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 30, 1, 64, *args) != 0
            assert call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 30, 1, 64, ptrs[0], ptrs[0], None, None) != 0
            assert call(ctx.h, flow.ptr, dw.ptr, dp.ptr, H, W, 30, 1, 0, *ptrs) != 0               # rounds 0
            assert call(ctx.h, None, None, None, 0, 0, 0, 1, 1, None, None, None, None) == 0        # no cells
        # a parameter outside the contract: the status bit, and the cell passes everything on
        for transfer, bad in (("decay", np.nan), ("decay", 1.5), ("retain", -1.0), ("limit", np.nan)):
            b = p.copy() if transfer == "decay" else p * 3
            b[33, 40] = bad
            with pytest.raises(ValueError):
                routing.route(s, b, transfer, w, 30)
            db = ctx.to_device(b)
            for entry, flow, raster in (("dt_dev_mfd_route", ds, s), ("dt_dev_dinf_route", da, a)):
                _lib.check(getattr(L, entry)(ctx.h, flow.ptr, dw.ptr, db.ptr, H, W, 30, MODE_ID[transfer], 256, *ptrs))
                assert ctx.status() == BAD_PARAM
                _all_equal("bad parameter as the identity", dict(zip(R.OUTPUTS, (x.to_host() for x in o))),
                           R.route(raster, b, transfer, w, 30))
            db.free()
        _lib.check(L.dt_dev_mfd_route(ctx.h, ds.ptr, dw.ptr, dp.ptr, H, W, 30, 1, 256, *ptrs))
        assert ctx.status() == 0
    finally:
        for b in [ds, da, dw, dp] + o:
            b.free()
        ctx.close()


# ---- two runs --------------------------------------------------------------------------------------------------------
def test_two_runs_give_identical_bytes():
    for kind in ("mfd", "dinf"):
        flow, w = terrain_flow(kind, 600, 1000, 0), terrain_weights(600, 1000)
        for t in MODES:
            p = terrain_param(kind, 600, 1000, 0, t)
            runs = [routing.route(flow, p, t, w, outputs=R.OUTPUTS) for _ in range(2)]
            _all_equal("%s %s, repeated" % (kind, t), runs[1], runs[0])


# ---- end to end ------------------------------------------------------------------------------------------------------
def _pitted(H=256, W=256):
    dem = oracle.synth_dem(5, H, W, nodata_pct=1).copy()
    rng = np.random.default_rng(8)
    for _ in range(60):
        y, x = int(rng.integers(3, H - 3)), int(rng.integers(3, W - 3))
        if (dem[y - 2:y + 3, x - 2:x + 3] > -100).all():
            dem[y - 1:y + 2, x - 1:x + 2] -= 25
            dem[y, x] -= 10
    return dem


def test_end_to_end_fill_and_spill():
    """the README's recipe on a pitted DEM: depressions fill from the rain on their catchments and spill on"""
    from descriptools_amd import flowdir
    dem = _pitted()
    fdr, filled = flowdir.d8_conditioned(dem, PX, return_filled=True)
    fb = 20   # one scale for the capacities and the routing: `retained == capacity` is then exact
    cap = routing.sink_capacity(dem, filled, fdr, PX, frac_bits=fb)
    exits = cap > 0
    assert exits.sum() >= 30
    full = {}
    for rain in (0.04, 0.4):
        w = np.where(dem > -100, rain * PX * PX, 0.0)
        outflow, retained = routing.retention_limited(fdr, cap, w, frac_bits=fb)
        ref = R.route(M.d8_shares(fdr), cap, "retain", w, fb)
        _bits_equal("outflow, rain %g" % rain, outflow, ref["outflow"])
        _bits_equal("retained, rain %g" % rain, retained, ref["retained"])
        assert (outflow != -100).all(), "conditioned codes have no cycle"
        assert (retained[~exits] == 0).all()
        spills = exits & (outflow > 0)
        assert (retained[spills] == cap[spills]).all(), "what spills has filled first"
        load = outflow + retained   # exact: both are multiples of 2^-20 below 2^32
        reached = exits & (load >= cap)
        assert (retained[reached] == cap[reached]).all() and (retained[exits & ~reached] < cap[exits & ~reached]).all()
        full[rain] = int(reached.sum())
        print("rain %g: %d of %d exits full, %d spill" % (rain, full[rain], exits.sum(), spills.sum()))
    assert full[0.4] >= full[0.04] and full[0.4] > 0
