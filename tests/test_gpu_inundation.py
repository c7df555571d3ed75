"""GPU (-m gpu): inundation.simulate (dt_inundation, dt_dev_inundation, k_in_* in dt_inundation.hip) against the
contract of descriptools_amd/inundation.py: depth, qx, qy, max_depth, arrival, t and the step count are the bits of the
numpy restatement in tests/_inundation_ref.py; a lake at rest stays at rest exactly; depths stay >= 0 and the volume is
conserved; the open boundary drains; sync_every, the tier, a second run and a resume change no bit.

Shapes are the smallest at which the paths differ (tiles are 64 x 16 with a two-cell halo): one cell, one row, one
column, exactly one tile column (64 x 64: four tile rows), 63 x 65 and 65 x 129 (a seam each way, partial tiles),
129 x 70 with nodata walls, one of them on a tile seam.  No case takes more than about 1000 steps."""
import math

import numpy as np
import pytest

import _inundation_ref as R

pytestmark = pytest.mark.gpu

ALL = ("depth", "max_depth", "arrival")


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _same(got, ref, valid, px=10.0):
    """the package's result against the reference's, bit for bit"""
    assert got.info["steps"] == ref["steps"] and got.state["steps"] == ref["steps"]
    assert got.info["t"] == ref["t"] and got.state["t"] == ref["t"]
    assert got.info["finished"] == ref["finished"]
    for name in ("depth", "qx", "qy", "max_depth", "arrival"):
        diff = _bits(got.state[name]) != _bits(ref[name])
        assert not diff.any(), "%s differs on %d cells, first at %s" % (name, diff.sum(), np.argwhere(diff)[0])
    assert np.array_equal(_bits(got.depth), _bits(np.where(valid, ref["depth"], -100.0)))
    assert np.array_equal(_bits(got.max_depth), _bits(np.where(valid, ref["max_depth"], -100.0)))
    assert np.array_equal(_bits(got.arrival), _bits(ref["arrival"]))
    assert got.info["hmax"] == ref["hmax"] and got.info["dt_last"] == ref["dt_last"]
    assert got.info["dt_min"] == ref["dt_min"] and got.info["limited_steps"] == ref["limited_steps"]
    assert got.info["volume"] == math.fsum((ref["depth"][valid] * (px * px)).tolist())


def _run(dem, px, t_end, **kw):
    from descriptools_amd import inundation
    return inundation.simulate(dem, px, t_end, outputs=ALL, **kw)


def _ref(dem, valid, px, t_end, **kw):
    """the reference on what the package takes: float32 heights, float32 rasters of manning and rain"""
    for name in ("manning", "rain"):
        if name in kw and np.ndim(kw[name]):
            kw[name] = np.asarray(kw[name], np.float32).astype(np.float64)
    kw.pop("sync_every", None)
    return R.simulate(np.asarray(dem, np.float32).astype(np.float64), valid, px, t_end, **kw)


# ---- 1. parity ------------------------------------------------------------------------------------------------------
def _case(shape, variant):
    """rough tilted terrain with a pond, an inflow on a tile corner where the raster has one -> (dem, valid, kwargs)"""
    H, W = shape
    rng = np.random.default_rng(H * 1000 + W)
    y, x = np.mgrid[0:H, 0:W]
    dem = (0.03 * x + 0.02 * y + 0.4 * rng.random((H, W))).astype(np.float32)
    if shape == (129, 70):
        dem[10:60, 64 % W] = -100.0   # a wall along a tile seam's first column
        dem[16, 5:40] = -100.0        # and along a seam's first row
        dem[100:104, 20:30] = -100.0
        dem[128, 69] = np.nan         # not finite: a wall too
    valid = (dem > -100) & np.isfinite(dem)
    depth = np.zeros((H, W))
    depth[: max(1, H // 3), : max(1, W // 3)] = 0.8
    depth[~valid] = 0.0
    corners = [(15, 63), (16, 64), (min(H, 33) - 1, min(W, 129) - 1), (0, 0)]
    cells = sorted({cy * W + cx for cy, cx in corners if cy < H and cx < W and valid[cy, cx]})
    times = np.array([0.0, 40.0, 90.0, 500.0])
    q = np.array([[2.0 + j, 15.0, 6.0 + 2 * j, 0.0] for j in range(len(cells))])
    kw = {"depth": depth, "inflow": (np.array(cells, np.int64), times, q)}
    if variant == "scalars-closed":
        kw.update(manning=0.04, rain=30e-3 / 3600.0, boundary="closed")
    else:
        kw.update(manning=(0.02 + 0.05 * rng.random((H, W))), rain=(80e-3 / 3600.0) * rng.random((H, W)),
                  boundary="open", boundary_slope=2e-3, dry=5e-4, alpha=0.6, arrival_depth=0.1)
    return dem, valid, kw


SHAPES = [(1, 1), (1, 200), (200, 1), (64, 64), (63, 65), (65, 129), (129, 70)]


@pytest.mark.parametrize("variant", ["scalars-closed", "rasters-open"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_parity_with_the_reference(shape, variant):
    dem, valid, kw = _case(shape, variant)
    ref = _ref(dem, valid, 10.0, 240.0, **kw)
    got = _run(dem, 10.0, 240.0, **kw)
    print("steps %d, hmax %.3f, limited steps %d, wet cells %d" % (ref["steps"], ref["hmax"], ref["limited_steps"],
                                                                  (ref["depth"] > 0).sum()))
    assert 20 <= ref["steps"] <= 1000 and ref["finished"]
    _same(got, ref, valid)


def test_parity_hunter_wave():
    inflow, ana = R.hunter()
    dem = np.zeros((1, 200), np.float32)
    valid = np.ones((1, 200), bool)
    ref = _ref(dem, valid, 25.0, 3600.0, manning=0.03, inflow=inflow)
    got = _run(dem, 25.0, 3600.0, manning=0.03, inflow=inflow)
    _same(got, ref, valid, 25.0)
    rmse = float(np.sqrt(np.mean((got.depth[0] - ana) ** 2)))
    print("steps %d, RMSE %.5f m" % (ref["steps"], rmse))
    assert rmse <= 1.5 * 0.03563 and rmse <= 0.05 * 2.38


# ---- 2. the host-test cases on the device ---------------------------------------------------------------------------
@pytest.mark.parametrize("level,islands", [(5.0, False), (2.0, True)])
def test_lake_at_rest(level, islands):
    dem, valid, depth = R.lake(level, islands)
    got = _run(dem, 10.0, 600.0, depth=depth)
    assert got.info["finished"] and got.info["t"] == 600.0 and got.info["steps"] > 100
    assert np.array_equal(_bits(got.state["depth"]), _bits(depth))
    assert not got.state["qx"].any() and not got.state["qy"].any()
    assert np.array_equal(_bits(got.max_depth), _bits(np.where(valid, depth, -100.0)))
    assert got.info["limited_steps"] == 0


def test_conservation_rain_and_inflow():
    dem, valid = R.rough_terrain()
    cell = 35 * dem.shape[1] + 3
    rain = 50e-3 / 3600.0
    kw = dict(rain=rain, inflow=(np.array([cell]), np.array([0.0]), np.array([[20.0]])))
    got = _run(dem, 10.0, 1800.0, **kw)
    v_in = (rain * valid.sum() * 100.0 + 20.0) * 1800.0
    print("steps %d, volume %.6f of %.6f" % (got.info["steps"], got.info["volume"], v_in))
    h = got.state["depth"]
    assert not np.isnan(h).any() and h.min() >= 0 and (got.depth[~valid] == -100).all()
    assert abs(got.info["volume"] - v_in) <= 1e-9 * v_in
    _same(got, _ref(dem, valid, 10.0, 1800.0, **kw), valid)


def test_conservation_dam_break():
    dem, valid, depth = R.dam_break()
    got = _run(dem, 10.0, 900.0, manning=0.01, depth=depth)
    v_in = math.fsum((depth * 100.0).reshape(-1).tolist())
    print("steps %d, volume %.6f of %.6f" % (got.info["steps"], got.info["volume"], v_in))
    h = got.state["depth"]
    assert not np.isnan(h).any() and h.min() >= 0
    assert abs(got.info["volume"] - v_in) <= 1e-9 * v_in
    _same(got, _ref(dem, valid, 10.0, 900.0, manning=0.01, depth=depth), valid)


def test_open_boundary_decay():
    dem, valid, depth = R.dam_break()
    v = [math.fsum((depth * 100.0).reshape(-1).tolist())]
    state = None
    for t_end in (300.0, 600.0, 1200.0, 2400.0, 3600.0):
        got = _run(dem, 10.0, t_end, manning=0.01, depth=depth, boundary="open", state=state)
        state = got.state
        v.append(got.info["volume"])
        assert got.state["depth"].min() >= 0 and got.info["t"] == t_end
    print("volumes %s" % v)
    assert (np.diff(v) <= 0).all() and v[1] < v[0]  # (what lies below the dry depth stays)
    assert v[-1] < 0.05 * v[0]
    # the legs end where the uncut run has no step boundary, so the uncut run is what is held to the reference
    whole = _run(dem, 10.0, 3600.0, manning=0.01, depth=depth, boundary="open")
    _same(whole, _ref(dem, valid, 10.0, 3600.0, manning=0.01, depth=depth, boundary="open"), valid)
    assert whole.info["volume"] < 0.05 * v[0]


# ---- 3. tiers and batching --------------------------------------------------------------------------------------------
def _dev(ctx, dem, valid, px, t_end, kw, max_steps):
    """dt_dev_inundation on resident rasters -> (depth, qx, qy, max_depth, arrival, info)"""
    from descriptools_amd import _lib
    H, W = dem.shape
    z = np.where(valid, dem, np.nan).astype(np.float32)
    h0 = np.ascontiguousarray(kw["depth"], np.float64)
    cells, times, q = kw["inflow"]
    par = np.array([px, 0.0, t_end, kw["manning"], kw["rain"], kw.get("alpha", 0.7), 60.0, kw.get("dry", 1e-3),
                    kw.get("boundary_slope", 1e-3), kw.get("arrival_depth", 0.05)], np.float64)
    arrays = [ctx.to_device(z), ctx.to_device(np.ascontiguousarray(cells, np.int64)),
              ctx.to_device(np.ascontiguousarray(times, np.float64)), ctx.to_device(np.ascontiguousarray(q, np.float64)),
              ctx.to_device(h0), ctx.to_device(np.zeros((H, W))), ctx.to_device(np.zeros((H, W))),
              ctx.to_device(h0.copy()), ctx.to_device(np.where(valid & (h0 > par[9]), 0.0, np.nan)),
              ctx.empty((8,), np.int64)]
    d_z, d_c, d_t, d_q, d_h, d_qx, d_qy, d_md, d_ar, d_i = arrays
    try:
        _lib.check(_lib.lib().dt_dev_inundation(ctx.h, d_z.ptr, None, None, H, W, _lib.ptr(par, _lib.c_f64p),
                                                1 if kw["boundary"] == "open" else 0, d_c.ptr, d_t.ptr, d_q.ptr,
                                                len(cells), len(times), 0, max_steps, d_h.ptr, d_qx.ptr, d_qy.ptr,
                                                d_md.ptr, d_ar.ptr, d_i.ptr))
        return [a.to_host() for a in (d_h, d_qx, d_qy, d_md, d_ar, d_i)]
    finally:
        for a in arrays:
            a.free()


def test_tiers_batching_repeat_and_resume():
    from descriptools_amd.device import Context
    dem, valid, kw = _case((65, 129), "scalars-closed")
    kw["boundary"] = "open"
    first = _run(dem, 10.0, 200.0, **kw)
    steps = first.info["steps"]
    assert first.info["finished"] and 20 <= steps <= 1000
    names = ("depth", "qx", "qy", "max_depth", "arrival")
    for sync_every in (1, 7, 1024, 64):  # 64 again: a second run
        again = _run(dem, 10.0, 200.0, sync_every=sync_every, **kw)
        assert again.info == first.info
        for name in names:
            assert np.array_equal(_bits(again.state[name]), _bits(first.state[name])), (name, sync_every)
    # a run cut at an odd and at an even number of steps (the state then sits in either copy), and gone on with
    for cut in (steps // 2 | 1, steps // 3 & ~1):
        part = _run(dem, 10.0, 200.0, max_steps=cut, **kw)
        assert part.info["steps"] == cut and not part.info["finished"] and part.info["t"] < 200.0
        rest = _run(dem, 10.0, 200.0, state=part.state, **{k: v for k, v in kw.items() if k != "depth"})
        assert rest.info["steps"] == steps and rest.info["t"] == first.info["t"] and rest.info["finished"]
        for name in names:
            assert np.array_equal(_bits(rest.state[name]), _bits(first.state[name])), (name, cut)
    ctx = Context()
    try:
        for extra in (0, 5):  # exactly the steps the run needs (odd or even), and guarded steps beyond the end
            h, qx, qy, md, ar, info = _dev(ctx, dem, valid, 10.0, 200.0, kw, steps + extra)
            assert info[0] == steps and info[1] == steps and info[7] == 1
            assert info[2:3].view(np.float64)[0] == 200.0
            for name, a in zip(names, (h, qx, qy, md, ar)):
                assert np.array_equal(_bits(a), _bits(first.state[name])), (name, extra)
        h, qx, qy, md, ar, info = _dev(ctx, dem, valid, 10.0, 200.0, kw, 9)
        part = _run(dem, 10.0, 200.0, max_steps=9, **kw)
        assert info[0] == 9 and info[7] == 0 and np.array_equal(_bits(h), _bits(part.state["depth"]))
        assert ctx.status() == 0
    finally:
        ctx.close()


# ---- 4. ends and refusals ---------------------------------------------------------------------------------------------
def test_ends():
    dem, valid, kw = _case((63, 65), "scalars-closed")
    got = _run(dem, 10.0, 77.7, **kw)
    assert got.info["t"] == 77.7 and got.info["finished"] and got.state["t"] == 77.7
    got = _run(dem, 10.0, 1e6, max_steps=5, **kw)
    assert got.info["steps"] == 5 and not got.info["finished"] and 0 < got.info["t"] < 1e6
    got = _run(dem, 10.0, 100.0, max_steps=0, **kw)
    assert got.info["steps"] == 0 and got.info["t"] == 0.0 and not got.info["finished"]
    assert np.array_equal(_bits(got.state["depth"]), _bits(kw["depth"]))
    assert got.info["hmax"] == 0.8


def test_all_nodata_and_empty():
    from descriptools_amd import inundation
    dem = np.full((20, 70), -100.0, np.float32)
    got = inundation.simulate(dem, 10.0, 600.0, rain=1e-5, outputs=ALL)
    assert got.info["finished"] and got.info["t"] == 600.0 and got.info["steps"] == 10 and got.info["volume"] == 0.0
    assert (got.depth == -100).all() and (got.max_depth == -100).all() and np.isnan(got.arrival).all()
    assert not got.state["qx"].any() and not got.state["depth"].any()
    for shape in ((0, 7), (5, 0)):
        got = inundation.simulate(np.zeros(shape, np.float32), 10.0, 600.0, outputs=ALL)
        assert got.depth.shape == shape and got.arrival.shape == shape
        assert got.info["finished"] and got.info["steps"] == 0 and got.info["volume"] == 0.0


def test_entry_refusals():
    """both entries refuse, before they touch a raster: the shape, each scalar, the inflow's sizes, NULL rasters"""
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    L = _lib.lib()
    good = [10.0, 0.0, 60.0, 0.05, 0.0, 0.7, 60.0, 1e-3, 1e-3, 0.05]

    def par(i=None, v=None):
        p = np.array(good, np.float64)
        if i is not None:
            p[i] = v
        return p

    cases = [((4, 4), par(0, 0.0), 0, 0, 0, b"px"), ((4, 4), par(0, float("nan")), 0, 0, 0, b"px"),
             ((-1, 4), par(), 0, 0, 0, b"shape"), ((65536, 32768), par(), 0, 0, 0, b"2^31"),
             ((4, 4), par(1, -1.0), 0, 0, 0, b"t0"), ((4, 4), par(2, 0.0), 0, 0, 0, b"t_end"),
             ((4, 4), par(2, float("inf")), 0, 0, 0, b"t_end"), ((4, 4), par(3, 0.0), 0, 0, 0, b"manning"),
             ((4, 4), par(4, -1e-9), 0, 0, 0, b"rain"), ((4, 4), par(5, 1.5), 0, 0, 0, b"alpha"),
             ((4, 4), par(5, 0.0), 0, 0, 0, b"alpha"), ((4, 4), par(6, 0.0), 0, 0, 0, b"dt_max"),
             ((4, 4), par(7, -1.0), 0, 0, 0, b"dry"), ((4, 4), par(8, 0.0), 0, 0, 0, b"boundary_slope"),
             ((4, 4), par(9, float("nan")), 0, 0, 0, b"arrival_depth"), ((4, 4), par(), 2, 0, 0, b"boundary"),
             ((4, 4), par(), 0, 4097, 1, b"inflow cells"), ((4, 4), par(), 0, 1, 0, b"inflow times"),
             ((4, 4), par(), 0, 0, 0, b"NULL raster")]
    info = np.zeros(8, np.int64)
    pi = _lib.ptr(info, _lib.c_i64p)
    ctx = Context()
    try:
        for (H, W), p, boundary, K, T, word in cases:
            pp = _lib.ptr(p, _lib.c_f64p)
            assert L.dt_inundation(None, None, None, H, W, pp, boundary, None, None, None, K, T, 0, -1, 64, None, None,
                                   None, None, None, pi) == -1, word
            assert word in L.dt_last_error(), (word, L.dt_last_error())
            assert L.dt_dev_inundation(ctx.h, None, None, None, H, W, pp, boundary, None, None, None, K, T, 0, 8, None,
                                       None, None, None, None, None) == -1, word
            assert word in L.dt_last_error(), (word, L.dt_last_error())
        pp = _lib.ptr(par(), _lib.c_f64p)
        for sync_every, max_steps, word in ((0, -1, b"sync_every"), (1025, -1, b"sync_every"), (64, -2, b"max_steps")):
            assert L.dt_inundation(None, None, None, 4, 4, pp, 0, None, None, None, 0, 0, 0, max_steps, sync_every, None,
                                   None, None, None, None, pi) == -1
            assert word in L.dt_last_error()
        for max_steps in (-1, (1 << 20) + 1):
            assert L.dt_dev_inundation(ctx.h, None, None, None, 4, 4, pp, 0, None, None, None, 0, 0, 0, max_steps, None,
                                       None, None, None, None, None) == -1
            assert b"max_steps" in L.dt_last_error()
        assert L.dt_dev_inundation(None, None, None, None, 4, 4, None, 0, None, None, None, 0, 0, 0, 8, None, None,
                                   None, None, None, None) != 0, "a NULL context is refused first"
        info[:] = 7
        assert L.dt_inundation(None, None, None, 0, 9, pp, 0, None, None, None, 0, 0, 0, -1, 64, None, None, None, None,
                               None, pi) == 0 and not info.any()
        assert L.dt_dev_inundation(ctx.h, None, None, None, 0, 7, pp, 0, None, None, None, 0, 0, 0, 8, None, None, None,
                                   None, None, None) == 0
        assert ctx.status() == 0
    finally:
        ctx.close()
