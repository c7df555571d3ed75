"""GPU (-m gpu): drainage, basins, watersheds and upslope length (watershed.py, dt_drainage, dt_upslope_length and the
device tier; k_dr_* / k_ul_* in dt_watershed.hip) against the pure-numpy reference (tests/_watershed_ref.py), bit for
bit: hand-built cases, a serpentine path of more than 2^20 moves across many tiles, random fields with planted
cycles and pour points, nodata blobs and non-finite DEMs, degenerate shapes, 4096^2 synthetic terrain (raw and
conditioned D8) and the bundled Example.  Cross-checks: basin sizes, upslope length at outlets, flow_hand_index, the
device tier on a Chain's fdr, NULL outputs and repeated runs."""
import numpy as np
import pytest

import oracle
from conftest import load_example

import _watershed_ref as R

pytestmark = pytest.mark.gpu


def _same(name, g, r):
    assert g.dtype == r.dtype, name
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        i = tuple(bad[0])
        raise AssertionError("%s: %d cells differ, first at %s: got %r, reference %r" % (name, len(bad), i, g[i], r[i]))


def check(fdr, px=1.0, dem=None, pour=None, upslope=True):
    """every output of every entry point against the reference; returns (target, length, label, upslope)"""
    from descriptools_amd import watershed as ws
    t, l, lb = R.drainage(fdr, px, dem, pour)
    got = ws.drainage(fdr, px, dem, pour)
    _same("target", got.target, t)
    _same("length", got.length, l)
    if pour is None:
        _same("basins", ws.basins(fdr, dem), t)
    else:
        _same("watersheds", ws.watersheds(fdr, pour, dem), lb)
    u = None
    if upslope:
        u = R.upslope_length(fdr, px, dem)
        _same("upslope", ws.upslope_length(fdr, px, dem), u)
    return t, l, lb, u


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_hand_built(name):
    fdr, dem, pour, px, tg, ln, lb, up = R.hand_cases()[name]
    t, l, b, u = check(fdr, px, dem, pour)
    np.testing.assert_array_equal(t, tg)
    np.testing.assert_array_equal(l, np.asarray(ln, np.float64))
    if lb is not None:
        np.testing.assert_array_equal(b, lb)
    np.testing.assert_array_equal(u, np.asarray(up, np.float64))


def _serpentine(H, W):
    fdr = np.zeros((H, W), np.uint8)
    fdr[0::2, :] = R.E
    fdr[1::2, :] = R.W_
    fdr[0::2, -1] = R.S
    fdr[1::2, 0] = R.S
    fdr[-1, -1 if H % 2 else 0] = 0
    return fdr


def test_serpentine_over_2_20_moves():
    """one path through every cell of 1025 x 1024 (1,049,599 moves, 17 x 16 tiles): exact counts, no move cap"""
    from descriptools_amd import watershed as ws
    H, W = 1025, 1024
    fdr = _serpentine(H, W)
    order = np.arange(H * W).reshape(H, W)
    order[1::2] = order[1::2, ::-1]
    M = H * W - 1
    px = 3.0
    tgt = H * W - 1 if H % 2 else (H - 1) * W
    dr = ws.drainage(fdr, px)
    assert (dr.target == tgt).all()
    np.testing.assert_array_equal(dr.length, (M - order).astype(np.float64) * px)
    np.testing.assert_array_equal(ws.upslope_length(fdr, px), order.astype(np.float64) * px)
    t, l, _ = R.drainage(fdr, px)
    _same("target", dr.target, t)
    _same("length", dr.length, l)
    # pour points every 100,000 cells along the path
    pour = np.zeros((H, W), np.int64)
    for k, i in enumerate(range(50000, H * W, 100000)):
        pour.reshape(-1)[np.flatnonzero(order.reshape(-1) == i)] = k + 1
    check(fdr, px, None, pour, upslope=False)


def _field(H, W, seed, cycles, nodata=False):
    rng = np.random.default_rng(seed)
    fdr = rng.choice(np.array([R.SW, R.S, R.SE, R.E], np.uint8), size=(H, W))
    fdr[rng.random((H, W)) < 0.002] = rng.choice(np.array([0, 3, 255], np.uint8))
    noisy = rng.random((H, W)) < 0.05
    fdr[noisy] = rng.choice(np.array([1, 2, 4, 8, 16, 32, 64, 128], np.uint8), size=int(noisy.sum()))
    for _ in range(cycles):
        y, x = int(rng.integers(0, H - 1)), int(rng.integers(0, W - 1))
        fdr[y, x], fdr[y, x + 1], fdr[y + 1, x + 1], fdr[y + 1, x] = R.E, R.S, R.W_, R.N
    # a long cycle across tiles
    y0, x0 = H // 3, W // 4
    fdr[y0, x0:x0 + 150] = R.E
    fdr[y0:y0 + 90, x0 + 150] = R.S
    fdr[y0 + 90, x0 + 1:x0 + 151] = R.W_
    fdr[y0 + 1:y0 + 91, x0] = R.N
    dem = None
    if nodata:
        dem = rng.random((H, W)).astype(np.float32) * 50
        yy, xx = np.mgrid[0:H, 0:W]
        for _ in range(6):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(5, 40)
            dem[(yy - cy) ** 2 + (xx - cx) ** 2 < r * r] = -100
        dem[rng.random((H, W)) < 0.01] = -150
    return fdr, dem


@pytest.mark.parametrize("W", [1024, 1000])
def test_random_fields_with_cycles(W):
    fdr, _ = _field(600, W, W, cycles=60)
    t, l, _, u = check(fdr, 2.5)
    assert (t == -100).any() and (u == -100).any() and (u > 100).any()


@pytest.mark.parametrize("W", [1024, 777])
def test_random_fields_with_pour_points_and_nodata(W):
    fdr, dem = _field(520, W, 3 * W, cycles=30, nodata=True)
    rng = np.random.default_rng(W)
    pour = np.where(rng.random(fdr.shape) < 0.002, rng.integers(1, 1 << 40, fdr.shape), 0).astype(np.int64)
    pour[dem == -100] = 77                               # on nodata: ignored
    cyc = np.argwhere(fdr == R.N)[0]
    pour[cyc[0], cyc[1]] = 5                             # on a cycle
    t, l, lb, _ = check(fdr, 1.0, dem, pour)
    assert (lb == 0).any() and (lb == -100).any() and (lb > 0).any()
    check(fdr, 1.0, dem, None)


def test_non_finite_dem():
    """the accumulate mask rule: dem <= -100 is nodata in the DEM's dtype; NaN and +inf are not, -inf is"""
    fdr, _ = _field(200, 300, 9, cycles=5)
    rng = np.random.default_rng(9)
    dem = rng.random(fdr.shape) * 10
    dem[rng.random(fdr.shape) < 0.05] = np.nan
    dem[rng.random(fdr.shape) < 0.03] = np.inf
    dem[rng.random(fdr.shape) < 0.03] = -np.inf
    dem[rng.random(fdr.shape) < 0.03] = -1e30
    dem[rng.random(fdr.shape) < 0.03] = -100.0
    dem[rng.random(fdr.shape) < 0.03] = -99.9999999
    check(fdr, 1.0, dem)
    check(fdr, 1.0, dem.astype(np.float32))


@pytest.mark.parametrize("shape", [(1, 1), (1, 5000), (5000, 1), (130, 67), (65, 129), (0, 0), (0, 9), (9, 0)])
def test_degenerate_shapes(shape):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    fdr = rng.choice(np.array([R.E, R.W_, R.S, R.N, R.SE, 0], np.uint8), size=shape)
    if shape[0] == 1:
        fdr[:] = R.E
    if shape[1] == 1:
        fdr[:] = R.S
    pour = (rng.random(shape) < 0.01).astype(np.int64) * 3
    check(fdr, 1.0)
    check(fdr, 1.0, None, pour, upslope=False)


def _basin_cross_checks(fdr, t, l, u, dem=None):
    valid = np.ones(fdr.shape, bool) if dem is None else ~(np.asarray(dem) <= -100)
    ok = t >= 0
    sizes = np.bincount(t[ok], minlength=fdr.size)
    assert sizes.sum() + int((valid & ~ok).sum()) == int(valid.sum())
    # upslope length at each outlet = the largest length in its basin
    mx = np.full(fdr.size, -np.inf)
    np.maximum.at(mx, t[ok], l[ok])
    outs = np.flatnonzero(sizes)
    np.testing.assert_array_equal(u.reshape(-1)[outs], mx[outs])


@pytest.mark.parametrize("conditioned", [False, True])
def test_synthetic_4096(conditioned):
    from descriptools_amd import flowdir
    n = 4096
    dem = oracle.synth_dem(5, n, n)
    fdr = flowdir.d8_conditioned(dem, 10.0) if conditioned else flowdir.d8(dem, 10.0)
    t, l, _, u = check(fdr, 10.0)
    _basin_cross_checks(fdr, t, l, u)
    assert u.max() > 1000.0


def test_example():
    """the bundled Example's GIS D8 raster, with its nodata"""
    dem, fdr, fac, _, _, _ = load_example()
    t, l, _, u = check(fdr, 30.0, dem)
    _basin_cross_checks(fdr, t, l, u, dem)
    pour = np.where(fac > 128000, 1 + np.arange(fac.size).reshape(fac.shape) % 1000, 0).astype(np.int64)
    check(fdr, 30.0, dem, pour, upslope=False)


def test_flow_hand_index_agrees():
    """with pour_points = river and no dem, wherever flow_hand_index gives an index, target equals it and
    float32(length) is within 1 ulp of its flow distance"""
    from descriptools_amd import flowacc, flowdir, flowhand, watershed as ws
    H, W = 700, 900
    dem = oracle.synth_dem(11, H, W)
    fdr = flowdir.d8(dem, 10.0)
    river = (flowacc.accumulate(fdr) > 500).astype(np.int8)
    fd, idx, _ = flowhand.flow_hand_index(dem, fdr, river, 10.0)
    dr = ws.drainage(fdr, 10.0, pour_points=river.astype(np.int64))
    m = idx >= 0
    assert m.sum() > 1000
    np.testing.assert_array_equal(dr.target[m], idx[m])
    l32 = dr.length[m].astype(np.float32)
    assert (np.abs(l32.view(np.int32).astype(np.int64) - fd[m].view(np.int32).astype(np.int64)) <= 1).all()


def test_device_tier_on_chain_fdr_and_null_outputs():
    """dt_dev_drainage / dt_dev_upslope_length on a Chain's own fdr equal the host tier; NULL outputs are left
    untouched; repeated runs are bit-identical"""
    from descriptools_amd import _lib, chain, device, watershed as ws
    H, W = 512, 640
    dem = oracle.synth_dem(7, H, W)
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=10.0, overlap=False, tune_placement=False, river_threshold=200)
    d = ctx.to_device(np.ascontiguousarray(dem, np.float32))
    pour = ((np.arange(H * W).reshape(H, W) % 997) == 0).astype(np.int64) * 4
    p_d = ctx.to_device(pour)
    tg_d = ctx.empty((H, W), np.int64)
    ln_d = ctx.to_device(np.full((H, W), 12345.0))
    lb_d = ctx.to_device(np.full((H, W), -777, np.int64))
    up_d = ctx.empty((H, W), np.float64)
    L = _lib.lib()
    try:
        ch.run(d.ptr)
        runs = []
        for _ in range(3):
            _lib.check(L.dt_dev_drainage(ctx.h, ch.p("fdr"), None, None, H, W, 10.0, tg_d.ptr, None, None))
            _lib.check(L.dt_dev_upslope_length(ctx.h, ch.p("fdr"), None, H, W, 10.0, up_d.ptr))
            ctx.sync()
            runs.append((tg_d.to_host(), up_d.to_host()))
        assert (ln_d.to_host() == 12345.0).all() and (lb_d.to_host() == -777).all()
        _lib.check(L.dt_dev_drainage(ctx.h, ch.p("fdr"), None, p_d.ptr, H, W, 10.0, None, None, lb_d.ptr))
        ctx.sync()
        lab = lb_d.to_host()
        assert (ln_d.to_host() == 12345.0).all()
        fdr = ch.buf["fdr"].to_host()
        # label requires pour; px must be finite and > 0
        assert L.dt_dev_drainage(ctx.h, ch.p("fdr"), None, None, H, W, 10.0, None, None, lb_d.ptr) != 0
        assert L.dt_dev_drainage(ctx.h, ch.p("fdr"), None, None, H, W, 0.0, tg_d.ptr, None, None) != 0
        assert L.dt_dev_upslope_length(ctx.h, ch.p("fdr"), None, H, W, float("nan"), up_d.ptr) != 0
        assert L.dt_dev_drainage(ctx.h, None, None, None, 0, 0, 1.0, None, None, None) == 0
    finally:
        for b in (d, p_d, tg_d, ln_d, lb_d, up_d):
            b.free()
        ch.free()
        ctx.close()
    for r in runs[1:]:
        np.testing.assert_array_equal(r[0], runs[0][0])
        np.testing.assert_array_equal(r[1], runs[0][1])
    np.testing.assert_array_equal(runs[0][0], ws.basins(fdr))
    np.testing.assert_array_equal(runs[0][1], ws.upslope_length(fdr, 10.0))
    np.testing.assert_array_equal(lab, ws.watersheds(fdr, pour))
    t, l, _ = R.drainage(fdr, 10.0)
    np.testing.assert_array_equal(runs[0][0], t)
    np.testing.assert_array_equal(runs[0][1], R.upslope_length(fdr, 10.0))


def test_one_graph_for_every_path_operator():
    """drainage, the downstream extreme and the downstream sum stop on the same graph (dt_path_tiles.h's pt_classify):
    with pour = stop, the cells with a target, with a `where` and with a sum are one set, on the host tier and on the
    device tier, and `where` of the raster that is 1 on the stop cells is the target.  130 x 67 is 3 x 2 tiles, both
    edges partial; the field has diagonal moves, in-tile cycles, a ring of 200 cells through four tiles (planted again
    over the nodata, so it crosses a tile border in both directions), nodata, codes that point out of the raster, stops
    on nodata (ignored) and a stop on the ring."""
    import _pathsum_ref as PR
    from descriptools_amd import _lib, device, flowpath as fp, watershed as ws
    H, W = 130, 67
    fdr, dem = PR.field(H, W, 24, cycles=6, nodata=True, ring=(50, 50))
    y0, x0 = H // 3, W // 4
    ring = np.zeros((H, W), bool)
    ring[y0, x0:x0 + 50], fdr[y0, x0:x0 + 50] = True, R.E
    ring[y0:y0 + 50, x0 + 50], fdr[y0:y0 + 50, x0 + 50] = True, R.S
    ring[y0 + 50, x0 + 1:x0 + 51], fdr[y0 + 50, x0 + 1:x0 + 51] = True, R.W_
    ring[y0 + 1:y0 + 51, x0], fdr[y0 + 1:y0 + 51, x0] = True, R.N
    dem[ring] = 1.0
    nod = dem <= -100
    on_cycle = (R.upslope_length(fdr, 1.0, dem) == -100) & ~nod
    # the whole ring is a cycle of valid cells through four tiles, and there are cycles beside it
    assert ring.sum() == 200 and on_cycle[ring].all() and (on_cycle & ~ring).sum() >= 4
    assert {(y // 64, x // 64) for y, x in np.argwhere(ring)} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    rng = np.random.default_rng(1024)
    stop = (rng.random((H, W)) < 0.01).astype(np.uint8)
    on_nodata = np.argwhere(nod)[::50]
    stop[on_nodata[:, 0], on_nodata[:, 1]] = 1
    stop[ring] = 0
    stop[y0, 20] = 1  # the one stop on the ring
    assert len(on_nodata) > 10
    pour = stop.astype(np.int64)
    values = stop.astype(np.float32)
    weights = rng.random((H, W))

    def same_set(target, where, total):
        has = target >= 0
        np.testing.assert_array_equal(where >= 0, has)
        np.testing.assert_array_equal(total != -100, has)
        assert has.any() and not has.all()
        np.testing.assert_array_equal(where[has], target[has])
        assert has[ring].all() and not has[nod].any()

    same_set(ws.drainage(fdr, 1.0, dem, pour).target,
             fp.downstream_extreme(fdr, values, "max", dem, stop, where=True).where,
             fp.downstream_sum(fdr, weights, dem, stop))

    ctx = device.Context()
    L = _lib.lib()
    ins = [ctx.to_device(a) for a in (fdr, _lib.nodata_mask(dem, fdr.shape), pour, stop, values, weights)]
    f_d, d_d, p_d, s_d, v_d, w_d = (a.ptr for a in ins)
    tg_d, wh_d, sum_d = ctx.empty((H, W), np.int64), ctx.empty((H, W), np.int64), ctx.empty((H, W), np.float64)
    try:
        _lib.check(L.dt_dev_drainage(ctx.h, f_d, d_d, p_d, H, W, 1.0, tg_d.ptr, None, None))
        _lib.check(L.dt_dev_flowpath_downstream(ctx.h, f_d, d_d, v_d, s_d, H, W, 0, None, wh_d.ptr))
        _lib.check(L.dt_dev_flowpath_downstream_sum(ctx.h, f_d, d_d, w_d, s_d, H, W, fp.path_frac_bits(weights),
                                                    sum_d.ptr))
        ctx.sync()
        same_set(tg_d.to_host(), wh_d.to_host(), sum_d.to_host())
    finally:
        for a in ins + [tg_d, wh_d, sum_d]:
            a.free()
        ctx.close()
