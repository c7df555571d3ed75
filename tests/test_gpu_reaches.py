"""GPU (-m gpu): reach catchments, channels, stage tables and inundation (reaches.py, dt_reach_*, dt_inundate and the
device tier; k_rc_* in dt_reaches.hip) against the pure-numpy reference (tests/_reaches_ref.py), bit for bit and for
every cell and table entry: hand-built cases, degenerate shapes, no network, the bundled Example, 4096^2 synthetic
terrain at a sparse and a dense threshold, catchment / HAND rasters made to stress the table kernel (one word for the
whole raster, white-noise reach ids, NaN / inf / -100 / negative heights and heights equal to stages, K = 1, 84, 1024,
non-uniform stages, float32 / float64 / int16 HAND, with and without slope, a capped and an absent LDS table), the
status bits, the device tier on a Chain's own rasters, repeated runs, and the volume cross-check against inundate."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import load_example

import _reaches_ref as R

pytestmark = pytest.mark.gpu

DT_STATUS_BAD_WEIGHT = 4
DT_STATUS_REACH_RANGE = 8
DT_DBG_RC_SLOTS = 10
FEET = 0.3048


def _same(name, g, r):
    g, r = np.asarray(g), np.asarray(r)
    assert g.dtype == r.dtype, "%s: dtype %s, reference %s" % (name, g.dtype, r.dtype)
    assert g.shape == r.shape, "%s: shape %s, reference %s" % (name, g.shape, r.shape)
    if g.tobytes() != r.tobytes():
        bad = np.argwhere(~((g == r) | ((g != g) & (r != r))))
        i = tuple(bad[0]) if len(bad) else None
        raise AssertionError("%s: %d entries differ, first at %s: got %r, reference %r"
                             % (name, len(bad), i, g[i] if i else None, r[i] if i else None))


def check_tables(cat, hand, px, stages, nr, slope=None, frac_bits=None):
    """hydraulic_tables against the reference, every entry; returns (tables, reference cells)"""
    from descriptools_amd import reaches
    t = reaches.hydraulic_tables(cat, hand, px, stages, nr, slope=slope, frac_bits=frac_bits)
    s = t.frac_bits
    if frac_bits is None and cat.size:
        assert s == R.default_frac_bits(cat.size, stages, slope)
    cells, hq, bq, took = R.tables(cat, hand, stages, nr, s, slope)
    area, vol, bed = R.derive(stages, cells, hq, bq, px, s)
    _same("cells", t.cells, cells)
    _same("area", t.area, area)
    _same("volume", t.volume, vol)
    _same("bed_area", t.bed_area, bed)
    if nr:
        assert int(t.cells[:, -1].sum()) == took
    return t, took


def check_inundation(cat, hand, px, t, k):
    """inundate with every reach at stages[k] against the reference, and against the tables' volume"""
    from descriptools_amd import reaches
    nr = t.cells.shape[0]
    stage = np.full(nr, t.stages[k])
    d = reaches.inundate(cat, hand, stage)
    _same("depth", d, R.inundate(cat, hand, stage))
    h = R.heights(hand).astype(np.float64)
    wet = d > 0
    assert (h[wet] < t.stages[k]).all()
    vol = np.bincount(cat[wet].astype(np.int64), weights=d[wet].astype(np.float64), minlength=nr) * (px * px)
    bound = t.cells[:, k] * (t.stages[k] * 2.0 ** -24 + 2.0 ** -(t.frac_bits + 1)) * (px * px)
    err = np.abs(vol - t.volume[:, k])
    worst = float((err / np.maximum(bound, 1e-300)).max()) if nr else 0.0
    print("volume cross-check: largest |sum(depth) px^2 - volume| / bound = %.3f" % worst)
    assert (err <= bound).all()
    return d


def check_network(fdr, river, dem, px, stages, slope=None, inundate_at=None):
    """every output of every entry point on a terrain case; returns the number of reaches"""
    from descriptools_amd import reaches
    link, idx, hand = R.network(dem, fdr, river)
    reach, cat, heads = R.catchments(link, idx)
    got = reaches.catchments(link, idx)
    _same("reach", got.reach, reach)
    _same("catchment", got.catchment, cat)
    _same("heads", got.heads, heads)
    nr = heads.size
    ch = reaches.channels(fdr, reach, px, nr)
    for name, g, r in zip(ch._fields, ch, R.channels(fdr, reach, px, nr)):
        _same(name, g, r)
    t, _ = check_tables(cat, hand, px, stages, nr, slope)
    if nr:
        check_inundation(cat, hand, px, t, len(stages) // 2 if inundate_at is None else inundate_at)
    else:
        _same("depth", reaches.inundate(cat, hand, np.zeros(0)), R.inundate(cat, hand, np.zeros(0)))
    return nr


@pytest.mark.parametrize("name", sorted(R.hand_cases()))
def test_hand_built(name):
    from descriptools_amd import reaches
    c = R.hand_cases()[name]
    got = reaches.catchments(c["link"], c["idx"])
    _same("reach", got.reach, c["reach"])
    _same("catchment", got.catchment, c["catch"])
    _same("heads", got.heads, c["heads"])
    nr = len(c["heads"])
    ch = reaches.channels(c["fdr"], got.reach, c["px"], nr)
    for k in ch._fields:
        _same(k, getattr(ch, k), c[k])
    t = reaches.hydraulic_tables(got.catchment, c["hand"], c["px"], c["stages"], nr, slope=c["slope"],
                                 frac_bits=c["s"])
    _same("cells", t.cells, c["cells"])
    _same("area", t.area, c["area"])
    _same("volume", t.volume, c["volume"])
    _same("bed_area", t.bed_area, c["bed_area"])
    _same("depth", reaches.inundate(got.catchment, c["hand"], c["stage"]), c["depth"])
    check_tables(c["catch"], c["hand"], c["px"], c["stages"], nr, c["slope"])   # the default frac_bits


@pytest.mark.parametrize("shape, thr", [((1, 1), 0), ((1, 3000), 5), ((3000, 1), 20), ((130, 67), 30),
                                        ((65, 129), 30), ((63, 1001), 100), ((257, 260), 100)])
def test_shapes(shape, thr):
    """1 x 1, one row, one column, sizes that are not multiples of the tile or of the 16-B vectors"""
    H, W = shape
    dem, slope, fdr, fac, river = R.terrain(H, W, 3 * H + W, thr)
    if shape == (1, 1):
        river[:] = 1
    nr = check_network(fdr, river, dem, 10.0, np.arange(1, 30) * 0.5, slope)
    assert nr > 0


def test_no_network():
    dem, slope, fdr, fac, river = R.terrain(200, 300, 5, 10 ** 9)
    assert check_network(fdr, river, dem, 10.0, np.array([1.0, 2.0]), slope) == 0


@pytest.mark.parametrize("thr, n_reaches", [(128000, 12), (2000, 475)])
def test_example(thr, n_reaches):
    """the bundled Example (an int16 DEM, so an int16 HAND) at the chain's threshold and at fac > 2000"""
    dem, fdr, fac, _, _, _ = load_example()
    river = (fac > thr).astype(np.int8)
    assert check_network(fdr, river, dem, 30.0, np.arange(84) * FEET) == n_reaches


@functools.lru_cache(maxsize=1)
def _terrain_4096():
    return R.terrain(4096, 4096, 5, 0)


@pytest.mark.parametrize("thr, with_slope", [(1000, False), (50, True)])
def test_synthetic_4096(thr, with_slope):
    """sparse and dense networks; the dense one has more reaches in a tile than the table has slots"""
    dem, slope, fdr, fac, _ = _terrain_4096()
    river = (fac > thr).astype(np.int8)
    nr = check_network(fdr, river, dem, 10.0, np.arange(84) * FEET, slope if with_slope else None)
    assert nr > (1000 if thr == 1000 else 50000)


def _noise_case(H, W, nr, K, dtype, with_slope, seed, uniform=True):
    """white-noise reach ids (negative ones too) with HAND full of special values"""
    rng = np.random.default_rng(seed)
    if K == 1:
        stages = np.array([2.5])
    elif uniform:
        stages = np.arange(K) * FEET
    else:
        stages = np.cumsum(rng.random(K) ** 3 + 1e-9) * (20.0 / K) + 0.25
    cat = rng.integers(0, nr, (H, W)).astype(np.int32)
    cat[rng.random((H, W)) < 0.05] = -100
    cat[rng.random((H, W)) < 0.01] = -1
    hand = (rng.random((H, W)) * stages[-1] * 1.1).astype(dtype)
    # heights equal to stages to the bit (as far as the dtype holds them), and just beside them
    eq = rng.random((H, W)) < 0.2
    hand[eq] = stages[rng.integers(0, K, int(eq.sum()))].astype(dtype)
    up = rng.random((H, W)) < 0.05
    hand[up] = np.nextafter(hand[up], dtype(np.inf))
    dn = rng.random((H, W)) < 0.05
    hand[dn] = np.nextafter(hand[dn], dtype(-np.inf))
    for v in (np.nan, np.inf, -np.inf, -100.0, -0.0, -1e-30, -5.0, 0.0):
        hand[rng.random((H, W)) < 0.01] = v
    slope = None
    if with_slope:
        slope = (rng.random((H, W)) ** 4 * 400).astype(np.float32)
        for v in (np.nan, np.inf, -np.inf, -3.0, 0.0):
            slope[rng.random((H, W)) < 0.01] = v
    return cat, hand, stages, slope


@pytest.mark.parametrize("K, dtype, with_slope, W", [
    (1, np.float32, False, 900), (1, np.float64, True, 901),
    (84, np.float32, False, 900), (84, np.float32, True, 900), (84, np.float64, False, 902), (84, np.float64, True, 900),
    (1024, np.float32, True, 900), (1024, np.float64, False, 900),
    (37, np.float32, True, 900), (37, np.float64, False, 899),            # non-uniform stages
])
def test_special_heights_and_stage_counts(K, dtype, with_slope, W):
    cat, hand, stages, slope = _noise_case(700, W, 300, K, dtype, with_slope, 7 * K + W, uniform=K != 37)
    t, took = check_tables(cat, hand, 10.0, stages, 300, slope)
    assert took > 1000
    check_inundation(np.where(cat < 300, cat, -100), hand, 10.0, t, K // 2)


def test_white_noise_over_100000_reaches():
    """thousands of reaches per tile: nearly every cell takes the fall-through path, whatever the slot count"""
    from descriptools_amd import reaches
    nr = 100000
    cat, hand, stages, slope = _noise_case(1500, 2048, nr, 84, np.float32, True, 11)
    t, took = check_tables(cat, hand, 10.0, stages, nr, slope)
    check_tables(cat, hand.astype(np.float64), 10.0, stages, nr, None)
    rng = np.random.default_rng(1)
    stage = rng.random(nr) * 30
    stage[rng.random(nr) < 0.1] = np.nan
    stage[rng.random(nr) < 0.05] = np.inf
    stage[rng.random(nr) < 0.05] = -1.0
    _same("depth", reaches.inundate(cat, hand, stage), R.inundate(cat, hand, stage))
    _same("depth64", reaches.inundate(cat, hand.astype(np.float64), stage),
          R.inundate(cat, hand.astype(np.float64), stage))


def test_count_scan_with_two_groups():
    """The scan of the per-block head counts (dt_launch_count_scan) at the smallest raster that has two groups: a block
    covers 2048 cells and a group 2048 blocks, so 2049 x 2048 cells are 2049 blocks, the last one alone in group 1.
    Sparse heads, among them cell 0, the last cell of block 2047, the first cell of block 2048 and the raster's last
    cell; exact against numpy.  The third level -- one thread of k_so_gscan owning several groups -- needs more than
    2^30 cells and stays untested."""
    from descriptools_amd import reaches
    H, W = 2049, 2048
    N, blk = H * W, 2048
    rng = np.random.default_rng(7)
    want = np.unique(np.concatenate([[0, 2048 * blk - 1, 2048 * blk, N - 1], rng.integers(0, N, 3000)]))
    link = np.full(N, -100, np.int64)
    link[want] = want
    idx = link.copy()  # the heads drain to themselves, every other cell to no river cell
    body = want[:-1] + 1  # a second cell on some links, where the next cell is no head itself
    body = body[link[body] < 0]
    link[body] = body - 1
    heads = np.flatnonzero(link == np.arange(N))
    assert heads.size == want.size and heads[heads >= 2048 * blk].size >= 2
    rank = np.full(N, -100, np.int32)
    rank[heads] = np.arange(heads.size, dtype=np.int32)
    reach = np.where(link >= 0, rank[np.maximum(link, 0)], np.int32(-100)).astype(np.int32)
    cat = np.where(idx >= 0, reach[np.maximum(idx, 0)], np.int32(-100)).astype(np.int32)
    got = reaches.catchments(link.reshape(H, W), idx.reshape(H, W))
    _same("heads", got.heads, heads)
    _same("reach", got.reach, reach.reshape(H, W))
    _same("catchment", got.catchment, cat.reshape(H, W))


def test_every_cell_in_one_word():
    """2048^2 cells of one reach in one bin: all adds meet in one word and the count is exactly N"""
    n = 2048
    cat = np.zeros((n, n), np.int32)
    hand = np.full((n, n), 0.5, np.float32)
    t, took = check_tables(cat, hand, 1.0, np.array([1.0]), 1)
    assert took == n * n and t.cells[0, 0] == n * n
    t, _ = check_tables(cat, hand, 1.0, np.arange(84) * FEET, 1, slope=np.full((n, n), 100.0, np.float32))
    assert t.cells[0, 1] == 0 and t.cells[0, 2] == n * n


@pytest.mark.parametrize("slots", [1, 3, -1])
def test_capped_and_absent_lds_table(slots):
    """the same tables with the LDS table capped at a few slots and without it (every cell on the fall-through path)"""
    from descriptools_amd import _lib
    dem, slope, fdr, fac, river = R.terrain(600, 800, 9, 40)
    link, idx, hand = R.network(dem, fdr, river)
    _, cat, heads = R.catchments(link, idx)
    L = _lib.lib()
    _lib.check(L.dt_debug_set(DT_DBG_RC_SLOTS, slots))
    try:
        check_tables(cat, hand, 10.0, np.arange(84) * FEET, heads.size, slope)
        check_tables(cat, hand, 10.0, np.arange(1, 5) * 2.0, heads.size, None)
    finally:
        _lib.check(L.dt_debug_set(DT_DBG_RC_SLOTS, 0))


def test_status_bits():
    """a catchment id >= R raises DT_STATUS_REACH_RANGE and the cell is left out; a bed weight beyond the bound of a
    fine frac_bits raises DT_STATUS_BAD_WEIGHT; both are errors through the host tier"""
    from descriptools_amd import _lib, device, reaches
    H, W, nr, K = 100, 128, 5, 3
    rng = np.random.default_rng(2)
    cat = rng.integers(0, nr, (H, W)).astype(np.int32)
    hand = rng.random((H, W)).astype(np.float32)
    stages = np.array([0.25, 0.5, 1.0])
    s = R.default_frac_bits(H * W, stages)
    L = _lib.lib()
    ctx = device.Context()
    bufs = []

    def dev_tables(cat_h, slope_h):
        c_d, h_d = ctx.to_device(cat_h), ctx.to_device(hand)
        s_d = ctx.to_device(slope_h) if slope_h is not None else None
        out = [ctx.empty((nr, K), np.int64) for _ in range(3)]
        bufs.extend([c_d, h_d] + out + ([s_d] if s_d else []))
        ctx.status()
        _lib.check(L.dt_dev_reach_tables(ctx.h, c_d.ptr, h_d.ptr, 4, s_d.ptr if s_d else None, H, W,
                                         stages.ctypes.data_as(_lib.c_f64p), K, nr, s, out[0].ptr, out[1].ptr,
                                         out[2].ptr))
        st = ctx.status()
        return st, [o.to_host() for o in out]

    try:
        st, tabs = dev_tables(cat, None)
        assert st == 0
        ref = R.tables(cat, hand, stages, nr, s)
        for g, r in zip(tabs, ref[:3]):
            _same("table", g, r)
        over = cat.copy()
        over[3, 5] = nr
        over[70, 100] = 2 ** 31 - 1
        st, tabs = dev_tables(over, None)
        assert st == DT_STATUS_REACH_RANGE
        for g, r in zip(tabs, R.tables(over, hand, stages, nr, s)[:3]):   # the reference leaves them out too
            _same("table", g, r)
        assert ctx.status() == 0
        slope = np.zeros((H, W), np.float32)
        slope[40, 40] = 1e30
        st, _ = dev_tables(cat, slope)
        assert st == DT_STATUS_BAD_WEIGHT
        st, _ = dev_tables(cat, None)
        assert st == 0                                                     # the context stays usable
    finally:
        for b in bufs:
            b.free()
        ctx.close()
    out = [np.zeros((nr, K), np.int64) for _ in range(3)]
    args = lambda c, sl: (c.ctypes.data_as(_lib.c_i32p), hand.ctypes.data_as(C.c_void_p), 4,
                          sl.ctypes.data_as(_lib.c_f32p) if sl is not None else None, H, W,
                          stages.ctypes.data_as(_lib.c_f64p), K, nr, s) + tuple(o.ctypes.data_as(_lib.c_i64p) for o in out)
    assert L.dt_reach_tables(*args(cat, None)) == 0
    with pytest.raises(RuntimeError, match="bed weight"):
        _lib.check(L.dt_reach_tables(*args(cat, slope)))
    with pytest.raises(RuntimeError, match="number of reaches"):
        _lib.check(L.dt_reach_tables(*args(over, None)))
    with pytest.raises(RuntimeError, match="number of reaches"):
        reaches.hydraulic_tables(over, hand, 1.0, stages, nr)
    with pytest.raises(ValueError, match="too fine"):
        reaches.hydraulic_tables(cat, hand, 1.0, stages, nr, slope=slope, frac_bits=s)
    check_tables(cat, hand, 1.0, stages, nr)


def test_device_tier_on_a_chain():
    """the device tier on a Chain's own idx (int32) / hand / slope and dt_dev_stream_order's link equals the host tier
    on the same rasters copied back, and the reference; two runs give identical bytes"""
    from descriptools_amd import _lib, chain, device, reaches
    H, W, px = 1024, 1280, 10.0
    import oracle
    dem = oracle.synth_dem(7, H, W)
    stages = np.arange(84) * FEET
    K = stages.size
    ctx = device.Context()
    ch = chain.Chain(H, W, ctx=ctx, px=px, overlap=False, tune_placement=False, river_threshold=200)
    L = _lib.lib()
    cap = 1 << 16
    d = ctx.to_device(np.ascontiguousarray(dem, np.float32))
    so_d = ctx.empty((H, W), np.int8)
    lk_d = ctx.empty((H, W), np.int64)
    rc_d, ct_d = ctx.empty((H, W), np.int32), ctx.empty((H, W), np.int32)
    hd_d, n_d = ctx.empty(cap, np.int64), ctx.empty(1, np.int64)
    dp_d = ctx.empty((H, W), np.float32)
    bufs = [d, so_d, lk_d, rc_d, ct_d, hd_d, n_d, dp_d]
    runs = []
    try:
        ch.run(d.ptr)
        _lib.check(L.dt_dev_stream_order(ctx.h, ch.p("fdr"), ch.p("river"), H, W, so_d.ptr, None, lk_d.ptr))
        for _ in range(2):
            _lib.check(L.dt_dev_reach_catchments(ctx.h, lk_d.ptr, ch.p("idx"), 4, H, W, rc_d.ptr, ct_d.ptr, hd_d.ptr,
                                                 cap, n_d.ptr))
            nr = int(n_d.to_host()[0])
            assert 0 < nr <= cap
            s = R.default_frac_bits(H * W, stages, ch.buf["slope"].to_host())
            cha = [ctx.empty(nr, np.int64) for _ in range(5)]
            tab = [ctx.empty((nr, K), np.int64) for _ in range(3)]
            stage_d = ctx.to_device(np.full(nr, stages[40]))
            bufs.extend(cha + tab + [stage_d])
            _lib.check(L.dt_dev_reach_channels(ctx.h, ch.p("fdr"), rc_d.ptr, H, W, nr, *[a.ptr for a in cha]))
            _lib.check(L.dt_dev_reach_tables(ctx.h, ct_d.ptr, ch.p("hand"), 4, ch.p("slope"), H, W,
                                             stages.ctypes.data_as(_lib.c_f64p), K, nr, s, *[a.ptr for a in tab]))
            _lib.check(L.dt_dev_inundate(ctx.h, ct_d.ptr, ch.p("hand"), 4, stage_d.ptr, H, W, nr, dp_d.ptr))
            assert ctx.status() == 0
            runs.append([rc_d.to_host(), ct_d.to_host(), hd_d.to_host()[:nr]] + [a.to_host() for a in cha + tab]
                        + [dp_d.to_host()])
        # heads alone, into a capacity smaller than R: only the first entries are written
        few = ctx.to_device(np.full(8, -7, np.int64))
        bufs.append(few)
        _lib.check(L.dt_dev_reach_catchments(ctx.h, lk_d.ptr, None, 0, H, W, None, None, few.ptr, 5, None))
        ctx.sync()
        np.testing.assert_array_equal(few.to_host(), list(runs[0][2][:5]) + [-7] * 3)
        link, idx = lk_d.to_host(), ch.buf["idx"].to_host()
        hand, slope, fdr = ch.buf["hand"].to_host(), ch.buf["slope"].to_host(), ch.buf["fdr"].to_host()
    finally:
        for b in bufs:
            b.free()
        ch.free()
        ctx.close()
    for a, b in zip(runs[0], runs[1]):
        assert a.tobytes() == b.tobytes()
    reach, cat, heads, end, down, n_cells, n_card, n_diag, cells, hq, bq, depth = runs[0]
    got = reaches.catchments(link, idx)
    _same("reach", reach, got.reach)
    _same("catchment", cat, got.catchment)
    _same("heads", heads, got.heads)
    hc = reaches.channels(fdr, reach, px, nr)
    for name, g, r in zip(hc._fields, (end, down, n_cells, n_card, n_diag), hc):
        _same(name, g, r)
    t = reaches.hydraulic_tables(cat, hand, px, stages, nr, slope=slope)
    assert t.frac_bits == s
    dv = reaches.tables_from_sums(stages, cells, hq, bq, px, s)
    _same("cells", dv.cells, t.cells)
    _same("volume", dv.volume, t.volume)
    _same("bed_area", dv.bed_area, t.bed_area)
    _same("depth", depth, reaches.inundate(cat, hand, np.full(nr, stages[40])))
    # ... and the reference on the same rasters
    r_reach, r_cat, r_heads = R.catchments(link, idx)
    _same("reach", reach, r_reach)
    _same("catchment", cat, r_cat)
    _same("heads", heads, r_heads)
    for name, g, r in zip(hc._fields, (end, down, n_cells, n_card, n_diag), R.channels(fdr, reach, px, nr)):
        _same(name, g, r)
    rc, rh, rb, _ = R.tables(cat, hand, stages, nr, s, slope)
    _same("cells", cells, rc)
    _same("Hq", hq, rh)
    _same("Bq", bq, rb)
