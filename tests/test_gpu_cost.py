"""GPU (-m gpu): cost.cost_distance / cost_hand (dt_cost_distance, dt_dev_cost_distance, k_cost_* in dt_cost.hip)
against the heap Dijkstra of tests/_cost_ref.py: cost as int64 bit patterns, indices and backlink equal, on every cell.
Trivial shapes; ragged tiles (65 x 63: 2 x 1 tiles of 64 x 64; 130 x 257: 3 x 5 tiles, every colour and an interior
tile) with uniform, integer (exact ties: the scan-order rule) and exp(U(-20, 20)) friction, 25 % barriers of every kind,
connectivity 8 and 4, and a visit limit of 1 that forces a global round per sweep; a serpentine whose path winds through
135 tiles, which shows that the multi-round path ran; watershed.basins on the back-links as an independent kernel; the
device tier and its budget; the C entry with NULL outputs between guard bands; the absorption example; cost_hand."""
import ctypes as C
import functools

import numpy as np
import pytest

import _cost_ref as R

pytestmark = pytest.mark.gpu

PX = 12.3  # inexact in binary: every product is rounded
TILE = 64  # CD_T of csrc/dt_cost.hip
SEED = 7


def _same(name, g, r):
    g, r = np.asarray(g), np.asarray(r)
    assert g.dtype == r.dtype, "%s: dtype %s, reference %s" % (name, g.dtype, r.dtype)
    assert g.shape == r.shape, "%s: shape %s, reference %s" % (name, g.shape, r.shape)
    gb = g.view(np.int64) if g.dtype == np.float64 else g
    rb = r.view(np.int64) if r.dtype == np.float64 else r
    if not np.array_equal(gb, rb):
        bad = np.argwhere(gb != rb)
        i = tuple(bad[0])
        raise AssertionError("%s: %d cells differ, first at %s: got %r, reference %r" % (name, len(bad), i, g[i], r[i]))


@functools.lru_cache(maxsize=None)
def _random_ref(shape, kind, conn):
    """(friction, sources, reference) of a random case: computed once, shared, never written to"""
    f, s = R.random_case(shape, kind, SEED)
    ref = R.reference(f, s, PX, conn)
    for a in (f, s) + ref[:3]:
        a.setflags(write=False)
    return f, s, ref


@functools.lru_cache(maxsize=None)
def _serpentine_ref():
    f, s = R.serpentine()
    ref = R.reference(f, s, PX, 8)
    for a in (f, s) + ref[:3]:
        a.setflags(write=False)
    return f, s, ref


def check(f, s, conn=8, limit=0, px=PX, ref=None):
    from descriptools_amd import cost
    got = cost.cost_distance(f, s, px, connectivity=conn, backlink=True, _visit_limit=limit)
    c, i, b, linkless, reached = ref if ref is not None else R.reference(f, s, px, conn)
    assert linkless == 0
    _same("cost", got.cost, c)
    _same("backlink", got.backlink, b)
    _same("indices", got.indices, i)
    assert got.info["reached"] == reached
    plain = cost.cost_distance(f, s, px, connectivity=conn, _visit_limit=limit)
    assert plain.backlink is None
    _same("cost without backlink", plain.cost, c)
    _same("indices without backlink", plain.indices, i)
    return got


# ---- trivial shapes -------------------------------------------------------------------------------------------------
def test_one_cell():
    got = check(np.ones((1, 1), np.float32), np.ones((1, 1), np.int8))
    assert got.cost[0, 0] == 0 and got.indices[0, 0] == 0 and got.backlink[0, 0] == 0 and got.info["reached"] == 1
    got = check(np.ones((1, 1), np.float32), np.zeros((1, 1), np.int8))
    assert got.cost[0, 0] == -100 and got.indices[0, 0] == -100 and got.backlink[0, 0] == 0
    assert got.info["reached"] == 0


@pytest.mark.parametrize("shape", [(1, 200), (200, 1)], ids=lambda s: "%dx%d" % s)
def test_one_row_and_one_column(shape):
    rng = np.random.default_rng(3)
    f = rng.uniform(0.5, 2.0, shape).astype(np.float32)
    f.reshape(-1)[150] = 0  # the cells beyond are cut off
    s = np.zeros(shape, np.int8)
    s.reshape(-1)[[20, 100]] = 1
    s.reshape(-1)[170] = 2  # not 1: no source
    got = check(f, s)
    assert (got.cost.reshape(-1)[150:] == -100).all() and got.info["reached"] == 150
    check(f, s, conn=4)


def test_all_barriers_and_no_source():
    shape = (70, 66)
    bar = np.array([0, -1, -100, np.nan, np.inf], np.float32)[np.arange(70 * 66) % 5].reshape(shape)
    for f, s in ((bar, np.ones(shape, np.int8)), (np.ones(shape, np.float32), np.zeros(shape, np.int8))):
        got = check(f, s)
        assert (got.cost == -100).all() and (got.indices == -100).all() and (got.backlink == 0).all()
        assert got.info["reached"] == 0


def test_empty_rasters():
    from descriptools_amd import cost
    for shape in ((0, 5), (5, 0), (0, 0)):
        got = cost.cost_distance(np.ones(shape, np.float32), np.ones(shape, np.int8), PX, backlink=True)
        assert got.cost.shape == shape and got.indices.shape == shape and got.backlink.shape == shape


# ---- ragged tiles, random friction ----------------------------------------------------------------------------------
CASES = [((65, 63), 0), ((65, 63), 1), ((130, 257), 0)]


@pytest.mark.parametrize("conn", [8, 4])
@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("shape,limit", CASES, ids=["65x63", "65x63-limit1", "130x257"])
def test_random_friction(shape, limit, kind, conn):
    f, s, ref = _random_ref(shape, kind, conn)
    assert ref[4] >= 0.7 * R.passable(f).sum(), "the case reaches too few cells to test anything: change the seed"
    got = check(f, s, conn=conn, limit=limit, ref=ref)
    if limit == 1:
        # one sweep per visit and one visit per round: a front moves one cell per round.  At most 0.4 % of 4095 cells
        # are sources (about 16), and 16 squares of (2 r + 1)^2 cells cover the raster only from r = 8
        assert got.info["rounds"] >= 8
    assert got.info["tile_visits"] >= got.info["rounds"]


def test_result_does_not_depend_on_px_scale_or_run():
    """another pixel size (a power of two: the costs scale exactly), and the same call twice"""
    from descriptools_amd import cost
    f, s, _ = _random_ref((65, 63), "uniform", 8)
    a = cost.cost_distance(f, s, 3.0, backlink=True)
    b = cost.cost_distance(f, s, 3.0, backlink=True)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    c = cost.cost_distance(f, s, 3.0 * 2 ** 20, backlink=True)
    assert np.array_equal(np.where(a.cost >= 0, a.cost * 2 ** 20, -100.0), c.cost)
    assert np.array_equal(a.backlink, c.backlink) and np.array_equal(a.indices, c.indices)
    check(f, s, px=3.0)


# ---- serpentine: many rounds ----------------------------------------------------------------------------------------
def test_serpentine_runs_many_rounds():
    f, s, ref = _serpentine_ref()
    c, i, b, linkless, reached = ref
    assert linkless == 0 and reached == int(R.passable(f).sum())
    parent = R.backlinks(f, s, PX, 8, np.where(c >= 0, c, np.inf))[1]
    cells, entries = R.path_tile_entries(parent, int(np.argmax(c)), TILE)
    assert cells == 8386 and entries >= 100
    got = check(f, s, ref=ref)
    print("serpentine: tile entries %d, rounds %d, tile visits %d" % (entries, got.info["rounds"],
                                                                      got.info["tile_visits"]))
    # a round visits each tile once, so a front crosses at most four tiles (one per colour) per round
    assert got.info["rounds"] >= entries / 4


# ---- an independent kernel ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [8, 4])
def test_basins_of_the_backlinks_are_the_allocation(conn):
    from descriptools_amd import cost, watershed
    f, s, ref = _random_ref((130, 257), "integer", conn)
    got = cost.cost_distance(f, s, PX, connectivity=conn, backlink=True)
    reached = got.cost >= 0
    assert reached.sum() == ref[4]
    assert np.array_equal(watershed.basins(got.backlink)[reached], got.indices[reached])
    f, s, ref = _serpentine_ref()
    got = cost.cost_distance(f, s, PX, backlink=True)
    reached = got.cost >= 0
    assert np.array_equal(watershed.basins(got.backlink)[reached], got.indices[reached])


# ---- the device tier ------------------------------------------------------------------------------------------------
def _dev(ctx, f, s, conn, limit, rounds, want=("indices", "backlink")):
    """dt_dev_cost_distance on resident rasters -> (cost, indices or None, backlink or None, status bits)"""
    from descriptools_amd import _lib
    H, W = f.shape
    d_f, d_s = ctx.to_device(np.ascontiguousarray(f, np.float32)), ctx.to_device(np.ascontiguousarray(s, np.int8))
    d_c = ctx.empty((H, W), np.float64)
    d_i = ctx.empty((H, W), np.int64) if "indices" in want else None
    d_b = ctx.empty((H, W), np.uint8) if "backlink" in want else None
    try:
        _lib.check(_lib.lib().dt_dev_cost_distance(ctx.h, d_f.ptr, d_s.ptr, H, W, PX, conn, limit, rounds, d_c.ptr,
                                                   d_i.ptr if d_i else None, d_b.ptr if d_b else None))
        st = ctx.status()
        return d_c.to_host(), d_i.to_host() if d_i else None, d_b.to_host() if d_b else None, st
    finally:
        for a in (d_f, d_s, d_c, d_i, d_b):
            if a is not None:
                a.free()


def test_device_tier_equals_the_host_tier():
    from descriptools_amd.device import Context
    ctx = Context()
    try:
        for kind, conn in (("exp", 8), ("integer", 4)):
            f, s, ref = _random_ref((130, 257), kind, conn)
            c, i, b, st = _dev(ctx, f, s, conn, 0, 64)
            assert st == 0
            _same("cost", c, ref[0])
            _same("indices", i, ref[1])
            _same("backlink", b, ref[2])
            c, i, b, st = _dev(ctx, f, s, conn, 0, 64, want=())
            assert st == 0 and i is None and b is None
            _same("cost alone", c, ref[0])
    finally:
        ctx.close()


def test_device_tier_budget():
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    f, s, ref = _serpentine_ref()
    ctx = Context()
    try:
        c, i, b, st = _dev(ctx, f, s, 8, 0, 1)
        assert st == 2, "DT_STATUS_NOT_CONVERGED"
        c, i, b, st = _dev(ctx, f, s, 8, 0, 4096)
        assert st == 0
        _same("cost", c, ref[0])
        _same("indices", i, ref[1])
        _same("backlink", b, ref[2])
        for rounds in (0, -1, 4097):
            assert _lib.lib().dt_dev_cost_distance(ctx.h, None, None, 4, 4, PX, 8, 0, rounds, None, None, None) == -1
            assert b"rounds" in _lib.lib().dt_last_error()
        assert _lib.lib().dt_dev_cost_distance(ctx.h, None, None, 0, 7, PX, 8, 0, 1, None, None, None) == 0
    finally:
        ctx.close()


# ---- the host-tier C entry itself -----------------------------------------------------------------------------------
def test_c_entry_with_null_outputs_between_guard_bands():
    from descriptools_amd import _lib
    f, s, ref = _random_ref((65, 63), "uniform", 8)
    H, W = f.shape
    GUARD = 4096

    def guarded(dtype):
        raw = np.full(2 * GUARD + H * W * np.dtype(dtype).itemsize, 0xA5, np.uint8)
        return raw, raw[GUARD:raw.size - GUARD].view(dtype).reshape(H, W)

    L = _lib.lib()
    raw_c, c = guarded(np.float64)
    info = np.full(4, -1, np.int64)
    _lib.check(L.dt_cost_distance(_lib.ptr(f, _lib.c_f32p), _lib.ptr(s, _lib.c_i8p), H, W, PX, 8, 0,
                                  _lib.ptr(c, _lib.c_f64p), None, None, _lib.ptr(info, _lib.c_i64p)))
    _same("cost", c, ref[0])
    assert info[0] >= 1 and info[1] == ref[4] and info[2] == 0 and info[3] >= 2
    assert (raw_c[:GUARD] == 0xA5).all() and (raw_c[-GUARD:] == 0xA5).all()
    # every output, each between its guard bands; info4 may be NULL
    raw_c, c = guarded(np.float64)
    raw_i, i = guarded(np.int64)
    raw_b, b = guarded(np.uint8)
    _lib.check(L.dt_cost_distance(_lib.ptr(f, _lib.c_f32p), _lib.ptr(s, _lib.c_i8p), H, W, PX, 8, 0,
                                  _lib.ptr(c, _lib.c_f64p), _lib.ptr(i, _lib.c_i64p), _lib.ptr(b, _lib.c_u8p), None))
    _same("cost", c, ref[0])
    _same("indices", i, ref[1])
    _same("backlink", b, ref[2])
    for raw in (raw_c, raw_i, raw_b):
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
    # refusals of the entry itself
    assert L.dt_cost_distance(_lib.ptr(f, _lib.c_f32p), _lib.ptr(s, _lib.c_i8p), H, W, PX, 6, 0,
                              _lib.ptr(c, _lib.c_f64p), None, None, None) == -1
    assert L.dt_cost_distance(_lib.ptr(f, _lib.c_f32p), _lib.ptr(s, _lib.c_i8p), H, W, 0.0, 8, 0,
                              _lib.ptr(c, _lib.c_f64p), None, None, None) == -1
    assert L.dt_cost_distance(None, None, 0, 9, PX, 8, 0, None, None, None, _lib.ptr(info, _lib.c_i64p)) == 0
    assert list(info) == [0, 0, 0, 0]


# ---- the absorption example -----------------------------------------------------------------------------------------
def test_absorption_example():
    from descriptools_amd import cost
    from descriptools_amd.device import Context
    f = np.array([[1, 1e30, 1e-30, 1e-30]], np.float32)
    s = np.array([[1, 0, 0, 0]], np.int8)
    ref = R.reference(f, s, PX)
    assert ref[3] == 1
    with pytest.raises(RuntimeError, match=r"\b1 reached cell"):
        cost.cost_distance(f, s, PX)
    ctx = Context()
    try:
        c, i, b, st = _dev(ctx, f, s, 8, 0, 8)
        assert st == 256, "DT_STATUS_NO_BACKLINK"
        _same("cost", c, ref[0])
        _same("indices", i, ref[1])
        _same("backlink", b, ref[2])
        c, i, b, st = _dev(ctx, f[:, :3], s[:, :3], 8, 0, 8)  # without the last cell nothing is absorbed
        assert st == 0
    finally:
        ctx.close()
    ctx = Context()
    try:
        from descriptools_amd import _lib
        d_f, d_s, d_c = ctx.to_device(f), ctx.to_device(s), ctx.empty((1, 4), np.float64)
        _lib.check(_lib.lib().dt_dev_cost_distance(ctx.h, d_f.ptr, d_s.ptr, 1, 4, PX, 8, 0, 8, d_c.ptr, None, None))
        with pytest.raises(RuntimeError, match="DT_STATUS_NO_BACKLINK"):
            ctx.raise_on_status()
        for a in (d_f, d_s, d_c):
            a.free()
    finally:
        ctx.close()


# ---- cost_hand ------------------------------------------------------------------------------------------------------
def test_cost_hand():
    from descriptools_amd import cost, flowhand
    rng = np.random.default_rng(5)
    shape = (65, 63)
    dem = rng.uniform(0, 50, shape).astype(np.float32)
    dem[rng.random(shape) < 0.1] = -100
    dem[10, 10] = -32768.0
    river = (rng.random(shape) < 0.01).astype(np.int8)
    river[10, 10] = 1  # a source on nodata is none
    fr = rng.uniform(0.5, 2.0, shape).astype(np.float32)
    for friction in (None, fr):
        c, i, h = cost.cost_hand(dem, river, PX, friction=friction)
        f = np.where(dem <= -100, np.float32(0), np.float32(1) if friction is None else fr).astype(np.float32)
        rc, ri = R.reference(f, river, PX)[:2]
        _same("cost", c, rc)
        _same("indices", i, ri)
        assert (c[dem <= -100] == -100).all() and (i[dem <= -100] == -100).all()
        want = flowhand.hand_calculator(dem, i)
        assert h.dtype == want.dtype and h.tobytes() == want.tobytes()
    c4 = cost.cost_hand(dem, river, PX, connectivity=4)[0]
    _same("cost, connectivity 4", c4, R.reference(np.where(dem <= -100, 0, 1).astype(np.float32), river, PX, 4)[0])
    # an int16 DEM keeps its dtype in hand
    d16 = np.where(dem <= -100, -100, dem).astype(np.int16)
    c, i, h = cost.cost_hand(d16, river, PX)
    assert h.dtype == flowhand.hand_calculator(d16, i).dtype
    assert h.tobytes() == flowhand.hand_calculator(d16, i).tobytes()


def test_cost_hand_straight_lines_are_exact():
    """friction None and no barriers: along the source's row and column the cost is px * k exactly (pixel sizes whose
    multiples up to 60 are float64 values: the k additions of px round nothing)"""
    from descriptools_amd import cost
    dem = np.zeros((70, 90), np.float32)
    river = np.zeros(dem.shape, np.int8)
    river[30, 40] = 1
    for px in (10.0, 0.375):
        c, i, h = cost.cost_hand(dem, river, px)
        assert (i == 30 * 90 + 40).all() and (h == 0).all()
        k = np.abs(np.arange(90) - 40).astype(np.float64)
        assert np.array_equal(c[30], px * k)
        k = np.abs(np.arange(70) - 30).astype(np.float64)
        assert np.array_equal(c[:, 40], px * k)
