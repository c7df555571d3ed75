"""GPU (-m gpu): D-infinity distance down to the stream (descriptools_amd.dinf.distance_down / hand,
dt_dinf_distance_down; k_dd_* in dt_dinf_dist.hip) against the numpy reference (tests/_dinf_dist_ref.py), bit for bit
in the horizontal, the vertical and the surface raster: every value is a function of its receivers' final values in a
fixed float64 association, so nothing depends on the schedule.  _visit_limit=1 makes a workgroup do one sweep per
visit, which forces many global rounds on small rasters."""
import ctypes as C

import numpy as np
import pytest

from descriptools_amd import _lib, dinf, reaches

import _dinf_dist_ref as DR
import _dinf_ref as R

pytestmark = pytest.mark.gpu

PX = DR.PX
NAMES = ("horizontal", "vertical", "surface")


def _bits_equal(name, g, r, equal_nan=False):
    assert g.dtype == np.float64 and r.dtype == np.float64 and g.shape == r.shape, name
    same = g.view(np.int64) == r.view(np.int64)
    if equal_nan:
        same |= np.isnan(g) & np.isnan(r)
    if not same.all():
        bad = np.argwhere(~same)
        i = tuple(bad[0])
        raise AssertionError("%s: %d cells differ, first at %s: got %r, reference %r" % (name, len(bad), i, g[i], r[i]))


def check(angle, river, px, dem, stat="ave", check_edges=True, limits=(0,), want=None):
    """GPU against the reference (or `want`) for every visit limit; returns the reference"""
    if want is None:
        want = DR.distance_down(angle, river, px, dem, stat, check_edges)
    for lim in limits:
        got = dinf.distance_down(angle, river, px, dem, stat, check_edges, _visit_limit=lim)
        assert isinstance(got, dinf.DinfDistance)
        for name, g, r in zip(NAMES, got, want):
            if r is None:
                assert g is None, name
            else:
                _bits_equal("%s (stat %s, check_edges %s, visit limit %d)" % (name, stat, check_edges, lim), g, r)
    return want


def call(angle, river, px, dem=None, stat=0, check_edges=1, visit_limit=0):
    """the C entry itself -> (rc, h, v, s, info4)"""
    a = np.ascontiguousarray(angle, np.float32)
    r = np.ascontiguousarray(river, np.int8)
    d = None if dem is None else np.ascontiguousarray(dem, np.float32)
    H, W = a.shape
    h = np.empty((H, W), np.float64)
    v = None if d is None else np.empty((H, W), np.float64)
    s = None if d is None else np.empty((H, W), np.float64)
    info = np.full(4, -7, np.int64)
    p = _lib.ptr
    rc = _lib.lib().dt_dinf_distance_down(p(a, _lib.c_f32p), p(r, _lib.c_i8p), p(d, _lib.c_f32p), H, W, px, stat,
                                          check_edges, visit_limit, p(h, _lib.c_f64p), p(v, _lib.c_f64p),
                                          p(s, _lib.c_f64p), p(info, _lib.c_i64p))
    return rc, h, v, s, info


# ---- terrains --------------------------------------------------------------------------------------------------------
SEEDS = [(65, 63, 0, 50), (130, 257, 2, 100), (200, 333, 2, 200)]


def _terrain_case(seed, surface, stat, check_edges, limits):
    t = DR.terrain(*seed)
    a, z = t[surface]
    want = DR.ref(*seed, surface, stat, check_edges)
    check(a, t["river"], PX, z, stat, check_edges, limits, want=want)
    live = a != -100
    reach = (want[0] != -100) & live
    frac = reach.sum() / live.sum()
    assert frac >= 0.30, "only %.2f of the cells reach: the case shows little" % frac
    if surface == "raw":
        assert (live & ~reach).any(), "on the raw surface some cell must fail to reach"


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("surface", ["raw", "cond"])
@pytest.mark.parametrize("stat", DR.STATS)
@pytest.mark.parametrize("check_edges", [True, False])
def test_terrain(seed, surface, stat, check_edges):
    _terrain_case(seed, surface, stat, check_edges, (0, 1))


@pytest.mark.parametrize("surface", ["raw", "cond"])
@pytest.mark.parametrize("check_edges", [True, False])
def test_terrain_600_by_1000(surface, check_edges):
    _terrain_case((600, 1000, 2, 2000), surface, "ave", check_edges, (0,))


@pytest.mark.parametrize("shape", [(32, 32), (31, 33), (33, 31), (64, 96), (63, 97), (65, 95)])
def test_tile_edges(shape):
    """the tile is 32 x 32: whole tiles and one cell less / more in either direction"""
    H, W = shape
    t = DR.terrain(H, W, 0, 30)
    for surface in ("raw", "cond"):
        a, z = t[surface]
        for ce in (True, False):
            want = check(a, t["river"], PX, z, "ave", ce, (0, 1))
            assert (want[0] > 0).any()


# ---- degenerate shapes -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 7), (9, 1)])
@pytest.mark.parametrize("what", ["target", "no_target", "nodata"])
def test_degenerate_shapes(shape, what):
    H, W = shape
    # along the raster towards its last cell (east in a row, south in a column); the last cell has no receiver
    a = np.full(shape, R.octant_angle(0 if H == 1 else 6), np.float32)
    a[-1, -1] = -1
    river = np.zeros(shape, np.int8)
    dem = np.arange(H * W, 0, -1, dtype=np.float32).reshape(shape)
    if what == "target":
        river[-1, -1] = 1
    if what == "nodata":
        a[:] = -100
        river[:] = 1
    for ce in (True, False):
        want = check(a, river, 2.5, dem, "ave", ce, (0, 1))
        if what == "target":
            assert (want[0] == 2.5 * np.arange(H * W - 1, -1, -1).reshape(shape)).all()
            assert (want[1] == np.arange(H * W - 1, -1, -1).reshape(shape)).all()
        else:
            assert all((m == -100).all() for m in want)
    rc, h, v, s, info = call(a, river, 2.5, dem)
    assert rc == 0
    n = H * W
    assert info.tolist()[1:] == {"target": [n, 0, 0], "no_target": [0, n, 0], "nodata": [0, 0, 0]}[what]


def test_empty_rasters():
    for shape in ((0, 5), (4, 0), (0, 0)):
        out = dinf.distance_down(np.zeros(shape, np.float32), np.zeros(shape, np.int8), 1.0, np.zeros(shape, np.float32))
        assert all(m.shape == shape and m.dtype == np.float64 for m in out)


# ---- the snake: one path that crosses every tile border hundreds of times -----------------------------------------------
def _snake(n=192):
    """even rows run alternately east and west, joined by south connectors through the odd rows.  Of the other
    odd-row cells those in even columns are -1 (dead from the start) and those in odd columns flow east into such a
    cell (or off the raster): a round has to settle them dead.  -> angle, path (flat indices, head first)"""
    E, W_, S = R.octant_angle(0), R.octant_angle(4), R.octant_angle(6)
    a = np.full((n, n), -1, np.float32)
    a[1::2, 1::2] = E
    path = []
    for i, y in enumerate(range(0, n, 2)):
        xs = range(n) if i % 2 == 0 else range(n - 1, -1, -1)
        a[y, :] = E if i % 2 == 0 else W_
        for x in xs:
            path.append(y * n + x)
        if y + 2 < n:
            xe = n - 1 if i % 2 == 0 else 0
            a[y, xe] = S
            a[y + 1, xe] = S
            path.append((y + 1) * n + xe)
    a.reshape(-1)[path[-1]] = -1  # the outlet has no receiver
    return a, np.asarray(path)


@pytest.mark.parametrize("limit", [0, 1])
def test_snake(limit):
    n = 192
    a, path = _snake(n)
    assert 18000 < len(path) < 19000
    river = np.zeros((n, n), np.int8)
    river.reshape(-1)[path[-1]] = 1
    hops = np.zeros(n * n, np.int64)
    hops[path] = np.arange(len(path) - 1, -1, -1)
    dem = (hops * 0.25).astype(np.float32).reshape(n, n)  # every sum is exact
    px = 2.0
    # a plain loop along the path, from the outlet up (every hop is cardinal: L = px, dz = 0.25)
    eh, ev, es = (np.full(n * n, -100.0) for _ in range(3))
    hop_s = float(np.sqrt(px * px + 0.25 * 0.25))
    h = v = s = 0.0
    for c in path[::-1]:
        eh[c], ev[c], es[c] = h, v, s
        h, v, s = h + px, v + 0.25, s + hop_s
    want = tuple(m.reshape(n, n) for m in (eh, ev, es))
    on = np.zeros(n * n, bool)
    on[path] = True
    assert (want[0].reshape(-1)[~on] == -100).all(), "the cells off the path are dead"
    if limit == 0:
        for ce in (True, False):
            check(a, river, px, dem, "ave", ce, (limit,), want=want)
    rc, gh, gv, gs, info = call(a, river, px, dem, visit_limit=limit)
    assert rc == 0
    for name, g, r in zip(NAMES, (gh, gv, gs), want):
        _bits_equal("%s (C entry, visit limit %d)" % (name, limit), g, r)
    assert info[0] > 1 and info[1] == len(path) and info[2] == n * n - len(path) and info[3] == 0


# ---- cycles ----------------------------------------------------------------------------------------------------------
def test_cycles_cost_one_quiet_round():
    H, W = 40, 70
    yy, xx = np.mgrid[0:H, 0:W]
    dem = (500 - 2 * yy - 0.5 * xx).astype(np.float32)  # a healthy hillslope that drains south-south-east
    a, _ = R.flow_direction(dem, PX)
    a = a.copy()
    river = np.zeros((H, W), np.int8)
    river[H - 4, :] = 1
    oct_ = R.octant_angle
    # a two-cell cycle with a tributary from the north
    a[10, 10], a[10, 11] = oct_(0), oct_(4)
    a[5:10, 10] = oct_(6)
    # an eight-cell ring (clockwise around (20, 40)) with tributaries from the north and the west
    ring = [(19, 39, 0), (19, 40, 0), (19, 41, 6), (20, 41, 6), (21, 41, 4), (21, 40, 4), (21, 39, 2), (20, 39, 2)]
    for y, x, k in ring:
        a[y, x] = oct_(k)
    a[12:19, 40] = oct_(6)
    a[20, 30:39] = oct_(0)
    (rh, rv, rs), x = DR.distance_down(a, river, PX, dem, "ave", True, full=True)
    unset = x["state"] == 0
    on_cycle = np.zeros((H, W), bool)
    on_cycle[10, 10:12] = True
    on_cycle[5:10, 10] = True
    on_cycle[12:19, 40] = True
    on_cycle[20, 30:39] = True
    for y, x_, _ in ring:
        on_cycle[y, x_] = True
    assert unset[on_cycle].all() and unset.sum() >= on_cycle.sum()
    for ce in (True, False):
        want = check(a, river, PX, dem, "ave", ce, (0, 1))
        _, xs = DR.distance_down(a, river, PX, dem, "ave", ce, full=True)
        assert (want[0][xs["state"] == 0] == -100).all() and (want[0][on_cycle] == -100).all()
        assert (want[0] != -100).sum() > H * W // 2
        rc, h, v, s, info = call(a, river, PX, dem, check_edges=int(ce))
        assert rc == 0  # the call returned: a round that settles nothing ends it
        assert info[3] == (xs["state"] == 0).sum() and info[1] == (xs["state"] == 1).sum() \
            and info[2] == (xs["state"] == 2).sum()


# ---- heights ---------------------------------------------------------------------------------------------------------
def test_without_heights():
    t = DR.terrain(*SEEDS[1])
    a, z = t["raw"]
    for ce in (True, False):
        full = dinf.distance_down(a, t["river"], PX, z, check_edges=ce)
        only = dinf.distance_down(a, t["river"], PX, check_edges=ce, _visit_limit=3)
        assert only.vertical is None and only.surface is None
        _bits_equal("horizontal without heights", only.horizontal, full.horizontal)
        _bits_equal("hand", dinf.hand(a, t["river"], z, PX, check_edges=ce), full.vertical)


def test_nan_height_on_a_hillslope():
    t = DR.terrain(*SEEDS[1])
    a, z = t["cond"]
    base = DR.ref(*SEEDS[1], "cond", "ave", False)
    far = np.argwhere((base[0] > 8 * PX) & (t["river"] == 0))
    z = z.copy()
    for y, x in far[:: max(1, len(far) // 5)][:5]:
        z[y, x] = np.nan
    z[tuple(far[0])] = np.inf
    with np.errstate(all="ignore"):
        want = DR.distance_down(a, t["river"], PX, z, "ave", False)
    assert np.isnan(want[1]).any() and np.isnan(want[2]).any()
    for lim in (0, 1):
        got = dinf.distance_down(a, t["river"], PX, z, "ave", False, _visit_limit=lim)
        _bits_equal("horizontal", got.horizontal, want[0])
        _bits_equal("horizontal is not affected", got.horizontal, base[0])
        _bits_equal("vertical", got.vertical, want[1], equal_nan=True)
        _bits_equal("surface", got.surface, want[2], equal_nan=True)


def test_scratch_hygiene():
    big, small = DR.terrain(*SEEDS[2]), DR.terrain(*SEEDS[0])
    check(big["raw"][0], big["river"], PX, big["raw"][1], want=DR.ref(*SEEDS[2], "raw", "ave", True))
    for surface in ("raw", "cond"):
        check(small[surface][0], small["river"], PX, small[surface][1], limits=(0, 1),
              want=DR.ref(*SEEDS[0], surface, "ave", True))


# ---- integration -----------------------------------------------------------------------------------------------------
def test_reaches_take_the_dinf_hand():
    seed = SEEDS[1]
    t = DR.terrain(*seed)
    a, z = t["cond"]
    H, W = a.shape
    hand = dinf.hand(a, t["river"], z, PX)
    _bits_equal("hand", hand, DR.ref(*seed, "cond", "ave", True)[1])
    n_reaches = 4
    cat = np.where(a == -100, -100, np.arange(W)[None, :] * n_reaches // W).astype(np.int32)
    stage = np.array([0.5, 2.0, np.nan, 8.0])
    depth = reaches.inundate(cat, hand, stage)
    st = np.where(cat >= 0, stage[np.clip(cat, 0, n_reaches - 1)], np.nan)
    with np.errstate(invalid="ignore"):
        wet = (cat >= 0) & np.isfinite(st) & (hand >= 0) & (hand <= st)
    want = np.where(hand == -100, np.float32(-100), np.where(wet, (st - hand).astype(np.float32), np.float32(0)))
    assert depth.dtype == np.float32 and np.array_equal(depth, want.astype(np.float32)) and (depth > 0).any()
    stages = np.array([0.0, 1.0, 4.0, 16.0])
    tab = reaches.hydraulic_tables(cat, hand, PX, stages, n_reaches)
    for r in range(n_reaches):
        for k, sk in enumerate(stages):
            assert tab.cells[r, k] == ((cat == r) & (hand >= 0) & (hand <= sk)).sum()
    assert tab.cells[:, -1].min() > 0


# ---- the C entry's refusals ------------------------------------------------------------------------------------------
def test_c_level_refusals():
    L = _lib.lib()
    a = np.full((4, 5), -1, np.float32)
    river = np.ones((4, 5), np.int8)
    dem = np.zeros((4, 5), np.float32)
    assert call(a, river, 1.0, dem)[0] == 0

    def refused(rc):
        assert rc == -1 and len(L.dt_last_error()) > 0

    refused(call(a, river, 1.0, dem, stat=3)[0])
    refused(call(a, river, 1.0, dem, stat=-1)[0])
    refused(call(a, river, 1.0, dem, check_edges=2)[0])
    refused(call(a, river, 1.0, dem, visit_limit=-1)[0])
    refused(call(a, river, 0.0, dem)[0])
    out = np.empty((4, 5), np.float64)
    p = _lib.ptr
    A, Rv, D, O = p(a, _lib.c_f32p), p(river, _lib.c_i8p), p(dem, _lib.c_f32p), p(out, _lib.c_f64p)
    f = L.dt_dinf_distance_down
    refused(f(A, Rv, None, 4, 5, 1.0, 0, 1, 0, O, O, None, None))   # v without dem
    refused(f(A, Rv, None, 4, 5, 1.0, 0, 1, 0, O, None, O, None))   # s without dem
    refused(f(None, Rv, D, 4, 5, 1.0, 0, 1, 0, O, None, None, None))
    refused(f(A, None, D, 4, 5, 1.0, 0, 1, 0, O, None, None, None))
    refused(f(A, Rv, D, 4, 5, 1.0, 0, 1, 0, None, None, None, None))
    refused(f(A, Rv, D, -1, 5, 1.0, 0, 1, 0, O, None, None, None))
    # dem with the vertical raster alone, and with neither: both are served
    v = np.empty((4, 5), np.float64)
    assert f(A, Rv, D, 4, 5, 1.0, 0, 1, 0, O, p(v, _lib.c_f64p), None, None) == 0 and (v == 0).all() and (out == 0).all()
    assert f(A, Rv, D, 4, 5, 1.0, 0, 1, 0, O, None, None, None) == 0
    # an angle outside the contract fails the call
    bad = a.copy()
    bad[1, 1] = np.nan
    rc = call(bad, river, 1.0, dem)[0]
    assert rc == -1 and b"angle" in L.dt_last_error()
    assert call(a, river, 1.0, dem)[0] == 0, "the status of a failed call does not leak into the next"
