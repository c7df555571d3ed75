"""GPU (-m gpu): regions.label / connected / sieve and reaches.inundate_connected (dt_regions_*, dt_inundate_connected,
k_rg_* in dt_regions.hip) against the numpy reference (tests/_regions_ref.py), every comparison bit for bit on dtype,
shape and bytes: degenerate and ragged shapes, the masks that stress each path (none, all, corners, random around the
percolation thresholds, checkerboard, combs, a serpentine corridor, nested rings, terrain), cells placed on the tile
seams and corners, a root that migrates across seams, sizes, seeds and minimum sizes, mask dtypes, connected inundation
with cases worked out by hand, composition with evaluation.binary_map, determinism, scratch reuse, the device tier and
the library's own refusals.

The reference is flood() (tests/test_regions_host.py holds it to relax() and to scipy); the 513 x 1030 random mask
takes relax(), which is faster there, and the serpentine of that size is known in closed form."""
import functools

import numpy as np
import pytest

import oracle
from conftest import golden

import _reaches_ref as RR
import _regions_ref as R

pytestmark = pytest.mark.gpu

CONN = [4, 8]
T = 64  # checked against regions.TILE below


def _same(name, g, r):
    g, r = np.asarray(g), np.asarray(r)
    assert g.dtype == r.dtype, "%s: dtype %s, reference %s" % (name, g.dtype, r.dtype)
    assert g.shape == r.shape, "%s: shape %s, reference %s" % (name, g.shape, r.shape)
    if g.tobytes() != r.tobytes():
        bad = np.argwhere(~((g == r) | ((g != g) & (r != r))))
        i = tuple(bad[0]) if len(bad) else None
        raise AssertionError("%s: %d cells differ, first at %s: got %r, reference %r"
                             % (name, len(bad), i, g[i] if i else None, r[i] if i else None))


@functools.lru_cache(maxsize=None)
def _masks(H, W):
    p = dict(R.patterns(H, W))
    p["terrain"] = R.terrain_mask(oracle, H, W)[0]
    p["terrain_nodata"] = R.terrain_mask(oracle, H, W, nodata_pct=5)[0]
    for m in p.values():
        m.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _ref(H, W, name, cn):
    lab = R.flood(_masks(H, W)[name], cn)
    lab.setflags(write=False)
    return lab


def check_label(mask, cn, ref=None):
    """label, with and without sizes, against the reference; returns (label, size)"""
    from descriptools_amd import regions
    ref = R.flood(mask, cn) if ref is None else ref
    _same("label", regions.label(mask, cn), ref)
    got = regions.label(mask, connectivity=cn, sizes=True)
    assert isinstance(got, regions.Regions)
    _same("label (sizes=True)", got.label, ref)
    _same("size", got.size, R.sizes(ref))
    fg = np.asarray(mask) != 0
    roots = got.label == np.arange(fg.size, dtype=np.int64).reshape(fg.shape)
    assert int(got.size[roots].sum()) == int(fg.sum())
    assert np.array_equal(got.size[fg], got.size.reshape(-1)[got.label[fg]])
    return got


def test_the_tile_edge_the_tests_assume():
    from descriptools_amd import regions
    assert regions.TILE == T


# ---- shapes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", CONN)
@pytest.mark.parametrize("shape", [(1, 1), (1, 17), (23, 1), (64, 64), (65, 63), (130, 257)], ids=lambda s: "%dx%d" % s)
def test_shapes(shape, cn):
    rng = np.random.default_rng(shape[0] * 7 + shape[1])
    for density in (0.5, 1.0, 0.0):
        check_label((rng.random(shape) < density).astype(np.uint8), cn)
    check_label(R.serpentine(*shape), cn)


@pytest.mark.parametrize("cn", CONN)
def test_513_x_1030(cn):
    """9 x 17 tiles: a random mask at the percolation threshold, and the corridor that crosses every seam it meets --
    one region of known size, the longest chain of roots"""
    from descriptools_amd import regions
    H, W = 513, 1030
    m = (np.random.default_rng(11).random((H, W)) < 0.5).astype(np.uint8)
    check_label(m, cn, R.relax(m, cn))
    s = R.serpentine(H, W)
    got = regions.label(s, cn, sizes=True)
    _same("label", got.label, np.where(s != 0, np.int64(0), np.int64(-100)))
    _same("size", got.size, np.where(s != 0, np.int64(R.serpentine_cells(H, W)), np.int64(0)))


# ---- patterns ----------------------------------------------------------------------------------------------------------
PATTERNS = sorted(R.patterns(3, 3)) + ["terrain", "terrain_nodata"]


@pytest.mark.parametrize("cn", CONN)
@pytest.mark.parametrize("name", PATTERNS)
@pytest.mark.parametrize("shape", [(65, 63), (130, 257)], ids=lambda s: "%dx%d" % s)
def test_patterns(shape, name, cn):
    from descriptools_amd import regions
    H, W = shape
    mask, ref = _masks(H, W)[name], _ref(H, W, name, cn)
    got = check_label(mask, cn, ref)
    fg = mask != 0
    if name == "checkerboard":  # assert outright
        if cn == 8:
            assert (got.label[fg] == 0).all() and (got.size[fg] == fg.sum()).all()
        else:
            assert np.array_equal(got.label[fg], np.flatnonzero(fg.reshape(-1))) and (got.size[fg] == 1).all()
    if name == "serpentine":
        assert (got.label[fg] == 0).all() and (got.size[fg] == R.serpentine_cells(H, W)).all()
    if name == "rings":
        assert np.unique(got.label[fg]).size == (min(H, W) + 1) // 2 // 3 + ((min(H, W) + 1) // 2 % 3 > 0)
    # selection: seeds of none, all, on background only, one per region, a sparse few; min_cells 1, 2, too many
    rng = np.random.default_rng(5)
    zero = np.zeros((H, W), np.uint8)
    one_each = zero.copy()
    last = {}
    for i in np.flatnonzero(fg.reshape(-1)).tolist():
        last[int(ref.reshape(-1)[i])] = i  # the region's largest cell
    one_each.reshape(-1)[list(last.values())] = 1
    sparse = (rng.random((H, W)) < 0.01).astype(np.uint8)
    _same("seeds none", regions.connected(mask, zero, cn), zero)
    _same("seeds all", regions.connected(mask, zero + 1, cn), fg.astype(np.uint8))
    _same("seeds on background only", regions.connected(mask, (~fg).astype(np.uint8), cn), zero)
    _same("one seed per region", regions.connected(mask, one_each, cn), fg.astype(np.uint8))
    _same("sparse seeds", regions.connected(mask, sparse, cn), R.connected(mask, sparse, cn, 1, lambda m, c: ref))
    largest = int(R.sizes(ref).max())
    for mc in (1, 2, largest + 1):
        _same("sieve %d" % mc, regions.sieve(mask, mc, cn), R.sieve(mask, mc, cn, lambda m, c: ref))
        _same("connected, min_cells %d" % mc, regions.connected(mask, sparse, cn, mc),
              R.connected(mask, sparse, cn, mc, lambda m, c: ref))
    _same("sieve too large", regions.sieve(mask, largest + 1, cn), zero)
    _same("sieve 1", regions.sieve(mask, 1, cn), fg.astype(np.uint8))
    _same("seeded by itself", regions.connected(mask, mask, cn), fg.astype(np.uint8))


# ---- seams -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cells", [((T - 1, T - 1), (T, T)), ((T - 1, T), (T, T - 1))], ids=["nw-se", "ne-sw"])
def test_two_cells_across_a_tile_corner(cells):
    """they touch only across the corner of four tiles: one region under 8-connectivity, two under 4"""
    from descriptools_amd import regions
    H, W = 2 * T + 3, 2 * T + 5
    m = np.zeros((H, W), np.uint8)
    for y, x in cells:
        m[y, x] = 1
    a, b = sorted(y * W + x for y, x in cells)
    got8 = regions.label(m, 8, sizes=True)
    got4 = regions.label(m, 4, sizes=True)
    assert got8.label.reshape(-1)[[a, b]].tolist() == [a, a] and got8.size.reshape(-1)[[a, b]].tolist() == [2, 2]
    assert got4.label.reshape(-1)[[a, b]].tolist() == [a, b] and got4.size.reshape(-1)[[a, b]].tolist() == [1, 1]
    for cn, got in ((8, got8), (4, got4)):
        _same("label", got.label, R.flood(m, cn))
    seeds = np.zeros_like(m)
    seeds.reshape(-1)[b] = 1
    assert int(regions.connected(m, seeds, 8).sum()) == 2 and int(regions.connected(m, seeds, 4).sum()) == 1


@pytest.mark.parametrize("cn", CONN)
def test_the_root_migrates_across_seams(cn):
    """a hook whose smallest cell lies in the last tile of the top row of tiles and which runs down, left through the
    tiles below and up again into the first tile: the first tile's own root is far from the region's"""
    H, W = 2 * T + 7, 3 * T + 9
    m = np.zeros((H, W), np.uint8)
    x1, x0, yb = 2 * T + 20, 5, 2 * T + 3
    m[3:yb + 1, x1] = 1     # down from (3, x1), in the last tile of the top row
    m[yb, x0:x1] = 1        # left along the bottom row of tiles
    m[10:yb, x0] = 1        # up into the first tile, ending below the start's row
    m[20, 40] = 1           # a bystander
    got = check_label(m, cn)
    fg = m != 0
    assert got.label[10, x0] == 3 * W + x1 and got.label[20, 40] == 20 * W + 40
    assert got.size[10, x0] == int(fg.sum()) - 1


@pytest.mark.parametrize("cn", CONN)
@pytest.mark.parametrize("shape", [(T - 1, T + 1), (T + 1, 2 * T - 1), (2 * T + 1, 2 * T - 1), (2 * T - 1, 3 * T + 1)],
                         ids=lambda s: "%dx%d" % s)
def test_shapes_one_off_the_tile(shape, cn):
    rng = np.random.default_rng(shape[0] + 3 * shape[1])
    for density in (0.41, 0.59):
        check_label((rng.random(shape) < density).astype(np.uint8), cn)
    check_label(R.serpentine(*shape), cn)
    check_label(R.serpentine(*shape[::-1]).T.copy(), cn)  # vertical corridors


# ---- dtypes ------------------------------------------------------------------------------------------------------------
def test_mask_dtypes():
    from descriptools_amd import regions
    H, W = 65, 63
    base = _masks(H, W)["random41"]
    ref = _ref(H, W, "random41", 8)
    fg = base != 0
    i8 = np.where(fg, np.random.default_rng(2).choice(np.array([-1, 2, -100], np.int8), (H, W)), np.int8(0))
    for m in (fg, i8.astype(np.int8), base.astype(np.uint8) * 255, base.astype(np.int64) << 40,
              np.asfortranarray(base), base.astype(np.int16)[:, ::-1][:, ::-1]):
        _same("label %s" % m.dtype, regions.label(m), ref)
        _same("connected %s" % m.dtype, regions.connected(base, m), fg.astype(np.uint8))
    _same("all foreground", regions.label(np.full((H, W), -100, np.int8)),
          np.zeros((H, W), np.int64))


# ---- connected inundation ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=1)
def _reach_case():
    H, W = 130, 257
    dem, slope, fdr, fac, river = RR.terrain(H, W, 3 * H + W, 30)
    link, idx, hand = RR.network(dem, fdr, river)
    reach, cat, heads = RR.catchments(link, idx)
    nr = heads.size
    assert nr > 8
    rng = np.random.default_rng(9)
    stage = rng.random(nr - 1) * 2.0   # one value short: the last reach's catchment is out of range
    stage[0] = 0.0
    stage[1] = np.nan
    stage[2] = np.inf
    stage[rng.random(nr - 1) < 0.2] = np.nan  # dry reaches cut tributaries off
    return cat, hand, stage, (fac > 1000).astype(np.int8)  # seeded from the main stem only


@pytest.mark.parametrize("cn", CONN)
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_inundate_connected_on_terrain(dtype, cn):
    from descriptools_amd import reaches
    cat, hand, stage, river = _reach_case()
    hand = hand.astype(dtype)
    assert (cat >= stage.size).any()
    plain = reaches.inundate(cat, hand, stage)
    _same("inundate itself", plain, RR.inundate(cat, hand, stage))
    ref, kept = R.inundate_connected(cat, hand, stage, river, cn)
    got = reaches.inundate_connected(cat, hand, stage, river, connectivity=cn)
    _same("depth", got, ref)
    _same("where kept", got[kept], plain[kept])
    wet = R.wet_mask(cat, hand, stage)
    assert np.array_equal(got[~wet], plain[~wet]) and np.isin(got[~kept], (0, -100)).all()
    assert 0 < int((wet & ~kept).sum()) < int(wet.sum())  # something is dropped, something is kept
    _same("the default is 8", reaches.inundate_connected(cat, hand, stage, river),
          R.inundate_connected(cat, hand, stage, river, 8)[0])


def test_inundate_connected_pit_behind_a_ridge_by_hand():
    """a pit below the stage behind a ridge one cell wide; the ridge steps sideways once, which leaves a diagonal gap
    between (3, 3) and (2, 4): the pit is kept under 8-connectivity, dropped under 4"""
    from descriptools_amd import reaches
    H, W = 7, 9
    hand = np.full((H, W), 0.5, np.float32)
    hand[:, 0] = 0.0
    hand[:3, 3] = 10.0
    hand[3:, 4] = 10.0
    hand[:3, 4:] = np.where(hand[:3, 4:] == 10.0, 10.0, 1.0)
    hand[:, 5:] = 1.0
    river = np.zeros((H, W), np.int8)
    river[:, 0] = 1
    cat = np.zeros((H, W), np.int32)
    stage = np.array([2.0])
    d8 = np.array([[2, 1.5, 1.5, 0, 1, 1, 1, 1, 1]] * 3 + [[2, 1.5, 1.5, 1.5, 0, 1, 1, 1, 1]] * 4, np.float32)
    d4 = d8.copy()
    d4[:3, 4:] = 0
    d4[:, 5:] = 0
    _same("inundate", reaches.inundate(cat, hand, stage), d8)
    _same("8", reaches.inundate_connected(cat, hand, stage, river, 8), d8)
    _same("4", reaches.inundate_connected(cat, hand, stage, river, 4), d4)
    for cn, d in ((8, d8), (4, d4)):
        _same("reference %d" % cn, R.inundate_connected(cat, hand, stage, river, cn)[0], d)


def test_inundate_connected_depth_zero_bridges():
    """hand == stage is wet at depth 0 and carries the connection; nodata keeps -100"""
    from descriptools_amd import reaches
    hand = np.array([[0, 1, 2, 0.5, 5, 0.5, -100, 0.25]], np.float64)
    river = np.array([[1, 0, 0, 0, 0, 0, 0, 0]], np.int8)
    cat = np.zeros((1, 8), np.int32)
    want = np.array([[2, 1, 0, 1.5, 0, 0, -100, 0]], np.float32)
    for cn in CONN:
        _same("bridge", reaches.inundate_connected(cat, hand, [2.0], river, cn), want)
        _same("reference", R.inundate_connected(cat, hand, [2.0], river, cn)[0], want)
    _same("float32", reaches.inundate_connected(cat, hand.astype(np.float32), [2.0], river), want)
    # a river cell that is not wet seeds nothing
    _same("dry river", reaches.inundate_connected(cat, hand + np.where(river == 1, 3.0, 0.0), [2.0], river),
          np.array([[0, 0, 0, 0, 0, 0, -100, 0]], np.float32))


# ---- composition ---------------------------------------------------------------------------------------------------------
def test_descriptor_map_kept_to_the_river():
    from descriptools_amd import evaluation, regions
    g = golden("ex_river")
    d, river = g["hand"].astype(np.float64), g["river"]
    binary = evaluation.binary_map(d, 3.0, "under")
    keep = regions.connected(binary == 1, river == 1)
    assert keep.dtype == np.uint8 and keep.shape == d.shape
    assert not (keep[binary != 1]).any()
    wet_river = (binary == 1) & (river == 1)
    assert wet_river.any() and keep[wet_river].all()
    _same("reference", keep, R.connected(binary == 1, river == 1))


# ---- determinism and state -------------------------------------------------------------------------------------------------
def test_twice_the_same_and_nothing_stale():
    from descriptools_amd import regions
    big, small = _masks(130, 257)["random50"], _masks(65, 63)["random59"]
    seeds_b, seeds_s = _masks(130, 257)["random5"], _masks(65, 63)["random5"]
    first = regions.label(big, 8, sizes=True), regions.connected(big, seeds_b, 4, 3)
    mid = regions.label(small, 8, sizes=True), regions.connected(small, seeds_s, 4, 3)
    again = regions.label(big, 8, sizes=True), regions.connected(big, seeds_b, 4, 3)
    for a, b in zip(first[0] + (first[1],), again[0] + (again[1],)):
        assert a.tobytes() == b.tobytes()
    _same("label", mid[0].label, _ref(65, 63, "random59", 8))
    _same("size", mid[0].size, R.sizes(_ref(65, 63, "random59", 8)))
    _same("keep", mid[1], R.connected(small, seeds_s, 4, 3))
    _same("label", first[0].label, _ref(130, 257, "random50", 8))


def test_device_tier_on_a_context():
    """dt_dev_regions_label / _select / dt_dev_inundate_connected on device rasters give the host tier's bytes, twice"""
    from descriptools_amd import _lib, device, reaches, regions
    L = _lib.lib()
    H, W = 130, 257
    mask, seeds = _masks(H, W)["random50"], _masks(H, W)["random5"]
    cat, hand, stage, river = _reach_case()
    hand = np.ascontiguousarray(hand, np.float32)
    ctx = device.Context()
    bufs = [ctx.to_device(np.ascontiguousarray(a)) for a in (mask, seeds, cat, hand, stage, river)]
    m_d, s_d, c_d, h_d, st_d, r_d = bufs
    lab_d, size_d = ctx.empty((H, W), np.int64), ctx.empty((H, W), np.int64)
    keep_d, dep_d = ctx.empty((H, W), np.uint8), ctx.empty((H, W), np.float32)
    bufs += [lab_d, size_d, keep_d, dep_d]
    runs = []
    try:
        for _ in range(2):
            _lib.check(L.dt_dev_regions_label(ctx.h, m_d.ptr, H, W, 8, lab_d.ptr, size_d.ptr))
            _lib.check(L.dt_dev_regions_select(ctx.h, m_d.ptr, s_d.ptr, H, W, 4, 2, keep_d.ptr))
            _lib.check(L.dt_dev_inundate_connected(ctx.h, c_d.ptr, h_d.ptr, 4, st_d.ptr, r_d.ptr, H, W, stage.size, 8,
                                                   dep_d.ptr))
            assert ctx.status() == 0
            runs.append([b.to_host() for b in (lab_d, size_d, keep_d, dep_d)])
            _lib.check(L.dt_dev_regions_label(ctx.h, m_d.ptr, H, W, 4, lab_d.ptr, None))  # without sizes, between runs
        lab4 = lab_d.to_host()
        # refusals: DT_EINVAL with a message, nothing enqueued
        lab, sel, inu = L.dt_dev_regions_label, L.dt_dev_regions_select, L.dt_dev_inundate_connected
        for call, msg in (
                (lambda: lab(ctx.h, m_d.ptr, H, W, 6, lab_d.ptr, None), b"connectivity must be 4 or 8"),
                (lambda: sel(ctx.h, m_d.ptr, None, H, W, 8, 0, keep_d.ptr), b"min_cells must be >= 1"),
                (lambda: lab(ctx.h, None, H, W, 8, lab_d.ptr, None), b"NULL raster"),
                (lambda: sel(ctx.h, m_d.ptr, None, H, W, 8, 1, None), b"NULL raster"),
                (lambda: lab(ctx.h, m_d.ptr, 1 << 16, 1 << 15, 8, lab_d.ptr, None), b"raster of 2^31 cells or more"),
                (lambda: inu(ctx.h, c_d.ptr, h_d.ptr, 2, st_d.ptr, r_d.ptr, H, W, 1, 8, dep_d.ptr),
                 b"hand's element size must be 4 or 8"),
                (lambda: inu(ctx.h, c_d.ptr, h_d.ptr, 4, st_d.ptr, None, H, W, 1, 8, dep_d.ptr), b"NULL raster"),
                (lambda: inu(ctx.h, c_d.ptr, h_d.ptr, 4, st_d.ptr, r_d.ptr, H, W, -1, 8, dep_d.ptr),
                 b"the number of reaches must lie in [0, 2^31)"),
                (lambda: inu(ctx.h, c_d.ptr, h_d.ptr, 4, st_d.ptr, r_d.ptr, H, W, 1, 5, dep_d.ptr),
                 b"connectivity must be 4 or 8")):
            assert call() == -1 and L.dt_last_error() == b"invalid argument: " + msg
        assert L.dt_dev_regions_label(ctx.h, None, 0, 5, 8, None, None) == 0
        ctx.sync()
    finally:
        for b in bufs:
            b.free()
        ctx.close()
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()
    lab, size, keep, depth = runs[0]
    host = regions.label(mask, 8, sizes=True)
    _same("label", lab, host.label)
    _same("size", size, host.size)
    _same("keep", keep, regions.connected(mask, seeds, 4, 2))
    _same("depth", depth, reaches.inundate_connected(cat, hand, stage, river, 8))
    _same("label, 4", lab4, regions.label(mask, 4))


def test_host_tier_refusals():
    """the library itself answers DT_EINVAL with a message to a bad connectivity and a bad min_cells"""
    from descriptools_amd import _lib
    L = _lib.lib()
    p = _lib.ptr
    m = np.ones((2, 2), np.uint8)
    lab = np.zeros((2, 2), np.int64)
    keep = np.zeros((2, 2), np.uint8)
    assert L.dt_regions_label(p(m, _lib.c_u8p), 2, 2, 6, p(lab, _lib.c_i64p), None) == -1
    assert L.dt_last_error() == b"invalid argument: connectivity must be 4 or 8"
    assert L.dt_regions_select(p(m, _lib.c_u8p), None, 2, 2, 8, 0, p(keep, _lib.c_u8p)) == -1
    assert L.dt_last_error() == b"invalid argument: min_cells must be >= 1"
    assert L.dt_regions_select(p(m, _lib.c_u8p), None, 2, 2, 8, 5, p(keep, _lib.c_u8p)) == 0 and not keep.any()
    assert L.dt_regions_label(p(m, _lib.c_u8p), 0, 2, 8, None, None) == 0
