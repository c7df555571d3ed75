"""GPU (-m gpu): proximity.nearest_river / euclidean_hand (dt_proximity, k_px_* in dt_proximity.hip) against the numpy
reference (tests/_proximity_ref.py), indices and distance bit for bit on every cell: degenerate and ragged shapes, rows
and columns long enough for the segment carries of the row pass and 13 levels of the column pass, the source patterns
that stress each path (none, all, corners, one row, one column: the sentinel path, sparse, dense, a lattice of ties,
terrain), values other than 1, nodata, HAND and its dtypes, a cross-check against the flow-path HAND where the flow path
is the straight line, composition with GFI and the reach catchments, determinism and scratch reuse.

The reference is brute() wherever cells x sources stays below 3e7 pairs, sweep() above (tests/test_proximity_host.py
holds the two to each other)."""
import functools

import numpy as np
import pytest

import oracle
from conftest import assert_float_close

import _proximity_ref as R
import _reaches_ref as RR

pytestmark = pytest.mark.gpu

PX = 12.3  # inexact in binary: the float64 product is rounded, then once more to float32


def _same(name, g, r):
    g, r = np.asarray(g), np.asarray(r)
    assert g.dtype == r.dtype, "%s: dtype %s, reference %s" % (name, g.dtype, r.dtype)
    assert g.shape == r.shape, "%s: shape %s, reference %s" % (name, g.shape, r.shape)
    if g.tobytes() != r.tobytes():
        bad = np.argwhere(g != r)
        i = tuple(bad[0]) if len(bad) else None
        raise AssertionError("%s: %d cells differ, first at %s: got %r, reference %r"
                             % (name, len(bad), i, g[i] if i else None, r[i] if i else None))


def reference(river, nodata=None, px=PX, form=None):
    if form is None:
        form = "brute" if river.size * max(1, int(R.sources(river, nodata).sum())) <= 3e7 else "sweep"
    idx, dist, _ = getattr(R, form)(river, nodata, px)
    return idx, dist


def check(river, dem=None, px=PX, form=None):
    from descriptools_amd import proximity
    got = proximity.nearest_river(river, px, dem=dem)
    nodata = None if dem is None else np.asarray(dem) <= -100
    idx, dist = reference(np.asarray(river), nodata, px, form)
    _same("indices", got.indices, idx)
    _same("distance", got.distance, dist)
    return got


def _random(shape, density, seed, at_most=None):
    rng = np.random.default_rng(seed)
    river = (rng.random(shape) < density).astype(np.int8)
    if at_most is not None:
        flat = np.flatnonzero(river.reshape(-1))
        river.reshape(-1)[flat[at_most:]] = 0
    if not river.any():
        river.reshape(-1)[rng.integers(river.size)] = 1
    return river


# ---- shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (1, 17), (23, 1), (64, 64), (65, 63), (130, 257)], ids=lambda s: "%dx%d" % s)
def test_shapes_against_brute(shape):
    check(_random(shape, 0.05, 11), form="brute")


@pytest.mark.parametrize("shape", [(3, 5000), (5000, 3)], ids=lambda s: "%dx%d" % s)
def test_long_rows_and_columns_against_brute(shape):
    """5000 columns: 79 segments of 64, so the carries cross a 64-segment chunk; 5000 rows: 13 levels"""
    river = _random(shape, 0.003, 12, at_most=50)
    assert 1 <= river.sum() <= 50
    check(river, form="brute")
    far = np.zeros(shape, np.int8)  # one source at the far end: every carry and every level hands it on
    far[-1, -1] = 1
    check(far, form="brute")


def test_513x1030_against_sweep():
    check(_random((513, 1030), 0.002, 13), form="sweep")


# ---- source patterns ------------------------------------------------------------------------------------------------
def _terrain_river(shape, nod):
    H, W = shape
    dem = oracle.synth_dem(7, H, W, 0, 0, H, W, nod)
    _, fdr = oracle.slope_d8(dem, 10.0)
    fac = oracle.flowacc(fdr, dem)
    return dem, fdr, fac, (fac >= max(8, H * W // 512)).astype(np.int8)


def _pattern(name, shape):
    H, W = shape
    z = np.zeros(shape, np.int8)
    if name == "none":
        return z, None
    if name == "all":
        return z + 1, None
    if name.startswith("corner"):
        y, x = {"corner_nw": (0, 0), "corner_ne": (0, W - 1), "corner_sw": (H - 1, 0), "corner_se": (H - 1, W - 1)}[name]
        z[y, x] = 1
        return z, None
    if name == "one_row":
        z[H // 3, ::3] = 1
        return z, None
    if name == "one_column":
        z[::5, (2 * W) // 3] = 1
        return z, None
    if name == "random_0.2pct":
        return _random(shape, 0.002, 21), None
    if name == "random_30pct":
        return _random(shape, 0.30, 22), None
    if name == "lattice":
        z[::8, ::8] = 1
        return z, None
    if name in ("terrain", "terrain_nodata"):
        dem, _, _, river = _terrain_river(shape, 5 if name == "terrain_nodata" else 0)
        assert river.any() and ((dem <= -100).any() == (name == "terrain_nodata"))
        return river, dem
    raise KeyError(name)


PATTERNS = ["none", "all", "corner_nw", "corner_ne", "corner_sw", "corner_se", "one_row", "one_column", "random_0.2pct",
            "random_30pct", "lattice", "terrain", "terrain_nodata"]


@pytest.mark.parametrize("shape", [(65, 63), (130, 257)], ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", PATTERNS)
def test_source_patterns(name, shape):
    river, dem = _pattern(name, shape)
    got = check(river, dem)
    if name == "none":
        assert (got.indices == -100).all() and (got.distance == -100).all()
    if name == "all":
        assert np.array_equal(got.indices.reshape(-1), np.arange(river.size)) and not got.distance.any()


def test_the_lattice_is_the_tie_test():
    """on the 8-cell lattice a fifth of the cells have more than one nearest source: 455 of 2304 at 48 x 48"""
    river = np.zeros((48, 48), np.int8)
    river[::8, ::8] = 1
    sy, sx = np.nonzero(river)
    yy, xx = np.mgrid[0:48, 0:48]
    d = (yy[..., None] - sy) ** 2 + (xx[..., None] - sx) ** 2
    assert int(((d == d.min(axis=2, keepdims=True)).sum(axis=2) > 1).sum()) == 455
    check(river, form="brute")


def test_values_other_than_1_are_not_sources():
    rng = np.random.default_rng(31)
    river = rng.choice(np.array([0, 2, -1, 1], np.int8), size=(65, 63), p=[0.5, 0.24, 0.24, 0.02])
    got = check(river)
    assert (river.reshape(-1)[got.indices.reshape(-1)] == 1).all()
    only = np.where(river == 1, 0, river)  # 0, 2 and -1 alone: no source at all
    assert (check(only).indices == -100).all()


# ---- nodata ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_nodata(dtype):
    from descriptools_amd import _lib, proximity
    H, W = 65, 63
    river = np.zeros((H, W), np.int8)
    river[10, 5] = river[60, 60] = river[64, 0] = 1
    river[20, 30] = 1  # a river cell on nodata: not a source
    dem = np.full((H, W), 50.0, dtype)
    if dtype == np.float64:
        dem += 1e-9  # heights float32 cannot hold
        assert _lib.heights(dem)[1]
        dem[3, 3] = -99.9999999  # float32 rounds it to -100; in the DEM's own dtype it is not nodata
        dem[3, 4] = -100.0000001
    dem[20, 30] = -100
    dem[10, 6:40] = -100  # a wall of nodata east of the source at (10, 5) ...
    dem[0:30, 20] = -150
    got = check(river, dem)
    nodata = dem <= -100
    assert (got.indices[nodata] == -100).all() and (got.distance[nodata] == -100).all()
    assert (got.indices[~nodata] != 20 * W + 30).all()
    assert got.indices[10, 41] == 10 * W + 5 and got.distance[10, 41] == np.float32(PX * 36.0)  # ... is no barrier
    free = proximity.nearest_river(np.where(nodata, 0, river), PX)  # the same sources, no nodata at all
    _same("indices beyond nodata", got.indices[~nodata], free.indices[~nodata])
    _same("distance beyond nodata", got.distance[~nodata], free.distance[~nodata])
    if dtype == np.float64:
        assert got.indices[3, 3] >= 0 and got.indices[3, 4] == -100


# ---- HAND -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.int16, np.float32, np.float64])
def test_euclidean_hand(dtype):
    from descriptools_amd import flowhand, proximity
    dem, fdr, _, river = _terrain_river((130, 257), 5)
    if dtype == np.int16:
        dem = np.where(dem <= -100, -100, np.rint(dem)).astype(np.int16)
    elif dtype == np.float64:
        dem = np.where(dem <= -100, -100.0, dem.astype(np.float64) + 1e-9)
    dist, idx, hand = proximity.euclidean_hand(dem, river, PX)
    near = proximity.nearest_river(river, PX, dem=dem)
    _same("distance", dist, near.distance)
    _same("indices", idx, near.indices)
    _same("hand", hand, flowhand.hand_calculator(dem, idx))
    ok = idx >= 0
    diff = dem - dem.reshape(-1)[np.where(ok, idx, 0)]
    _same("hand (numpy)", hand, np.where(ok, np.maximum(diff, 0), -100).astype(dem.dtype))
    assert (hand[dem <= -100] == -100).all()
    flow = flowhand.flow_hand_index(dem, fdr, river, PX)
    assert [a.dtype for a in (dist, idx, hand)] == [a.dtype for a in flow]
    assert [a.dtype for a in (dist, idx, hand)] == [np.float32, np.int64, np.dtype(dtype)]


def test_flow_path_that_is_the_straight_line():
    """independent of the new reference: every cell flows east into a river along the last column"""
    from descriptools_amd import flowhand, proximity
    H, W, px = 40, 50, 10.0
    fdr = np.ones((H, W), np.uint8)
    river = np.zeros((H, W), np.int8)
    river[:, -1] = 1
    fd, idx, _ = flowhand.flow_hand_index(np.zeros((H, W), np.float32), fdr, river, px)
    got = proximity.nearest_river(river, px)
    _same("indices", got.indices, idx)
    _same("distance", got.distance, fd)


# ---- composition ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _composed():
    from descriptools_amd import proximity
    dem, fdr, fac, river = _terrain_river((130, 257), 5)
    dist, idx, hand = proximity.euclidean_hand(dem, river, 10.0)
    return dem, fdr, fac, river, idx, hand


def test_gfi_on_euclidean_outputs():
    from descriptools_amd import gfi
    dem, fdr, fac, river, idx, hand = _composed()
    assert_float_close(gfi.gfi_calculator(hand, fac, idx, 0.4, 0.1, 10.0), oracle.gfi(hand, fac, idx, 0.4, 0.1, 10.0),
                       rtol=1e-5, atol=1e-6, what="gfi")
    ra = gfi.river_accumulation(fac, idx)
    _same("river accumulation", ra, np.where(idx != -100, fac.reshape(-1)[np.where(idx != -100, idx, 0)],
                                             fac.reshape(-1)[0]).astype(np.int64))


def test_reach_catchments_on_euclidean_indices():
    from descriptools_amd import reaches
    dem, fdr, fac, river, idx, hand = _composed()
    link, _, _ = RR.network(dem, fdr, river)
    got = reaches.catchments(link, idx)
    reach, cat, heads = RR.catchments(link, idx)
    _same("reach", got.reach, reach)
    _same("catchment", got.catchment, cat)
    _same("heads", got.heads, heads)
    assert (cat[idx >= 0] >= 0).all()  # every allocated cell belongs to a reach


# ---- determinism and state ------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bytes():
    from descriptools_amd import proximity
    river, _ = _pattern("lattice", (130, 257))
    a = proximity.nearest_river(river, PX)
    b = proximity.nearest_river(river, PX)
    assert a.indices.tobytes() == b.indices.tobytes() and a.distance.tobytes() == b.distance.tobytes()


def test_a_call_after_another_shape():
    """the scratch of a larger, then a smaller, then the first raster again: nothing stale is read"""
    first = _random((65, 63), 0.01, 41)
    check(_random((130, 257), 0.3, 42))
    check(first)
    check(_random((23, 1), 0.2, 43))
    check(first)
