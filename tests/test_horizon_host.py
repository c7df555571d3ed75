"""CPU (not gpu): the numpy reference of the line-of-sight attributes (tests/_horizon_ref.py) is pinned here -- the
landform table and its duality, the flatness tangent, surfaces whose landforms are known, the cells that have a value,
nodata in a line of sight -- and so are the argument checks of descriptools_amd.horizon, which run before any library
call.

A tie.  The digit rule gives -1 to a direction with |tmax| == |tmin| > T whatever the sign (rule 2 holds with
|tmax| <= |tmin|).  That is every direction with a single sample, and in exact arithmetic every up-slope ray of an
exactly straight flank: all its samples share one tangent, so whether an ideal ramp, inverted cone or V-valley reads +1
or -1 up-slope is a matter of the last bit of k * (1 / (k step)).  test_a_tie_goes_to_minus_one pins the rule.  The
analytic landforms are therefore asserted on surfaces whose flanks steepen by 1 % per cell (curl = 0.01 in
_horizon_ref: s + 0.01 s^2 for the distance s, 10^3 times the float32 rounding of the heights), where the tangents of
an up-slope ray grow with k and tmax > tmin > T holds by construction -- the tests assert that too -- and where every
direction has two samples or more.  What holds on the exactly straight surfaces whatever the rounding (the down-slope
-1 digits, the level 0 digits, peak and ridge) is asserted on those."""
import math

import numpy as np
import pytest

import _horizon_ref as R
from descriptools_amd import horizon

T1 = R.flat_tangent(1.0)
N, NE, E, SE, S, SW, W, NW = range(8)


def _digits(dem, px, radius, skip=0, T=T1):
    out = R.attributes(dem, px, T, ("pattern", "landform"), radius, skip)
    return R.decode(out["pattern"]), out["landform"], out["pattern"]


# ---- the table and the tangent -----------------------------------------------------------------------------------
def test_landform_table_is_self_dual():
    """swapping m and p maps 2 <-> 10, 3 <-> 9, 4 <-> 8, 5 <-> 7 and leaves 1 and 6 fixed; every (m, p) with
    m + p <= 8 has a landform and no other entry has one"""
    assert list(R.DUAL) == [0, 1, 10, 9, 8, 7, 6, 5, 4, 3, 2]
    for m in range(9):
        for p in range(9):
            if m + p <= 8:
                assert 1 <= R.TABLE[m, p] <= 10
                assert R.TABLE[p, m] == R.DUAL[R.TABLE[m, p]], (m, p)
            else:
                assert R.TABLE[m, p] == 0
    assert set(R.TABLE[R.TABLE > 0]) == set(range(1, 11)) == set(horizon.LANDFORMS)
    # the module's table is the reference's
    assert len(horizon.LANDFORM_TABLE) == 9
    for m, row in enumerate(horizon.LANDFORM_TABLE):
        assert tuple(R.TABLE[m, :9 - m]) == tuple(row)
    assert horizon.LANDFORMS[2] == "peak" and horizon.LANDFORMS[10] == "pit" and horizon.LANDFORMS[9] == "valley"


def test_flat_tangent():
    assert horizon.flat_tangent(0) == 0.0
    assert horizon.flat_tangent(1.0) == math.tan(math.radians(1.0)) == R.flat_tangent(1.0)
    assert horizon.flat_tangent(30) == math.tan(math.radians(30.0))
    assert abs(horizon.flat_tangent(45.0) - 1.0) < 1e-15
    assert horizon.flat_tangent(89.9) > 500
    for bad in (90, 90.0, -0.5, 120, float("nan"), float("inf"), True, "flat", None):
        with pytest.raises(ValueError):
            horizon.flat_tangent(bad)


def test_reciprocal_table():
    inv = R.reciprocals(7.3, 64)
    assert inv[0][1] == 1.0 / 7.3 and inv[0][64] == 1.0 / (64.0 * 7.3)
    assert inv[1][3] == 1.0 / (3.0 * (7.3 * 1.4142135623730951))


# ---- analytic surfaces, flat = 1 degree ---------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 3, 10])
def test_level_plane(radius):
    dem = np.full((2 * radius + 5, 2 * radius + 7), 250, np.float32)
    out = R.attributes(dem, 10.0, T1, R.OUTPUTS, radius)
    has = out["landform"] != 0
    assert has.sum() == (dem.shape[0] - 2) * (dem.shape[1] - 2)
    assert (out["landform"][has] == 1).all() and (out["pattern"][has] == 3280).all()
    assert np.abs(out["positive"][has].astype(np.float64) - math.pi / 2).max() < 1e-6  # float32 of pi / 2
    tmax, tmin = R.extremes(dem, 10.0, radius)
    pos = sum(R.HALF_PI - np.arctan(tmax[d]) for d in range(8)) / 8.0
    neg = sum(R.HALF_PI + np.arctan(tmin[d]) for d in range(8)) / 8.0
    assert np.abs(pos[has] - math.pi / 2).max() <= 1e-12 and np.abs(neg[has] - math.pi / 2).max() <= 1e-12
    assert (out["positive"][has] == np.float32(math.pi / 2)).all()
    assert (out["negative"][has] == np.float32(math.pi / 2)).all()
    assert (out["sky_view"][has] == 1).all()
    assert (out["pattern"][~has] == 65535).all() and (out["sky_view"][~has] == -100).all()


CURL = 0.01
UP = (NE, E, SE)


def _inner(shape):
    inner = np.zeros(shape, bool)
    inner[2:-2, 2:-2] = True  # two samples or more in every direction
    return inner


def _assert_rising(dem, px, radius, dirs, where):
    """the tangents of these directions grow along the ray: tmax > tmin > T, no tie"""
    tmax, tmin = R.extremes(dem, px, radius)
    for d in dirs:
        assert (tmax[d][where] > tmin[d][where]).all() and (tmin[d][where] > T1).all(), d


def test_a_tie_goes_to_minus_one():
    """one sample per direction (radius 1): a higher neighbour and a lower neighbour both read -1, a level one 0"""
    dem = np.full((3, 3), 100, np.float32)
    dem[1, 2], dem[1, 0] = 130, 70
    dg, form, _ = _digits(dem, 10.0, 1)
    assert dg[E, 1, 1] == -1 and dg[W, 1, 1] == -1 and (dg[[N, NE, SE, S, SW, NW], 1, 1] == 0).all()
    assert form[1, 1] == R.TABLE[2, 0] == 1
    # with a second, lower sample behind the higher neighbour the direction reads +1
    dem = np.full((5, 5), 100, np.float32)
    dem[2, 3] = 130
    assert _digits(dem, 10.0, 2)[0][E, 2, 2] == 1


@pytest.mark.parametrize("radius", [2, 5, 12])
def test_plane_rising_to_the_east_is_slope(radius):
    shape = (2 * radius + 9, 2 * radius + 11)
    inner = _inner(shape)
    dem = R.plane_east(*shape, rise=0.7, curl=CURL)
    _assert_rising(dem, 10.0, radius, UP, inner)
    dg, form, _ = _digits(dem, 10.0, radius)
    for d in UP:
        assert (dg[d][inner] == 1).all(), d
    for d in (SW, W, NW):
        assert (dg[d][inner] == -1).all(), d
    for d in (N, S):
        assert (dg[d][inner] == 0).all(), d
    assert (form[inner] == 6).all()
    # the exactly straight ramp: down-slope -1, level 0; up-slope a tie or a last-bit win, never 0
    dg, form, _ = _digits(R.plane_east(*shape, rise=0.7), 10.0, radius)
    for d in (SW, W, NW):
        assert (dg[d][inner] == -1).all(), d
    for d in (N, S):
        assert (dg[d][inner] == 0).all(), d
    for d in UP:
        assert (dg[d][inner] != 0).all(), d
    assert (form[inner][(dg[list(UP)][:, inner] == 1).all(axis=0)] == 6).all()


@pytest.mark.parametrize("radius", [2, 5, 12])
def test_cone_apex_is_peak_and_inverted_cone_apex_is_pit(radius):
    n = 2 * radius + 5
    c = n // 2
    for curl in (0.0, CURL):
        dg, form, _ = _digits(R.cone(n, rise=0.7, curl=curl), 10.0, radius)
        assert (dg[:, c, c] == -1).all() and form[c, c] == 2
    pit = (np.float32(200) - R.cone(n, rise=0.7, curl=CURL)).astype(np.float32)
    apex = np.zeros((n, n), bool)
    apex[c, c] = True
    _assert_rising(pit, 10.0, radius, range(8), apex)
    dg, form, _ = _digits(pit, 10.0, radius)
    assert (dg[:, c, c] == 1).all() and form[c, c] == 10


@pytest.mark.parametrize("radius", [2, 5, 12])
def test_valley_axis_is_valley_and_ridge_crest_is_ridge(radius):
    rows, cols = 2 * radius + 7, 2 * radius + 5
    x = cols // 2
    axis = np.zeros((rows, cols), bool)
    axis[2:rows - 2, x] = True
    flanks, along = [NE, E, SE, SW, W, NW], [N, S]
    valley = R.valley_ns(rows, cols, rise=0.7, curl=CURL)
    _assert_rising(valley, 10.0, radius, flanks, axis)
    dg, form, _ = _digits(valley, 10.0, radius)
    assert (dg[flanks][:, axis] == 1).all() and (dg[along][:, axis] == 0).all()
    assert (form[axis] == 9).all()
    for curl in (0.0, CURL):
        ridge = (np.float32(300) - R.valley_ns(rows, cols, rise=0.7, curl=curl)).astype(np.float32)
        dg, form, _ = _digits(ridge, 10.0, radius)
        assert (dg[flanks][:, axis] == -1).all() and (dg[along][:, axis] == 0).all()
        assert (form[axis] == 3).all()


def test_openness_and_sky_view_of_a_pit_and_a_peak():
    """in a pit the horizon stands high: positive openness and the sky view are low, negative openness is above
    pi / 2; on a peak it is the other way round"""
    n, c = 25, 12
    cone = R.cone(n, rise=5.0)
    peak = R.attributes(cone, 10.0, T1, R.OUTPUTS, 10)
    pit = R.attributes((np.float32(200) - cone).astype(np.float32), 10.0, T1, R.OUTPUTS, 10)
    assert peak["sky_view"][c, c] == 1 and 0 < pit["sky_view"][c, c] < 0.6
    assert peak["positive"][c, c] > math.pi / 2 > pit["positive"][c, c] > 0
    assert pit["negative"][c, c] > math.pi / 2 > peak["negative"][c, c] > 0
    # a slope of 0.5 all round: the horizon angle is atan(0.5), its sine 0.5 / sqrt(1.25)
    assert abs(pit["sky_view"][c, c] - (1 - 0.5 / math.sqrt(1.25))) < 1e-3
    assert abs(pit["positive"][c, c] - (math.pi / 2 - math.atan(0.5))) < 1e-3


# ---- which cells have a value -------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 3), (1, 37), (4, 9), (7, 8), (12, 15)])
@pytest.mark.parametrize("radius,skip", [(1, 0), (3, 0), (3, 1), (3, 2), (8, 0), (8, 7)])
def test_valued_cell_count_on_an_all_valid_raster(shape, radius, skip):
    H, W = shape
    dem = np.random.default_rng(H * 100 + W).uniform(10, 400, shape).astype(np.float32)
    out = R.attributes(dem, 7.3, T1, R.OUTPUTS, radius, skip)
    want = max(H - 2 * (skip + 1), 0) * max(W - 2 * (skip + 1), 0)
    for k in R.OUTPUTS:
        none = {"landform": 0, "pattern": 65535}.get(k, -100)
        assert (out[k] != none).sum() == want, k
    has = np.zeros(shape, bool)
    if want:
        has[skip + 1:H - skip - 1, skip + 1:W - skip - 1] = True
    assert np.array_equal(out["landform"] != 0, has)
    assert out["landform"].dtype == np.uint8 and out["pattern"].dtype == np.uint16
    assert out["positive"].dtype == out["negative"].dtype == out["sky_view"].dtype == np.float32


def test_nodata_in_a_line_of_sight_is_skipped_not_a_stop():
    base = np.full((9, 9), 100, np.float32)
    base[4, 6] = 110  # two cells east of the centre
    clean = _digits(base, 10.0, 4)
    assert clean[0][E, 4, 4] == 1 and clean[1][4, 4] != 0
    for hole in (np.float32(-100), np.float32("nan"), np.float32("inf"), np.float32(-500)):
        dem = base.copy()
        dem[4, 5] = hole  # the cell between them
        dg, form, pat = _digits(dem, 10.0, 4)
        assert form[4, 4] != 0 and dg[E, 4, 4] == 1, hole
        assert pat[4, 4] == clean[2][4, 4] and form[4, 4] == clean[1][4, 4]
        assert form[4, 5] == 0 and pat[4, 5] == 65535  # the hole itself has no value
    # a direction whose every sample is invalid: no value
    dem = base.copy()
    dem[4, 5:] = -100
    assert _digits(dem, 10.0, 4)[1][4, 4] == 0
    # ... but one valid sample at the end of the line is enough
    dem[4, 8] = 100
    assert _digits(dem, 10.0, 4)[1][4, 4] != 0
    assert _digits(dem, 10.0, 3)[1][4, 4] == 0  # out of reach at radius 3


def test_skip_leaves_the_nearest_cells_out():
    dem = np.full((11, 11), 100, np.float32)
    dem[5, 6] = 150  # next to the centre, east
    assert _digits(dem, 10.0, 4, skip=0)[0][E, 5, 5] == 1
    assert _digits(dem, 10.0, 4, skip=1)[0][E, 5, 5] == 0
    assert _digits(dem, 10.0, 4, skip=1)[1][5, 5] == 1


def test_flat_threshold():
    dem = R.plane_east(9, 9, rise=1.0, curl=CURL)  # 0.1 east-west at px 10: 5.7 degrees
    assert _digits(dem, 10.0, 3, T=R.flat_tangent(1.0))[1][4, 4] == 6
    assert _digits(dem, 10.0, 3, T=R.flat_tangent(30.0))[1][4, 4] == 1
    assert _digits(dem, 10.0, 3, T=R.flat_tangent(30.0))[2][4, 4] == 3280


# ---- the public interface ------------------------------------------------------------------------------------------
def test_alias_module_and_constants():
    import descriptools.horizon
    assert descriptools.horizon.attributes is horizon.attributes
    assert descriptools.horizon.OUTPUTS == horizon.OUTPUTS == R.OUTPUTS
    assert horizon.OUTPUTS == ("landform", "pattern", "positive", "negative", "sky_view")
    assert horizon.RADIUS_MAX == 64
    assert sorted(horizon.LANDFORMS) == list(range(1, 11))
    for word in ("1.4142135623730951", "skip + 1", "65535", "'over'", "'under'"):
        assert word in horizon.__doc__, word


def test_source_is_in_the_build():
    from descriptools_amd import build
    assert "dt_horizon.hip" in build.SOURCES


DEM = np.zeros((6, 7), np.float32)


@pytest.mark.parametrize("call", [
    lambda: horizon.attributes(np.zeros(5, np.float32), 10.0),                       # not 2-D
    lambda: horizon.attributes(np.zeros((2, 3, 4), np.float32), 10.0),
    lambda: horizon.attributes(np.array([[0.1, 0.2]], np.float64), 10.0),            # float32 cannot hold it
    lambda: horizon.attributes(np.array([[2 ** 24 + 1]], np.int64), 10.0),
    lambda: horizon.attributes(DEM, 0.0),
    lambda: horizon.attributes(DEM, float("nan")),
    lambda: horizon.attributes(DEM, True),
    lambda: horizon.attributes(DEM, 10.0, radius=0),
    lambda: horizon.attributes(DEM, 10.0, radius=65),
    lambda: horizon.attributes(DEM, 10.0, radius=1.5),
    lambda: horizon.attributes(DEM, 10.0, radius=True),
    lambda: horizon.attributes(DEM, 10.0, radius=-3),
    lambda: horizon.attributes(DEM, 10.0, radius=None),
    lambda: horizon.attributes(DEM, 10.0, radius=4, skip=4),
    lambda: horizon.attributes(DEM, 10.0, radius=4, skip=9),
    lambda: horizon.attributes(DEM, 10.0, radius=4, skip=-1),
    lambda: horizon.attributes(DEM, 10.0, radius=4, skip=1.0),
    lambda: horizon.attributes(DEM, 10.0, radius=4, skip=True),
    lambda: horizon.attributes(DEM, 10.0, radius=1, skip=1),
    lambda: horizon.attributes(DEM, 10.0, flat=90),
    lambda: horizon.attributes(DEM, 10.0, flat=float("nan")),
    lambda: horizon.attributes(DEM, 10.0, flat=-1.0),
    lambda: horizon.attributes(DEM, 10.0, flat="flat"),
    lambda: horizon.attributes(DEM, 10.0, outputs=()),
    lambda: horizon.attributes(DEM, 10.0, outputs=[]),
    lambda: horizon.attributes(DEM, 10.0, outputs="landform"),
    lambda: horizon.attributes(DEM, 10.0, outputs=None),
    lambda: horizon.attributes(DEM, 10.0, outputs=("landform", "landform")),
    lambda: horizon.attributes(DEM, 10.0, outputs=("landform", "openness")),
    lambda: horizon.attributes(DEM, 10.0, outputs=("sky_view", 3)),
    lambda: horizon.geomorphons(DEM, 10.0, radius=65),
    lambda: horizon.geomorphons(DEM, 10.0, 10, 10),
    lambda: horizon.geomorphons(DEM, 10.0, flat=90.0),
    lambda: horizon.geomorphons(np.array([[0.1]], np.float64), 10.0),
    lambda: horizon.openness(DEM, 10.0, kind="both"),
    lambda: horizon.openness(DEM, 10.0, kind=None),
    lambda: horizon.openness(DEM, 10.0, radius=0),
    lambda: horizon.openness(DEM, -1.0),
    lambda: horizon.sky_view(DEM, 10.0, radius=2.0),
    lambda: horizon.sky_view(DEM, 10.0, 3, 3),
])
def test_bad_arguments_raise_value_error(call, monkeypatch):
    from descriptools_amd import _lib

    def no_library():
        raise AssertionError("the library was reached before the arguments were checked")
    monkeypatch.setattr(_lib, "lib", no_library)
    with pytest.raises(ValueError):
        call()


def test_too_many_cells_is_refused():
    big = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 16, 2 ** 15), (0, 0))
    with pytest.raises(ValueError, match="2\\^31"):
        horizon.attributes(big, 10.0)
