"""GPU (-m gpu): descriptools_amd.morphology (dt_morph_reconstruct, dt_dev_morph_reconstruct, k_mo_* in
dt_morphology.hip) against tests/_morphology_ref.py.  Every comparison is on bit patterns, dtype and shape included.
Trivial shapes; ragged tiles (65 x 63: 2 x 1 tiles of 64 x 64; 130 x 257: 3 x 5 tiles, every colour and an interior tile)
with uniform, rounded (plateaus, exact ties) and nodata-ridden fields, both kinds, both connectivities, and a visit limit
of 1; -0.0 beside +0.0; a serpentine through all nine tiles of 192 x 192, which shows that the multi-round path ran; a
spiral inside one tile, which shows the repeat-until-quiet loop of a visit; the fill against the priority flood, against
flowdir.d8_conditioned and with chosen outlets; h-minima / h-maxima; the regional extrema against the plateau labelling;
opening / closing by reconstruction against reconstruct(filters.minimum / maximum); the binary cross-check against
regions.connected; the device tier and its budget; the C entry between guard bands.  A case is kept from being vacuous
by a condition on its REFERENCE: at least 10 % of the valid cells have R != F0."""
import functools

import numpy as np
import pytest

import _morphology_ref as R

pytestmark = pytest.mark.gpu

TILE = 64  # MO_T of csrc/dt_morphology.hip
SEED = 7
KINDS = ("dilation", "erosion")
MARKER, SHIFT, STEP, OUTLETS, WINDOW = range(5)  # DT_MORPH_*


def _same(name, g, r):
    g, r = np.asarray(g), np.asarray(r)
    assert g.dtype == r.dtype, "%s: dtype %s, reference %s" % (name, g.dtype, r.dtype)
    assert g.shape == r.shape, "%s: shape %s, reference %s" % (name, g.shape, r.shape)
    gb = g.view(np.uint32) if g.dtype == np.float32 else g
    rb = r.view(np.uint32) if r.dtype == np.float32 else r
    if not np.array_equal(gb, rb):
        bad = np.argwhere(gb != rb)
        i = tuple(bad[0])
        raise AssertionError("%s: %d cells differ, first at %s: got %r, reference %r" % (name, len(bad), i, g[i], r[i]))


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _tiles(shape):
    return -(-shape[0] // TILE) * -(-shape[1] // TILE)


@functools.lru_cache(maxsize=None)
def _case(shape, field):
    return _frozen(*R.random_case(shape, field, SEED))


@functools.lru_cache(maxsize=None)
def _random_ref(shape, field, kind, cn):
    """(marker, mask, reference, cells with R != F0, valid cells): computed once, shared, never written to"""
    marker, mask = _case(shape, field)
    ref = R.reconstruct(marker, mask, kind, cn)
    _frozen(ref)
    return marker, mask, ref, R.changed(marker, mask, kind, ref), int(R.valid(mask).sum())


@functools.lru_cache(maxsize=None)
def _serpentine_ref():
    marker, mask = R.serpentine(192)
    ref = R.reconstruct(marker, mask)
    return _frozen(marker, mask, ref)


@functools.lru_cache(maxsize=None)
def _void_dem(shape=(130, 257)):
    return _frozen(R.dem_with_voids(shape, SEED))[0]


def check(marker, mask, kind, cn, limit=0, ref=None):
    from descriptools_amd import morphology
    out = morphology.reconstruct(marker, mask, kind=kind, connectivity=cn, _visit_limit=limit)
    ref = R.reconstruct(marker, mask, kind, cn) if ref is None else ref
    _same("reconstruct %s/%d limit %d" % (kind, cn, limit), out, ref)
    assert isinstance(out, morphology.Reconstruction) and set(out.info) == {"rounds", "changed", "tile_visits"}
    assert out.info["changed"] == R.changed(marker, mask, kind, ref)
    assert out.info["tile_visits"] >= _tiles(np.shape(mask))
    return out


# ---- trivial shapes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_one_cell(kind):
    out = check(np.float32([[7.0]]), np.float32([[5.0]]), kind, 8)
    assert out.info["rounds"] == 0 and out.info["tile_visits"] == 1 and out.info["changed"] == 0
    out = check(np.float32([[np.nan]]), np.float32([[5.0]]), kind, 8)
    assert out[0, 0] == -100 and out.info["rounds"] == 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("shape", ((1, 200), (200, 1)))
def test_lines_cut_by_an_invalid_cell(shape, kind):
    rng = np.random.default_rng(SEED)
    mask = rng.uniform(1, 9, shape).astype(np.float32)
    marker = np.full(shape, np.nan, np.float32)
    marker.reshape(-1)[3] = 5.0
    mask.reshape(-1)[120] = -100.0  # cuts the line: nothing beyond it is reached
    for cn in (8, 4):
        out = check(marker, mask, kind, cn)
        assert (out.reshape(-1)[120:] == -100).all() and (out.reshape(-1)[:120] != -100).all()


def test_all_invalid_and_empty_rasters():
    from descriptools_amd import morphology as M
    for v in (-100.0, np.nan, np.inf, -np.inf, -9999.0):
        mask = np.full((70, 5), v, np.float32)
        out = check(np.ones((70, 5), np.float32), mask, "dilation", 8)
        assert (out == -100).all() and out.info["rounds"] == 0 and out.info["changed"] == 0
        assert not M.regional_minima(mask).any() and (M.fill(mask) == -100).all()
    for shape in ((0, 0), (0, 9), (9, 0)):
        e = np.zeros(shape, np.float32)
        for out in (M.reconstruct(e, e), M.fill(e), M.hminima(e, 1.0), M.hmaxima(e, 1.0),
                    M.opening_by_reconstruction(e, 2), M.closing_by_reconstruction(e, 2)):
            assert out.shape == shape and out.dtype == np.float32
        assert M.reconstruct(e, e).info == {"rounds": 0, "changed": 0, "tile_visits": 0}
        assert M.regional_minima(e).shape == shape and M.regional_maxima(e).dtype == np.uint8


# ---- ragged tiles ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", (8, 4))
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("field", R.FIELDS)
@pytest.mark.parametrize("shape", ((65, 63), (130, 257)))
def test_random_fields_on_ragged_tiles(shape, field, kind, cn):
    marker, mask, ref, changed, n_valid = _random_ref(shape, field, kind, cn)
    assert changed >= 0.10 * n_valid, "the case is vacuous: %d of %d valid cells change" % (changed, n_valid)
    for limit in (0, 1):
        out = check(marker, mask, kind, cn, limit, ref)
        assert out.info["rounds"] >= 1


def test_signs_of_zero():
    """-0.0 is below +0.0 in the key order: the output carries the bit pattern the order selects"""
    pz, nz = np.float32(0.0), np.float32(-0.0)
    mask = np.array([[pz, nz, pz, nz, pz, pz]], np.float32)
    marker = np.array([[pz, np.nan, np.nan, np.nan, np.nan, nz]], np.float32)
    for kind in KINDS:
        for cn in (8, 4):
            out = check(marker, mask, kind, cn)
            want = [0, 1, 1, 1, 1, 1] if kind == "dilation" else [0, 0, 0, 0, 0, 0]
            # dilation: +0.0 passes the -0.0 cell as -0.0 and stays -0.0 (min of the path); from the right -0.0 arrives.
            # erosion: +0.0 is above -0.0, so max(mask, .) along the path is +0.0 everywhere it passes
            assert np.signbit(np.asarray(out)).astype(int).tolist() == [want], (kind, cn, out)
    from descriptools_amd import morphology as M
    z = np.array([[pz, nz, pz], [pz, pz, pz]], np.float32)
    assert M.regional_minima(z).tolist() == [[0, 1, 0], [0, 0, 0]]
    assert M.regional_maxima(-z).tolist() == [[0, 1, 0], [0, 0, 0]]


# ---- many rounds, and many sweeps within a visit --------------------------------------------------------------------
@pytest.mark.parametrize("limit", (0, 1))
def test_serpentine_winds_through_every_tile(limit):
    marker, mask, ref = _serpentine_ref()
    assert (ref[mask == 10] == 10).all() and (ref[mask == 1] == 1).all()
    out = check(marker, mask, "dilation", 8, limit, ref)
    assert out.info["rounds"] > 1 and out.info["tile_visits"] > 9
    if limit == 0:
        out4 = check(marker, mask, "dilation", 4, 0)
        assert out4.info["rounds"] > 1
        # the same path by erosion: the negated rasters
        check(np.negative(marker), np.negative(mask), "erosion", 8)


def test_spiral_inside_one_tile():
    marker, mask = R.spiral(64)
    ref, sweeps = R.jacobi(marker, mask)
    assert sweeps > 1500 and (ref[mask == 10] == 10).all()
    out = check(marker, mask, "dilation", 8, 0, ref)
    # one tile: nothing can come in from outside, so its single visit iterated to the end
    assert out.info["rounds"] == 1 and out.info["tile_visits"] == 1
    out = check(marker, mask, "dilation", 8, 1, ref)
    assert out.info["rounds"] > 1 and out.info["tile_visits"] == out.info["rounds"] + 1


# ---- fill -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", (8, 4))
def test_fill_equals_the_priority_flood(cn):
    from descriptools_amd import morphology as M
    dem = _void_dem()
    ref = R.priority_flood(dem, cn=cn)
    ok = R.valid(dem)
    assert (ref[ok] > dem[ok]).mean() >= 0.10
    out = M.fill(dem, connectivity=cn)
    _same("fill/%d" % cn, out, ref)
    assert out.info["changed"] == int((ok & ~R.default_outlets(dem)).sum())


def test_fill_equals_the_conditioning_fill():
    from descriptools_amd import flowdir, morphology as M
    dem = _void_dem()
    ok = R.valid(dem)
    filled = flowdir.d8_conditioned(np.where(ok, dem, np.float32(-100)), 10.0, return_filled=True)[1]
    out = np.asarray(M.fill(dem))
    assert filled.dtype == np.float32 and np.array_equal(out[ok], filled[ok])


def test_fill_towards_chosen_outlets():
    from descriptools_amd import morphology as M
    dem = np.array(_void_dem((100, 150)))
    dem[R.valid(dem) == 0] = 20.0            # no voids but the ones placed here
    dem[40:61, 40] = dem[40:61, 60] = dem[40, 40:61] = dem[60, 40:61] = np.nan   # a basin without outlets
    dem[80, 100] = -9999.0                   # a one-cell void in the plain
    seeds = np.zeros(dem.shape, np.int16)
    seeds[0, :] = 3
    seeds[50, 40] = 1                        # a seed on an invalid cell seeds nothing
    for cn in (8, 4):
        ref = R.priority_flood(dem, seeds, cn)
        out = M.fill(dem, outlets=seeds, connectivity=cn)
        _same("seeded fill/%d" % cn, out, ref)
        assert (np.asarray(out)[41:60, 41:60] == -100).all()
        # the void is no outlet any more: with the default rule its neighbours keep their heights, now some are filled
        free = np.asarray(M.fill(dem, connectivity=cn))
        ring = R.valid(dem[79:82, 99:102])
        assert (free[79:82, 99:102][ring] == dem[79:82, 99:102][ring]).all()
        assert (ref[79:82, 99:102][ring] > dem[79:82, 99:102][ring]).any()
        reached = ref != -100
        assert (ref[reached] >= free[reached]).all()
    _same("bool outlets", M.fill(dem, outlets=seeds != 0), R.priority_flood(dem, seeds, 8))


# ---- h-minima / h-maxima --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", (8, 4))
def test_h_extrema_equal_the_reference(cn):
    from descriptools_amd import morphology as M
    _, dem = _case((130, 257), "nodata")
    for h in (0.5, 7.25):
        lo = R.h_extrema(dem, h, False, cn)
        assert (lo != dem)[R.valid(dem)].mean() >= 0.10
        _same("hminima", M.hminima(dem, h, connectivity=cn), lo)
        _same("hmaxima", M.hmaxima(dem, h, connectivity=cn), R.h_extrema(dem, h, True, cn))


def test_h_minima_removes_the_pit_under_h_and_keeps_the_one_over_it():
    from descriptools_amd import morphology as M
    z = np.full((70, 140), 10.0, np.float32)
    under = np.nextafter(np.float32(9.5), np.float32(10))   # depth just under 0.5
    over = np.nextafter(np.float32(9.5), np.float32(9))     # depth just over 0.5
    z[10, 10], z[30, 100], z[66, 130] = under, over, 5.0
    out = M.hminima(z, 0.5)
    _same("hminima", out, R.h_extrema(z, 0.5, False))
    assert out[10, 10] == 10.0
    assert out[30, 100] == np.float32(np.float64(over) + 0.5) and out[30, 100] < 10.0
    assert out[66, 130] == 5.5
    keep = np.ones(z.shape, bool)
    keep[10, 10] = keep[30, 100] = keep[66, 130] = False
    assert (np.asarray(out)[keep] == 10.0).all()
    top = M.hmaxima(-z, 0.5)
    _same("hmaxima", top, R.h_extrema(-z, 0.5, True))
    assert top[10, 10] == -10.0 and top[30, 100] == -out[30, 100] and top[66, 130] == -5.5


def test_h_maxima_floor_near_the_sentinel():
    from descriptools_amd import morphology as M
    rng = np.random.default_rng(SEED)
    z = rng.uniform(-99.99, -90.0, (66, 70)).astype(np.float32)
    z[:, :30] = rng.uniform(-99.99, -98.5, (66, 30)).astype(np.float32)  # every marker here is the floor ...
    z[:, 30] = -100.0                                                     # ... and nothing higher comes in
    ref = R.h_extrema(z, 2.0, True)
    assert (ref[:, :30] == R.FLOOR).all()
    assert (ref > R.FLOOR).any() and (ref[R.valid(z)] > -100).all() and (ref[:, 30] == -100).all()
    _same("hmaxima at the floor", M.hmaxima(z, 2.0), ref)
    big = np.full((3, 3), 3e38, np.float32)  # z + h overflows to +inf: given all the same, clamped by the mask's dual
    _same("hminima overflow", M.hminima(big, 3e38), R.h_extrema(big, 3e38, False))


# ---- regional extrema -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", (8, 4))
def test_regional_extrema_equal_the_plateau_labelling(cn):
    from descriptools_amd import morphology as M
    _, dem = _case((130, 257), "nodata")
    dem = np.array(dem)
    dem[60:68, 60:70] = 1.0      # a plateau split by a tile seam (rows and columns 63 | 64): a minimum
    dem[0:3, 100:140] = 1.0      # a plateau on the raster's edge and across a seam: a minimum
    dem[100, 10:150] = 2.0       # a plateau through three tiles with one lower cell at its far end: no minimum
    dem[100, 150] = 1.5
    for maxima in (False, True):
        z = np.where(R.valid(dem), -dem, np.float32(np.nan)) if maxima else dem  # (-(-9999) would be a valid height)
        ref = R.regional(z, maxima, cn)
        assert ref[60:68, 60:70].all() and ref[0:3, 100:140].all()
        assert not ref[100, 10:150].any() and ref[100, 150] == 1
        got = (M.regional_maxima if maxima else M.regional_minima)(z, connectivity=cn)
        _same("regional %s/%d" % ("maxima" if maxima else "minima", cn), got, ref)


# ---- opening / closing by reconstruction ----------------------------------------------------------------------------
@pytest.mark.parametrize("radius", (1, 70))
def test_by_reconstruction_equals_reconstruct_of_the_window_extreme(radius):
    from descriptools_amd import filters, morphology as M
    _, dem = _case((130, 257), "nodata")
    for cn in (8, 4):
        want = M.reconstruct(filters.minimum(dem, radius), dem, connectivity=cn)
        got = M.opening_by_reconstruction(dem, radius, connectivity=cn)
        _same("opening", got, np.asarray(want))
        assert got.info["changed"] == want.info["changed"]
        want = M.reconstruct(filters.maximum(dem, radius), dem, kind="erosion", connectivity=cn)
        _same("closing", M.closing_by_reconstruction(dem, radius, connectivity=cn), np.asarray(want))
    ok = R.valid(dem)
    assert (np.asarray(want) != dem)[ok].mean() >= 0.10
    _same("opening against the reference", M.opening_by_reconstruction(dem, radius),
          R.reconstruct(filters.minimum(dem, radius), dem))


def test_opening_removes_a_building_and_keeps_the_slope():
    from descriptools_amd import morphology as M
    H, W = 70, 140
    dem = np.broadcast_to(np.float32(0.25) * np.arange(W, dtype=np.float32), (H, W)).copy()
    dem[20:25, 60:65] += np.float32(8.0)   # 5 cells wide on a slope that rises to the east
    out = np.asarray(M.opening_by_reconstruction(dem, 3))
    away = np.ones(dem.shape, bool)
    away[20:25, 60:65] = False
    away[:, W - 3:] = False                # the top of the slope is an object narrower than the window too
    assert np.array_equal(out[away].view(np.uint32), dem[away].view(np.uint32))
    assert (out[20:25, 60:65] == dem[0, 65]).all()   # the highest ground beside it
    assert (out[:, W - 3:] == dem[0, W - 4]).all()
    # closing: a 5-cell pit is closed, the slope keeps its bits but for its foot
    pit = np.broadcast_to(np.float32(0.25) * np.arange(W, dtype=np.float32), (H, W)).copy()
    pit[20:25, 60:65] -= np.float32(8.0)
    out = np.asarray(M.closing_by_reconstruction(pit, 3))
    away[:, W - 3:] = True
    away[:, :3] = False
    assert np.array_equal(out[away].view(np.uint32), pit[away].view(np.uint32))
    assert (out[20:25, 60:65] == pit[0, 59]).all() and (out[:, :3] == pit[0, 3]).all()


# ---- binary cross-check ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cn", (8, 4))
def test_binary_reconstruction_is_regions_connected(cn):
    from descriptools_amd import morphology as M, regions
    rng = np.random.default_rng(SEED)
    mask = rng.random((130, 257)) < (0.40 if cn == 8 else 0.58)  # just under the percolation thresholds
    seeds = rng.random(mask.shape) < 0.002
    keep = regions.connected(mask, seeds, connectivity=cn)
    assert 0.1 * mask.sum() < keep.sum() < 0.9 * mask.sum()
    out = M.reconstruct((seeds & mask).astype(np.float32), mask.astype(np.float32), connectivity=cn)
    _same("binary", out, keep.astype(np.float32))


# ---- the device tier ------------------------------------------------------------------------------------------------
def _dev(ctx, mode, erosion, cn, mask, marker=None, seeds=None, h=0.0, radius=0, limit=0, rounds=4096, u8=False):
    """dt_dev_morph_reconstruct on resident rasters -> (output, status bits)"""
    from descriptools_amd import _lib
    H, W = mask.shape
    held = [ctx.to_device(np.ascontiguousarray(mask, np.float32))]
    d_marker = d_seeds = None
    if marker is not None:
        d_marker = ctx.to_device(np.ascontiguousarray(marker, np.float32))
        held.append(d_marker)
    if seeds is not None:
        d_seeds = ctx.to_device(np.ascontiguousarray(seeds != 0, np.uint8))
        held.append(d_seeds)
    d_out = ctx.empty((H, W), np.uint8 if u8 else np.float32)
    held.append(d_out)
    try:
        _lib.check(_lib.lib().dt_dev_morph_reconstruct(
            ctx.h, mode, erosion, cn, held[0].ptr, d_marker.ptr if d_marker else None,
            d_seeds.ptr if d_seeds else None, h, radius, H, W, limit, rounds, None if u8 else d_out.ptr,
            d_out.ptr if u8 else None))
        st = ctx.status()
        return d_out.to_host(), st
    finally:
        for d in held:
            d.free()


def test_device_tier_equals_the_host_tier():
    from descriptools_amd import morphology as M
    from descriptools_amd.device import Context
    marker, dem = _case((130, 257), "nodata")
    seeds = np.zeros(dem.shape, np.uint8)
    seeds[:, 0] = 1
    ctx = Context()
    try:
        for kind in KINDS:
            for cn in (8, 4):
                out, st = _dev(ctx, MARKER, int(kind == "erosion"), cn, dem, marker=marker)
                assert st == 0
                _same("reconstruct", out, _random_ref((130, 257), "nodata", kind, cn)[2])
        for got, want in ((_dev(ctx, OUTLETS, 1, 8, dem), M.fill(dem)),
                          (_dev(ctx, OUTLETS, 1, 4, dem, seeds=seeds), M.fill(dem, outlets=seeds, connectivity=4)),
                          (_dev(ctx, SHIFT, 1, 8, dem, h=0.5), M.hminima(dem, 0.5)),
                          (_dev(ctx, SHIFT, 0, 8, dem, h=0.5, limit=1), M.hmaxima(dem, 0.5)),
                          (_dev(ctx, STEP, 1, 8, dem, u8=True), M.regional_minima(dem)),
                          (_dev(ctx, STEP, 0, 4, dem, u8=True), M.regional_maxima(dem, connectivity=4)),
                          (_dev(ctx, WINDOW, 0, 8, dem, radius=5), M.opening_by_reconstruction(dem, 5)),
                          (_dev(ctx, WINDOW, 1, 8, dem, radius=5), M.closing_by_reconstruction(dem, 5))):
            assert got[1] == 0
            _same("device tier", got[0], np.asarray(want))
    finally:
        ctx.close()


def test_device_tier_budget_and_refusals():
    from descriptools_amd import _lib
    from descriptools_amd.device import Context
    marker, mask, ref = _serpentine_ref()
    L = _lib.lib()
    ctx = Context()
    try:
        out, st = _dev(ctx, MARKER, 0, 8, mask, marker=marker, rounds=1)
        assert st == 2, "DT_STATUS_NOT_CONVERGED"
        out, st = _dev(ctx, MARKER, 0, 8, mask, marker=marker, rounds=4096)
        assert st == 0
        _same("serpentine", out, ref)
        call = L.dt_dev_morph_reconstruct
        for rounds in (0, -1, 4097):
            assert call(ctx.h, 0, 0, 8, None, None, None, 0.0, 0, 4, 4, 0, rounds, None, None) == -1
            assert b"rounds" in L.dt_last_error()
        assert call(ctx.h, 0, 0, 8, None, None, None, 0.0, 0, 0, 7, 0, 1, None, None) == 0
        assert call(ctx.h, 0, 0, 8, None, None, None, 0.0, 0, 4, 4, 0, 1, None, None) == -1
        assert b"exactly one of out and out8" in L.dt_last_error()
        assert call(ctx.h, 0, 0, 8, None, None, None, 0.0, 0, 1 << 16, 1 << 15, 0, 1, None, None) == -1
        assert b"2^31" in L.dt_last_error()
        for args, word in (((5, 0, 8, 0.0, 0, 0), b"mode"), ((-1, 0, 8, 0.0, 0, 0), b"mode"),
                           ((0, 2, 8, 0.0, 0, 0), b"erosion"), ((0, 0, 6, 0.0, 0, 0), b"connectivity"),
                           ((1, 0, 8, 0.0, 0, 0), b"h must"), ((1, 0, 8, float("nan"), 0, 0), b"h must"),
                           ((4, 0, 8, 0.0, 0, 0), b"radius"), ((4, 0, 8, 0.0, 4097, 0), b"radius"),
                           ((0, 0, 8, 0.0, 0, -1), b"visit_limit")):
            mode, erosion, cn, h, radius, limit = args
            assert call(ctx.h, mode, erosion, cn, None, None, None, h, radius, 0, 0, limit, 1, None, None) == -1
            assert word in L.dt_last_error(), args
        d = ctx.to_device(np.ones((4, 4), np.float32))
        e = ctx.empty((4, 4), np.float32)
        try:
            assert call(ctx.h, 0, 0, 8, d.ptr, None, None, 0.0, 0, 4, 4, 0, 1, e.ptr, None) == -1
            assert L.dt_last_error() == b"invalid argument: NULL raster"
            assert call(ctx.h, 0, 0, 8, d.ptr, e.ptr, None, 0.0, 0, 4, 4, 0, 1, d.ptr, None) == -1
            assert b"neither mask nor marker" in L.dt_last_error()
        finally:
            d.free()
            e.free()
        assert ctx.status() == 0
    finally:
        ctx.close()


# ---- the host-tier C entry itself -----------------------------------------------------------------------------------
def test_c_entry_with_null_outputs_between_guard_bands():
    from descriptools_amd import _lib, morphology as M
    marker, mask = _case((65, 63), "nodata")
    marker, mask = np.ascontiguousarray(marker), np.ascontiguousarray(mask)
    H, W = mask.shape
    GUARD = 4096
    want = M.reconstruct(marker, mask)

    def guarded(dtype):
        raw = np.full(2 * GUARD + H * W * np.dtype(dtype).itemsize, 0xA5, np.uint8)
        return raw, raw[GUARD:raw.size - GUARD].view(dtype).reshape(H, W)

    L = _lib.lib()
    p = _lib.ptr
    f32, u8, i64 = _lib.c_f32p, _lib.c_u8p, _lib.c_i64p
    call = L.dt_morph_reconstruct
    for with_info in (True, False):
        raw, out = guarded(np.float32)
        info = np.full(4, -1, np.int64)
        _lib.check(call(MARKER, 0, 8, p(mask, f32), p(marker, f32), None, 0.0, 0, H, W, 0, p(out, f32), None,
                        p(info, i64) if with_info else None))
        _same("float output", out, np.asarray(want))
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
        if with_info:
            assert info[0] >= 1 and info[1] == want.info["changed"] and info[2] >= 2 and info[3] == 0
    # the uint8 output: the keys stay in the scratch; marker, seeds and info4 NULL
    raw, out8 = guarded(np.uint8)
    _lib.check(call(STEP, 1, 8, p(mask, f32), None, None, 0.0, 0, H, W, 0, None, p(out8, u8), None))
    _same("uint8 output", out8, M.regional_minima(mask))
    assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
    # the modes that take no marker raster, with marker and seeds NULL
    for mode, erosion, h, radius, ref in ((SHIFT, 1, 0.5, 0, M.hminima(mask, 0.5)), (OUTLETS, 1, 0.0, 0, M.fill(mask)),
                                          (WINDOW, 0, 0.0, 2, M.opening_by_reconstruction(mask, 2))):
        raw, out = guarded(np.float32)
        _lib.check(call(mode, erosion, 8, p(mask, f32), None, None, h, radius, H, W, 0, p(out, f32), None, None))
        _same("mode %d" % mode, out, np.asarray(ref))
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
    # refusals of the entry itself
    raw, out = guarded(np.float32)
    info = np.full(4, -1, np.int64)
    assert call(MARKER, 0, 8, p(mask, f32), None, None, 0.0, 0, H, W, 0, p(out, f32), None, None) == -1
    assert L.dt_last_error() == b"invalid argument: NULL raster"
    assert call(MARKER, 0, 8, None, p(marker, f32), None, 0.0, 0, H, W, 0, p(out, f32), None, None) == -1
    assert call(MARKER, 0, 8, p(mask, f32), p(marker, f32), None, 0.0, 0, H, W, 0, None, None, None) == -1
    assert call(MARKER, 0, 8, p(mask, f32), p(marker, f32), None, 0.0, 0, H, W, 0, p(out, f32), p(out8, u8), None) == -1
    assert call(MARKER, 0, 5, p(mask, f32), p(marker, f32), None, 0.0, 0, H, W, 0, p(out, f32), None, None) == -1
    assert call(SHIFT, 0, 8, p(mask, f32), None, None, -1.0, 0, H, W, 0, p(out, f32), None, None) == -1
    assert call(WINDOW, 0, 8, p(mask, f32), None, None, 0.0, 0, H, W, 0, p(out, f32), None, None) == -1
    assert call(MARKER, 0, 8, p(mask, f32), p(marker, f32), None, 0.0, 0, H, W, -1, p(out, f32), None, None) == -1
    assert (raw == 0xA5).all()
    assert call(MARKER, 0, 8, None, None, None, 0.0, 0, 0, 9, 0, None, None, p(info, i64)) == 0
    assert list(info) == [0, 0, 0, 0]
    assert call(MARKER, 0, 8, None, None, None, 0.0, 0, 1 << 16, 1 << 15, 0, None, None, None) == -1
    assert b"2^31" in L.dt_last_error()
