"""GPU (-m gpu): harmonic.interpolate / fill_voids / base_level / vdcn (dt_harmonic, dt_dev_harmonic, k_hm_* in
dt_harmonic.hip) against the contract of descriptools_amd/harmonic.py: fixed cells exact, the residual of
tests/_harmonic_ref.py (the same expression) <= tol on every solved cell, the distance to the direct solve within
tol * max(t) (t: the hitting time, so that product is derived, not chosen), NaN on exactly the cells without a value,
the same bits on every run.  Equality with the reference is NOT asked: which iterate passes depends on the schedule.

Shapes are the smallest at which the paths differ: strips with two tile seams and three pyramid levels, 40 x 70 and
70 x 40 (a seam each way, two levels), 200 x 333 (4 x 6 tiles, every colour, interior tiles, four levels)."""
import numpy as np
import pytest

import _harmonic_ref as R

pytestmark = pytest.mark.gpu

TOL = 1e-5


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.int64)


def _check(got, v, fixed, dom, tol=TOL):
    """what every call must hold, against the reference's own sets; -> (reach, solved)"""
    u = got.field
    reach = R.reachable(fixed, dom)
    assert u.dtype == np.float64 and u.shape == v.shape
    assert np.array_equal(np.isnan(u), ~reach), "NaN exactly outside the domain and on the cells without a value"
    assert np.array_equal(_bits(u[fixed]), _bits(v[fixed].astype(np.float64))), "fixed cells carry their value"
    r = R.residual(np.where(reach, u, 0.0), fixed, reach)
    print("residual %.3g (info %.3g), rounds %s, tile visits %d" % (r.max(), got.info["residual"],
                                                                     got.info["rounds_per_level"],
                                                                     got.info["tile_visits"]))
    assert r.max() <= tol
    assert got.info["residual"] == r.max(), "the call reports the residual of the field it returns"
    assert got.info["converged"] and got.info["unreached"] == int((dom & ~reach).sum())
    assert got.info["levels"] == len(got.info["rounds_per_level"]) >= 1
    assert got.info["rounds_all"] == sum(got.info["rounds_per_level"]) and got.info["rounds"] >= 1
    return reach


# ---- 1. strips ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 130), (130, 1)])
def test_strip(shape):
    from descriptools_amd import harmonic
    v = np.zeros(130, np.float32)
    v[0], v[-1] = 2.0, 66.5
    fixed = np.zeros(130, bool)
    fixed[0] = fixed[-1] = True
    v, fixed = v.reshape(shape), fixed.reshape(shape)
    dom = np.ones(shape, bool)
    got = harmonic.interpolate(v, fixed.astype(np.int8), tol=TOL)
    _check(got, v, fixed, dom)
    tmax = R.hitting_time(fixed, dom).max()
    assert 129 ** 2 / 4 - 1 <= tmax <= 129 ** 2 / 4 + 1  # i (129 - i) at the middle of 128 free cells
    ramp = 2.0 + (66.5 - 2.0) * np.arange(130) / 129.0
    err = np.abs(got.field.reshape(-1) - ramp).max()
    print("error %.3g, bound %.3g" % (err, TOL * tmax))
    assert err <= TOL * tmax
    assert got.info["levels"] == 3


# ---- 2. a constant is exact -----------------------------------------------------------------------------------------
def test_constant_is_exact():
    from descriptools_amd import harmonic
    rng = np.random.default_rng(5)
    H, W = 70, 130
    dom = rng.random((H, W)) >= 0.10
    fixed = dom & (rng.random((H, W)) < 0.02)
    v = np.where(fixed, np.float32(37.5), np.float32(np.nan))
    got = harmonic.interpolate(v, fixed.astype(np.int8), dom.astype(np.int8), tol=TOL)
    reach = _check(got, v, fixed, dom)
    assert reach.sum() > 0.8 * H * W
    # sums of two, three and four copies of 37.5 and their quotients are exact: any deviation is a defect
    assert (got.field[reach] == 37.5).all()
    assert got.info["residual"] == 0.0


# ---- 3. against the direct solve ------------------------------------------------------------------------------------
def _random_case(shape, seed):
    rng = np.random.default_rng(seed)
    H, W = shape
    dom = rng.random((H, W)) >= 0.10
    # 5 x 5 cells of nodata, 62..66 along the long side and 0..4 along the short one: on the corner that the two tiles
    # share at the raster's edge (the corner of four tiles is in the 200 x 333 case)
    if H > W:
        dom[62:67, 0:5] = False
    else:
        dom[0:5, 62:67] = False
    fixed = dom & (rng.random((H, W)) < 0.02)
    v = np.where(fixed, rng.normal(200.0, 50.0, (H, W)), 0.0).astype(np.float32)
    return v, fixed, dom


_DIRECT = {}


def _direct(shape, seed):
    key = (shape, seed)
    if key not in _DIRECT:
        v, fixed, dom = _random_case(shape, seed)
        _DIRECT[key] = (v, fixed, dom, R.direct(v, fixed, dom), R.hitting_time(fixed, dom).max())
    return _DIRECT[key]


@pytest.mark.parametrize("seed", range(4))
@pytest.mark.parametrize("shape", [(40, 70), (70, 40)])
def test_direct_solve(shape, seed):
    from descriptools_amd import harmonic
    v, fixed, dom, exact, tmax = _direct(shape, seed)
    got = harmonic.interpolate(v, fixed.astype(np.int8), dom.astype(np.int8), tol=TOL)
    reach = _check(got, v, fixed, dom)
    assert np.array_equal(np.isnan(exact), ~reach | (reach & ~fixed & (R.average(exact, dom)[1] == 0)))
    both = reach & ~np.isnan(exact)
    err = np.abs(got.field[both] - exact[both]).max()
    print("error %.3g, bound %.3g (max t %.1f)" % (err, TOL * tmax, tmax))
    assert err <= TOL * tmax + 1e-9 * np.abs(v).max()
    assert got.info["levels"] == 2


# ---- 4. larger: residual, maximum principle, the same bits -----------------------------------------------------------
def _large():
    rng = np.random.default_rng(11)
    H, W = 200, 333
    dom = rng.random((H, W)) >= 0.10
    dom[62:67, 62:67] = False      # on the corner of four tiles
    dom[120:124, 100:200] = False  # a wall
    fixed = dom & (rng.random((H, W)) < 0.002)
    v = np.where(fixed, rng.normal(0.0, 300.0, (H, W)), 0.0).astype(np.float32)
    return v, fixed, dom


def test_larger_residual_maximum_principle_and_bits():
    from descriptools_amd import harmonic
    v, fixed, dom = _large()
    got = harmonic.interpolate(v, fixed.astype(np.int8), dom.astype(np.int8), tol=TOL)
    reach = _check(got, v, fixed, dom)
    assert got.info["levels"] == 4
    # the start copies fixed values of the coarsest level (means of input values) and every later value is an average:
    # for float32 inputs k * max is a float64, so no rounding carries a value out of [min, max]
    lo, hi = float(v[fixed].min()), float(v[fixed].max())
    assert got.field[reach].min() >= lo and got.field[reach].max() <= hi
    again = harmonic.interpolate(v, fixed.astype(np.int8), dom.astype(np.int8), tol=TOL)
    assert np.array_equal(_bits(got.field), _bits(again.field))
    assert again.info == got.info


# ---- 5. components --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("thick,H", [(8, 70), (1, 20)])
def test_rooms(thick, H):
    from descriptools_amd import harmonic
    W = 150
    dom = np.ones((H, W), bool)
    dom[:, 48:48 + thick] = False  # the left room has no fixed cell
    dom[:, 96:96 + thick] = False  # the middle room (across the seam at column 64) has one; the right room has two
    fixed = np.zeros((H, W), bool)
    fixed[H - 4, 60] = fixed[3, 110] = fixed[H - 2, 140] = True
    v = np.zeros((H, W), np.float32)
    v[H - 4, 60], v[3, 110], v[H - 2, 140] = 12.25, -3.0, 5.0
    got = harmonic.interpolate(v, fixed.astype(np.int8), dom.astype(np.int8), tol=TOL)
    _check(got, v, fixed, dom)
    assert np.isnan(got.field[:, :48 + thick]).all() and got.info["unreached"] == 48 * H
    middle = got.field[:, 48 + thick:96]
    if thick == 8:
        # the walls survive both coarsenings (8 cells from a multiple of 8): the room (across the seams at row 64 and
        # column 64) is closed off on every level, starts from its own fixed value and never leaves it
        assert (middle == 12.25).all()
    else:
        # a coarse cell merges both sides of a one-cell wall: the room starts from a mixture and comes back to its value
        # as far as tol says
        room = np.zeros((H, W), bool)
        room[:, 49:96] = True
        tmax = R.hitting_time(fixed & room, room).max()
        print("room: error %.3g, bound %.3g" % (np.abs(middle - 12.25).max(), TOL * tmax))
        assert np.abs(middle - 12.25).max() <= TOL * tmax
    right = got.field[:, 96 + thick:]
    assert right.min() >= -3.0 and right.max() <= 5.0 and right.min() < right.max()


# ---- 6. the budget ---------------------------------------------------------------------------------------------------
def _dev(ctx, v, fixed, dom, tol, max_rounds):
    """dt_dev_harmonic on resident rasters -> (field, info, status bits)"""
    from descriptools_amd import _lib
    H, W = v.shape
    d_v = ctx.to_device(np.ascontiguousarray(v, np.float32))
    d_f = ctx.to_device(np.ascontiguousarray(fixed, np.int8))
    d_d = ctx.to_device(np.ascontiguousarray(dom, np.int8)) if dom is not None else None
    d_o, d_i = ctx.empty((H, W), np.float64), ctx.empty((40,), np.int64)
    try:
        _lib.check(_lib.lib().dt_dev_harmonic(ctx.h, d_v.ptr, d_f.ptr, d_d.ptr if d_d else None, H, W, tol, max_rounds,
                                              d_o.ptr, d_i.ptr))
        st = ctx.status()
        return d_o.to_host(), d_i.to_host(), st
    finally:
        for a in (d_v, d_f, d_d, d_o, d_i):
            if a is not None:
                a.free()


def test_budget():
    from descriptools_amd import _lib, harmonic
    from descriptools_amd.device import Context
    v, fixed, dom = _large()
    reach = R.reachable(fixed, dom)
    with pytest.raises(RuntimeError, match=r"residual.*max_rounds = 1\b"):
        harmonic.interpolate(v, fixed.astype(np.int8), dom.astype(np.int8), tol=1e-12, max_rounds=1)
    # strict=False hands out the last iterate, warns, and says so in the info
    with pytest.warns(RuntimeWarning, match=r"residual.*max_rounds = 1\b"):
        last = harmonic.interpolate(v, fixed.astype(np.int8), dom.astype(np.int8), tol=1e-12, max_rounds=1,
                                    strict=False)
    assert not last.info["converged"] and last.info["rounds"] == 1 and last.info["residual"] > 1e-12
    assert np.array_equal(np.isnan(last.field), ~reach)
    assert np.array_equal(_bits(last.field[fixed]), _bits(v[fixed].astype(np.float64)))
    assert last.info["residual"] == R.residual(np.where(reach, last.field, 0.0), fixed, reach).max()
    ctx = Context()
    try:
        u, info, st = _dev(ctx, v, fixed, reach, 1e-12, 1)
        assert np.array_equal(_bits(u), _bits(last.field)), "both tiers stop at the same iterate"
        assert st == 2, "DT_STATUS_NOT_CONVERGED"
        assert info[5] == 0 and info[1] == 1 and info[4:5].view(np.float64)[0] > 1e-12
        assert np.array_equal(_bits(u[fixed]), _bits(v[fixed].astype(np.float64)))
        L = _lib.lib()
        for tol, n, word in ((0.0, 8, b"tol"), (float("inf"), 8, b"tol"), (1e-5, 0, b"max_rounds"),
                             (1e-5, 4097, b"max_rounds")):
            assert L.dt_dev_harmonic(ctx.h, None, None, None, 4, 4, tol, n, None, None) == -1
            assert word in L.dt_last_error()
        assert L.dt_dev_harmonic(ctx.h, None, None, None, 4, 4, 1e-5, 8, None, None) == -1
        assert b"NULL raster" in L.dt_last_error()
        assert L.dt_dev_harmonic(ctx.h, None, None, None, 0, 7, 1e-5, 8, None, None) == 0
        assert ctx.status() == 0
    finally:
        ctx.close()


def test_host_entry_refusals():
    """dt_harmonic refuses, in this order and before it touches a raster: the shape, tol, the budget, NULL rasters"""
    from descriptools_amd import _lib
    L = _lib.lib()
    info = np.zeros(40, np.int64)
    pi = _lib.ptr(info, _lib.c_i64p)
    for args, word in (((-1, 4, 1e-5, 8), b"shape"), ((65536, 32768, 1e-5, 8), b"2^31"), ((4, 4, 0.0, 8), b"tol"),
                       ((4, 4, float("nan"), 8), b"tol"), ((4, 4, float("inf"), 8), b"tol"),
                       ((4, 4, 1e-5, 0), b"max_rounds"), ((4, 4, 1e-5, 4097), b"max_rounds"),
                       ((4, 4, 1e-5, 8), b"NULL raster")):
        assert L.dt_harmonic(None, None, None, *args, None, pi) == -1, args
        assert word in L.dt_last_error(), (args, L.dt_last_error())
    info[:] = 7
    assert L.dt_harmonic(None, None, None, 0, 9, 1e-5, 8, None, pi) == 0 and not info.any()


# ---- 7. non-finite and below-sentinel values -------------------------------------------------------------------------
def test_nonfinite_values():
    from descriptools_amd import harmonic
    v, fixed, dom, _, _ = _direct((40, 70), 0)
    fx8, dom8 = fixed.astype(np.int8), dom.astype(np.int8)
    clean = harmonic.interpolate(v, fx8, dom8, tol=TOL)
    # on free cells (and outside the domain) the values are never read
    dirty = v.copy()
    bad = np.array([np.nan, np.inf, -np.inf, -1000.0, -100.0, 3e38], np.float32)
    dirty[~fixed] = bad[np.arange(int((~fixed).sum())) % bad.size]
    got = harmonic.interpolate(dirty, fx8, dom8, tol=TOL)
    assert np.array_equal(_bits(got.field), _bits(clean.field)) and got.info == clean.info
    # a cell with fixed == 1 and a non-finite value is outside the domain, whatever `domain` says
    ys, xs = np.nonzero(fixed)
    hurt = v.copy()
    for i, b in enumerate((np.nan, np.inf, -np.inf)):
        hurt[ys[i], xs[i]] = b
    gone = np.zeros_like(fixed)
    gone[ys[:3], xs[:3]] = True
    got = harmonic.interpolate(hurt, fx8, dom8, tol=TOL)
    _check(got, v, fixed & ~gone, dom & ~gone)
    assert np.isnan(got.field[gone]).all()
    # a DEM height at or below the sentinel is nodata to base_level and vdcn, on a river cell too
    dem = (100.0 + 0.25 * np.arange(70, dtype=np.float32))[None, :].repeat(40, 0)
    river = np.zeros((40, 70), np.int8)
    river[:, 5] = 1
    dem[7, 5], dem[20, 30], dem[21, 5] = -1000.0, -100.0, np.nan
    base = harmonic.base_level(dem, river, tol=TOL)
    vd = harmonic.vdcn(dem, river, tol=TOL)
    for y, x in ((7, 5), (20, 30), (21, 5)):
        assert base[y, x] == -100.0 and vd[y, x] == -100.0
    ok = np.ones((40, 70), bool)
    ok[7, 5] = ok[20, 30] = ok[21, 5] = False
    assert (base[ok] == 101.25).all() and np.array_equal(vd[ok], dem[ok].astype(np.float64) - 101.25)


# ---- 8. fill_voids ---------------------------------------------------------------------------------------------------
def _holes(shape):
    seam = np.zeros(shape, bool)
    seam[60:67, 58:67] = True      # 7 x 9, across the seams at row 64 and column 64
    single = np.zeros(shape, bool)
    single[20, 100] = True
    edge = np.zeros(shape, bool)
    edge[90:96, 30:34] = True      # touches the last row
    large = np.zeros(shape, bool)
    large[10:40, 110:140] = True   # 900 cells
    return seam, single, edge, large


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_fill_voids(dtype):
    from descriptools_amd import harmonic
    H, W = 96, 150
    yy, xx = np.mgrid[0:H, 0:W]
    plane = (2.0 * xx + 0.5 * yy).astype(dtype)
    seam, single, edge, large = _holes((H, W))
    dem = plane.copy()
    dem[seam | single | edge | large] = -100
    dem[large & (xx == 120)] = -9999  # every value <= -100 is nodata
    got = harmonic.fill_voids(dem, max_cells=100)
    assert got.dtype == dem.dtype and got is not dem
    kept = ~(seam | single)
    assert np.array_equal(got[kept].view(np.uint8), dem[kept].view(np.uint8)), "valid and unfilled cells: the same bits"
    # an interior void of a plane is harmonic with the plane as its solution; the bound is tol * max(t) of that void
    for void in (seam, single):
        tmax = R.hitting_time(~void, np.ones((H, W), bool)).max()
        err = np.abs(got[void].astype(np.float64) - plane[void]).max()
        print("void of %d cells: error %.3g, bound %.3g" % (void.sum(), err, TOL * tmax))
        assert err <= TOL * tmax + (2.0 ** -24 * 400 if dtype is np.float32 else 1e-9 * 400)
    every = harmonic.fill_voids(dem, edges=True)
    assert (every > -100).all()
    valid = ~(seam | single | edge | large)
    assert np.array_equal(every[valid].view(np.uint8), dem[valid].view(np.uint8))
    # (a void on the border is no Dirichlet problem of the plane: zero flux at the edge bends it; within the range)
    assert every[edge].min() >= plane[85:, 25:40].min() and every[large].max() <= plane[5:45, 105:145].max()
    assert harmonic.fill_voids(plane) is not plane and np.array_equal(harmonic.fill_voids(plane), plane)
    assert np.array_equal(harmonic.fill_voids(dem, max_cells=0), dem)


def test_fill_voids_takes_nan_holes():
    from descriptools_amd import harmonic
    H, W = 20, 80
    yy, xx = np.mgrid[0:H, 0:W]
    plane = (2.0 * xx + 0.5 * yy).astype(np.float32)
    dem = plane.copy()
    dem[5:9, 60:68] = np.nan     # a hole of NaN across the seam
    dem[8:11, 66:70] = -100      # grown together with one of the sentinel: one void
    dem[15, 10] = np.inf         # neither valid nor a void
    got = harmonic.fill_voids(dem)
    void = np.isnan(dem) | (dem <= -100)
    keep = ~void
    assert np.array_equal(got[keep].view(np.uint32), dem[keep].view(np.uint32)) and got[15, 10] == np.inf
    tmax = R.hitting_time(~void & np.isfinite(dem), np.isfinite(dem) | void).max()
    assert np.abs(got[void].astype(np.float64) - plane[void]).max() <= TOL * tmax + 2.0 ** -24 * 200


def test_fill_voids_integer_dem():
    from descriptools_amd import harmonic
    dem = (10 * np.arange(80, dtype=np.int16))[None, :].repeat(9, 0)
    dem[3:6, 62:67] = -32768
    got = harmonic.fill_voids(dem)
    assert got.dtype == np.int16 and np.array_equal(got, (10 * np.arange(80, dtype=np.int16))[None, :].repeat(9, 0))


# ---- 9. vdcn ---------------------------------------------------------------------------------------------------------
def test_vdcn_of_a_valley():
    from descriptools_amd import harmonic
    H, W = 50, 130
    dem = (0.5 * np.abs(np.arange(W) - 40.0)).astype(np.float32)[None, :].repeat(H, 0)
    river = np.zeros((H, W), np.int8)
    river[:, 40] = 1
    base = harmonic.base_level(dem, river)
    assert base.dtype == np.float64 and (base == 0.0).all()
    vd = harmonic.vdcn(dem, river)
    assert vd.dtype == np.float64 and np.array_equal(_bits(vd), _bits(dem.astype(np.float64)))
    hole = np.zeros((H, W), bool)
    hole[10:13, 60:70] = hole[30, 40] = True
    hole[:, 100] = True  # cuts the columns beyond it off the river: no value there either
    dem2 = np.where(hole, np.float32(-100), dem)
    vd2 = harmonic.vdcn(dem2, river)
    none = hole | (np.arange(W) > 100)[None, :]
    assert (vd2[none] == -100.0).all()
    assert np.array_equal(_bits(vd2[~none]), _bits(dem[~none].astype(np.float64)))


def test_vdcn_of_a_float64_dem_is_zero_on_the_river():
    from descriptools_amd import harmonic
    H, W = 12, 70
    dem = 100.1 + 0.3 * np.abs(np.arange(W) - 20.0)[None, :].repeat(H, 0)  # no float32 holds these heights
    river = np.zeros((H, W), np.int8)
    river[:, 20] = 1
    vd = harmonic.vdcn(dem, river)
    d32 = dem.astype(np.float32).astype(np.float64)
    assert (vd[:, 20] == 0.0).all() and np.array_equal(_bits(vd), _bits(d32 - d32[0, 20]))


# ---- 10. the device tier ---------------------------------------------------------------------------------------------
def test_device_tier_equals_the_host_tier():
    from descriptools_amd import harmonic
    from descriptools_amd.device import Context
    ctx = Context()
    try:
        for shape, seed in (((40, 70), 1), ((70, 40), 2)):  # the second call reclaims the scratch at another shape
            v, fixed, dom, _, _ = _direct(shape, seed)
            want = harmonic.interpolate(v, fixed.astype(np.int8), dom.astype(np.int8), tol=TOL)
            reach = R.reachable(fixed, dom)  # (the C entries' precondition: what the Python tier hands them)
            u, info, st = _dev(ctx, v, fixed, reach, TOL, 1024)  # (these cases take some hundred rounds)
            assert st == 0
            assert np.array_equal(_bits(u), _bits(want.field))
            assert info[0] == want.info["levels"] and info[1] == want.info["rounds"]
            assert info[2] == want.info["rounds_all"] and info[3] == want.info["tile_visits"] and info[5] == 1
            assert info[4:5].view(np.float64)[0] == want.info["residual"]
    finally:
        ctx.close()
