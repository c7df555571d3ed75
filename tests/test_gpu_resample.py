"""GPU (-m gpu): resample.warp / align / resize / aggregate (dt_resample, dt_dev_resample, k_rs_* in dt_resample.hip)
against tests/_resample_ref.py, every comparison on bit patterns, dtype and shape included.  Trivial shapes (1 x 1,
1 x 200, 200 x 1); 65 x 63 <-> 130 x 126; a 130 x 257 source against destinations whose tiles are ragged in both axes;
identity, integer zooms x2 x3 x4 up and down, non-integer ratios with offsets, destinations partly and wholly outside
(offsets of +-10^12), rotation, flip and transpose for the point methods, centres on cell edges; nodata of every kind
as single cells, a block over a tile corner, a whole row, a whole raster; cubic's fallback beside complete windows; every
dtype of nearest; mode with all 256 values, exact ties and nodata, on its thread-per-cell and its histogram path; the
footprint cap at 255, 256 and 257; a 1700 x 2401 source onto 330 x 1050, the tiling of large rasters (256-column tiles,
several stages of 4 rows).  Independent of the reference: identity, np.repeat, reshape-sums, exact ramps, ranges.  The
device tier against the host tier, the C entry between guard bands, the coarse-simulation recipe end to end."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import _resample_ref as R

pytestmark = pytest.mark.gpu

IDENTITY = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)
FLOAT_METHODS = ("nearest", "bilinear", "cubic", "average", "sum", "min", "max")
POINT_METHODS = ("nearest", "bilinear", "cubic")
AREA_METHODS = ("average", "sum", "min", "max")


@functools.lru_cache(maxsize=None)
def _dem(shape, dtype="float64", holes=True, seed=1):
    """smooth + noise, with nodata of every kind: single cells, a block over the corner of the first 64 x 64 tile, a whole
    row"""
    H, W = shape
    rng = np.random.default_rng(seed + 17 * H + W)
    yy, xx = np.mgrid[0:H, 0:W]
    z = 300.0 + 40.0 * np.sin(xx / 9.0) * np.cos(yy / 7.0) + rng.uniform(-3.0, 3.0, shape)
    z = z.astype(dtype)
    if holes:
        flat = z.reshape(-1)
        n = flat.size
        for k, bad in enumerate((-100.0, -100.5, -1e30, np.nan, np.inf, -np.inf)):
            flat[(7 + 31 * k) % n] = bad
            flat[(n // 2 + 5 * k) % n] = bad
        if H > 70 and W > 70:
            z[60:67, 61:69] = np.nan
            z[100, :] = -100.0
            z[20:24, 20:24] = 1e6 * rng.uniform(-1.0, 1.0, (4, 4))   # a spike: cubic overshoots, sums cancel
    z.setflags(write=False)
    return z


def check(src, matrix, shape, method, **kw):
    from descriptools_amd import resample
    got = resample.warp(src, matrix, shape, method, **kw)
    R.same("%s %s -> %s %r" % (method, np.asarray(src).shape, shape, matrix), got, R.warp(src, matrix, shape, method, **kw))
    return got


# ---- shapes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("shape", [(1, 1), (1, 200), (200, 1)])
def test_trivial_shapes(shape, dtype):
    z = _dem(shape, dtype, holes=shape != (1, 1))
    H, W = shape
    for method in FLOAT_METHODS:
        check(z, IDENTITY, shape, method)
        check(z, (0.0, W / (2 * W + 1), 0.0, 0.0, 0.0, H / (H + 2)), (H + 2, 2 * W + 1), method)
        check(z, (-0.25, max(W / 7, 1.0), 0.0, -0.5, 0.0, max(H / 5, 1.0)), (6, 8), method)
    check(np.full((1, 1), -100.0, dtype), IDENTITY, (3, 3), "bilinear")


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("method", FLOAT_METHODS)
def test_identity_and_integer_zooms(method, dtype):
    from descriptools_amd import resample
    z = _dem((65, 63), dtype)
    check(z, IDENTITY, z.shape, method)
    up = check(z, (0.0, 0.5, 0.0, 0.0, 0.0, 0.5), (130, 126), method)
    check(up, (0.0, 2.0, 0.0, 0.0, 0.0, 2.0), (65, 63), method)
    for k in (3, 4):
        check(z, (0.0, 1.0 / k, 0.0, 0.0, 0.0, 1.0 / k), (65 * k, 63 * k), method)
        check(z, (0.0, float(k), 0.0, 0.0, 0.0, float(k)), (-(-65 // k), -(-63 // k)), method)
    R.same("resize", resample.resize(z, (130, 126), method), R.resize(z, (130, 126), method))
    if method in AREA_METHODS:
        R.same("aggregate", resample.aggregate(z, (2, 3), method), R.aggregate(z, (2, 3), method))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("method", FLOAT_METHODS)
def test_ragged_tiles_and_offsets(method, dtype):
    z = _dem((130, 257), dtype)
    check(z, (-0.3, 257 / 70, 0.0, 0.2, 0.0, 130 / 33), (33, 70), method)          # 257 -> 70 columns
    check(z, (0.7, 257 / 300, 0.0, -1.4, 0.0, 130 / 131), (131, 300), method)       # just under 1: two cells per tap
    check(z, (-3.5, 0.37, 0.0, 2.25, 0.0, 0.41), (259, 515), method)                # up, past two edges
    check(z, (100.0, 17.3, 0.0, 50.0, 0.0, 9.9), (12, 13), method)                  # wide footprints, partly outside
    check(z, (-40.0, 1.0, 0.0, -30.0, 0.0, 1.0), (200, 340), method)                # the source inside the destination


@pytest.mark.parametrize("method", FLOAT_METHODS)
def test_wholly_outside_and_far_away(method):
    z = _dem((65, 63), "float32")
    for a0, b0 in ((1e12, 0.0), (-1e12, 0.0), (0.0, 1e12), (5.0, -1e12), (63.0, 0.0), (-70.0, 3.0), (1e300, -1e300)):
        got = check(z, (a0, 1.0, 0.0, b0, 0.0, 1.0), (66, 70), method)
        assert (got == np.float32(-100)).all()
    far = check(z, (-1e12, 1e12 / 32, 0.0, 2.0, 0.0, 1.0), (8, 70), "nearest")      # strides of 3 * 10^10 cells
    assert (far != np.float32(-100)).sum() <= 8


@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("method", POINT_METHODS)
def test_rotation_flip_transpose(method, dtype):
    z = _dem((130, 257), dtype)
    c, s = math.cos(math.radians(30.0)), math.sin(math.radians(30.0))
    check(z, (60.0, c, -s, -20.0, s, c), (150, 200), method)
    check(z, (0.0, 1.0, 0.0, 130.0, 0.0, -1.0), (130, 257), method)                 # vertical flip
    check(z, (257.0, -0.5, 0.0, 0.0, 0.0, 0.5), (260, 514), method)                 # mirrored and zoomed
    check(z, (0.0, 0.0, 1.0, 0.0, 1.0, 0.0), (257, 130), method)                    # transpose
    if method == "nearest":
        from descriptools_amd import resample
        assert np.array_equal(resample.warp(z, (0.0, 0.0, 1.0, 0.0, 1.0, 0.0), (257, 130)).view(np.int64 if dtype == "float64" else np.int32),
                              z.T.view(np.int64 if dtype == "float64" else np.int32))


@pytest.mark.parametrize("method", FLOAT_METHODS)
def test_centres_on_cell_edges(method):
    z = _dem((65, 63), "float64")
    check(z, (-0.5, 1.0, 0.0, -0.5, 0.0, 1.0), (67, 65), method)                    # u = j: every centre on a corner
    check(z, (0.0, 2.0, 0.0, 0.0, 0.0, 2.0), (33, 32), method)                      # u = 2j + 1
    check(z, (0.5, 1.0, 0.0, 0.0, 0.0, 1.0), (65, 64), method)                      # edges in x only


def test_all_nodata_raster():
    bad = np.array([-100.0, -250.0, np.nan, np.inf, -np.inf])[np.arange(70 * 66) % 5].reshape(70, 66)
    for method in FLOAT_METHODS[1:]:
        for m, shape in ((IDENTITY, (70, 66)), ((0.0, 0.5, 0.0, 0.0, 0.0, 0.5), (140, 132)), ((0.0, 3.0, 0.0, 0.0, 0.0, 3.0), (24, 22))):
            assert (check(bad, m, shape, method) == -100.0).all()


def test_cubic_falls_back_beside_complete_windows():
    from descriptools_amd import resample
    z = np.array(_dem((65, 63), "float64", holes=False))
    z[30, 30] = np.nan
    m, shape = (0.0, 0.5, 0.0, 0.0, 0.0, 0.5), (130, 126)
    cub, bil = check(z, m, shape, "cubic"), check(z, m, shape, "bilinear")
    same = cub.view(np.int64) == bil.view(np.int64)
    u, v = R.centres(m, shape)
    c0, r0 = np.floor(u - 0.5), np.floor(v - 0.5)
    edge = (c0 < 1) | (r0 < 1) | (c0 + 2 > 62) | (r0 + 2 > 64)
    hole = (np.abs(c0 + 0.5 - 30) <= 1.5) & (np.abs(r0 + 0.5 - 30) <= 1.5)
    assert same[edge | hole].all(), "the window touches the edge or the invalid cell: bilinear"
    assert (~same[~(edge | hole)]).mean() > 0.9, "complete windows: cubic"
    assert (resample.resize(z, shape, "cubic")[60:62, 60:62] == -100.0).all()


# ---- nearest: every dtype ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["bool", "int8", "uint8", "int16", "uint16", "float16", "int32", "uint32", "float32",
                                   "int64", "uint64", "float64"])
def test_nearest_every_dtype(dtype):
    from descriptools_amd import resample
    rng = np.random.default_rng(9)
    raw = rng.integers(0, 256, (65, 63, 8), dtype=np.uint8)
    dt = np.dtype(dtype)
    z = (raw[..., 0] > 127) if dt.kind == "b" else np.ascontiguousarray(raw[..., :dt.itemsize]).view(dt)[..., 0]
    if dt == np.int64:
        z = np.arange(65 * 63, dtype=np.int64).reshape(65, 63) * (1 << 33) - 7       # flat-index labels beyond 2^32
    for m, shape in ((IDENTITY, (65, 63)), ((0.0, 1 / 3, 0.0, 0.0, 0.0, 1 / 3), (195, 189)),
                     ((-2.5, 63 / 40, 0.0, 1.5, 0.0, 65 / 90), (95, 47)), ((0.0, 0.0, 1.0, 0.0, 1.0, 0.0), (63, 65))):
        check(z, m, shape, "nearest")
    fill = {"b": True, "u": 200, "i": -7, "f": 2.5}[dt.kind]
    got = check(z, (-2.0, 1.0, 0.0, -1.0, 0.0, 1.0), (70, 70), "nearest", fill=fill)
    assert got[0, 0] == fill and got.dtype == dt
    k = 3
    assert np.array_equal(resample.resize(z, (65 * k, 63 * k)).view(np.uint8),
                          np.repeat(np.repeat(z, k, axis=0), k, axis=1).view(np.uint8)), "np.repeat"


# ---- mode -----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _classes(shape=(130, 257)):
    rng = np.random.default_rng(21)
    z = rng.integers(0, 6, shape).astype(np.uint8)                  # few classes: ties everywhere
    z[:32, :64] = np.arange(2048, dtype=np.int64).reshape(32, 64) % 256   # all 256 values, each 8 times in 32 x 64
    z[40:48, 40:48] = np.array([[250, 3], [3, 250]], np.uint8).repeat(4, 0).repeat(4, 1)  # a tie, the larger value first
    z[100:, 200:] = 9
    z.setflags(write=False)
    return z


@pytest.mark.parametrize("factor", [1, 2, 3, 5, 7, 8, 32, (32, 64), (3, 40)])
def test_mode(factor):
    from descriptools_amd import resample
    z = _classes()
    for kw in ({}, {"nodata": 3}, {"nodata": 9, "fill": 255}):
        R.same("mode %r %r" % (factor, kw), resample.aggregate(z, factor, "mode", **kw), R.aggregate(z, factor, "mode", **kw))
    if factor == (32, 64):
        assert resample.aggregate(z, factor, "mode")[0, 0] == 0, "all 256 values tie: the smallest"
    if factor == 8:
        got = resample.aggregate(z, 8, "mode")
        assert got[5, 5] == 3, "a tie goes to the smaller value, not the first met"
        assert resample.aggregate(z, 8, "mode", nodata=9, fill=255)[15, 30] == 255


def test_mode_ragged_and_outside():
    z = _classes()
    check(z, (-0.3, 257 / 70, 0.0, 0.2, 0.0, 130 / 33), (33, 70), "mode")
    check(z, (-3.5, 0.37, 0.0, 2.25, 0.0, 0.41), (259, 515), "mode", fill=7)
    check(z, (100.0, 17.3, 0.0, 50.0, 0.0, 9.9), (12, 13), "mode", nodata=0)
    check(z, (1e12, 9.0, 0.0, 0.0, 0.0, 9.0), (5, 5), "mode", fill=1)
    check(z, (1e12, 1.0, 0.0, 0.0, 0.0, 1.0), (5, 5), "mode", fill=1)
    check(np.full((1, 1), 4, np.uint8), (-1.0, 1.0, 0.0, -1.0, 0.0, 1.0), (3, 3), "mode")


# ---- the footprint cap ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", [255, 256])
def test_footprint_cap_is_served(factor):
    from descriptools_amd import resample
    for dtype in ("float32", "float64"):
        z = _dem((300, 520), dtype)
        for how in AREA_METHODS:
            R.same("%s %d" % (how, factor), resample.aggregate(z, factor, how), R.aggregate(z, factor, how))
    u8 = np.random.default_rng(2).integers(0, 256, (300, 520), dtype=np.uint8)
    R.same("mode", resample.aggregate(u8, factor, "mode"), R.aggregate(u8, factor, "mode"))
    ones = np.ones((300, 520), np.uint8)
    assert resample.aggregate(ones, factor, "mode")[0, 0] == 1, "%d^2 cells of one value: more than a 16-bit count" % factor


def test_footprint_cap_is_refused_beyond():
    from descriptools_amd import _lib, resample
    z = _dem((300, 520), "float32")
    with pytest.raises(ValueError, match="chain two calls"):
        resample.aggregate(z, 257, "average")
    L = _lib.lib()
    out = np.zeros((2, 3), np.float32)
    m = (C.c_double * 6)(0.0, 257.0, 0.0, 0.0, 0.0, 257.0)
    assert L.dt_resample(z.ctypes.data, 32, 300, 520, m, 3, -1, 0, out.ctypes.data, 2, 3) == -1
    assert b"chain two calls" in L.dt_last_error()
    assert (out == 0).all()


# ---- independent of the reference -------------------------------------------------------------------------------------
def test_sums_of_integer_valued_data_are_exact():
    from descriptools_amd import resample
    rng = np.random.default_rng(7)
    z = rng.integers(-90, 100000, (128, 192)).astype(np.float64)
    for fy, fx in ((2, 2), (4, 3), (64, 64), (128, 192)):
        want = z.reshape(128 // fy, fy, 192 // fx, fx).sum(axis=(1, 3))
        got = resample.aggregate(z, (fy, fx), "sum")
        assert np.array_equal(got, want) and got.sum() == z.sum()
        assert np.array_equal(resample.aggregate(z, (fy, fx), "max"), z.reshape(128 // fy, fy, 192 // fx, fx).max(axis=(1, 3)))


def test_ramp_is_exact():
    from descriptools_amd import resample
    Hs, Ws = 65, 63
    ramp = 500.0 + 2.0 * np.arange(Ws)[None, :] - 5.0 * np.arange(Hs)[:, None]        # > -100 everywhere
    for zoom in (2, 4, 8):
        shape = (Hs * zoom, Ws * zoom)
        u, v = R.centres((0.0, 1.0 / zoom, 0.0, 0.0, 0.0, 1.0 / zoom), shape)
        want = np.broadcast_to(500.0 + 2.0 * (u - 0.5) - 5.0 * (v - 0.5), shape)
        for method, margin in (("bilinear", 0.5), ("cubic", 1.5)):
            got = resample.resize(ramp, shape, method)
            inner = (u >= margin) & (u < Ws - margin) & (v >= margin) & (v < Hs - margin)
            assert np.array_equal(got[inner], want[inner]), (zoom, method)


def test_ranges():
    """R.range_case: the same raster and the same checks that tests/test_resample_host.py runs on the reference"""
    from descriptools_amd import resample
    z = R.range_case()
    R.check_ranges(z, [resample.aggregate(z, 3, how) for how in ("min", "average", "max")],
                   resample.warp(z, *R.RANGE_ZOOM, "bilinear"))


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_identity_returns_the_input(dtype):
    """without the reference: nearest gives the input's bits, every other float method the input where it is valid
    (finite and > -100) and -100 elsewhere, every dtype of nearest its own bits"""
    from descriptools_amd import resample
    bits = np.int32 if dtype == "float32" else np.int64
    for shape in ((65, 63), (130, 257)):
        z = _dem(shape, dtype)
        with np.errstate(invalid="ignore"):
            want = np.where(np.isfinite(z) & (z > -100), z, np.dtype(dtype).type(-100))
        assert not np.array_equal(want.view(bits), z.view(bits)), "the raster holds nodata of other bit patterns"
        for method in FLOAT_METHODS:
            got = resample.warp(z, IDENTITY, shape, method)
            assert got.dtype == z.dtype and got.shape == z.shape
            assert np.array_equal(got.view(bits), (z if method == "nearest" else want).view(bits)), (method, shape)
    u8 = _classes()
    for method in ("nearest", "mode"):
        assert np.array_equal(resample.warp(u8, IDENTITY, u8.shape, method), u8), method
    lab = np.arange(130 * 257, dtype=np.int64).reshape(130, 257) * (1 << 33) - 7
    assert np.array_equal(resample.warp(lab, IDENTITY, lab.shape), lab)


# ---- tiers and plumbing ---------------------------------------------------------------------------------------------
def _dev(ctx, src, matrix, shape, method, nodata=-1, fill_bits=0):
    from descriptools_amd import _lib, resample
    a = np.ascontiguousarray(src)
    code = resample._code(method, a.dtype)
    d_src, d_dst = ctx.to_device(a), ctx.empty(shape, a.dtype)
    try:
        m = (C.c_double * 6)(*matrix)
        _lib.check(_lib.lib().dt_dev_resample(ctx.h, d_src.ptr, code, a.shape[0], a.shape[1], m,
                                              resample.METHODS.index(method), nodata, fill_bits, d_dst.ptr, shape[0], shape[1]))
        return d_dst.to_host()
    finally:
        d_src.free()
        d_dst.free()


def test_device_tier_equals_the_host_tier():
    from descriptools_amd import _lib, resample
    from descriptools_amd.device import Context
    z32, z64, u8 = _dem((130, 257), "float32"), _dem((130, 257), "float64"), _classes()
    i64 = np.arange(130 * 257, dtype=np.int64).reshape(130, 257) << 20
    f32_bits = int(np.array(-100, np.float32).view(np.uint32))
    i64_bits = int(np.array(-100, np.int64).view(np.uint64))
    ctx = Context()
    try:
        for m, shape in (((-0.3, 257 / 70, 0.0, 0.2, 0.0, 130 / 33), (33, 70)), ((-3.5, 0.37, 0.0, 2.25, 0.0, 0.41), (259, 515))):
            for method in FLOAT_METHODS[1:]:
                for z in (z32, z64):
                    R.same(method, _dev(ctx, z, m, shape, method), resample.warp(z, m, shape, method))
            R.same("nearest f32", _dev(ctx, z32, m, shape, "nearest", fill_bits=f32_bits), resample.warp(z32, m, shape))
            R.same("nearest i64", _dev(ctx, i64, m, shape, "nearest", fill_bits=i64_bits), resample.warp(i64, m, shape))
            R.same("mode", _dev(ctx, u8, m, shape, "mode", nodata=3, fill_bits=77), resample.warp(u8, m, shape, "mode", nodata=3, fill=77))
        assert ctx.status() == 0
        L = _lib.lib()
        mat = (C.c_double * 6)(*IDENTITY)
        assert L.dt_dev_resample(ctx.h, None, 32, 4, 4, mat, 1, -1, 0, None, 4, 4) == -1
        assert L.dt_last_error() == b"invalid argument: NULL raster"
        assert L.dt_dev_resample(ctx.h, None, 32, 4, 4, (C.c_double * 6)(0.0, 257.0, 0.0, 0.0, 0.0, 1.0), 3, -1, 0, None, 4, 4) == -1
        assert b"chain two calls" in L.dt_last_error()
    finally:
        ctx.close()


@functools.lru_cache(maxsize=None)
def _wide_tiles_case():
    """a destination of 346,500 cells: tiles of 256 columns (the last one ragged), several stages of 4 rows per tile
    (b2 = 5.3 takes 6 or 7 rows), offsets in both axes.  -> (float64 source, matrix, shape, {method: reference})"""
    H, W = 1700, 2401
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:H, 0:W]
    z = 300.0 + 40.0 * np.sin(xx / 90.0) * np.cos(yy / 70.0) + rng.uniform(-3.0, 3.0, (H, W))
    z[rng.random((H, W)) < 0.01] = np.nan
    z[1000:1040, 500:1300] = -100.0
    z[3, :] = np.inf
    z.setflags(write=False)
    m, shape = (-1.3, 2.3, 0.0, -0.7, 0.0, 5.3), (330, 1050)
    return z, m, shape


@pytest.mark.parametrize("method, dtype", [("average", "float32"), ("average", "float64"), ("sum", "float32"),
                                           ("min", "float64"), ("max", "float32")])
def test_wide_tiles_and_many_stages_in_both_tiers(method, dtype):
    from descriptools_amd import resample
    from descriptools_amd.device import Context
    z64, m, shape = _wide_tiles_case()
    z = z64.astype(dtype)
    ref = R.warp(z, m, shape, method)
    assert (ref > -100).mean() > 0.9
    R.same("host tier", resample.warp(z, m, shape, method), ref)
    ctx = Context()
    try:
        R.same("device tier", _dev(ctx, z, m, shape, method), ref)
    finally:
        ctx.close()


GUARD = 4096


@pytest.mark.parametrize("method, dtype", [("nearest", "uint8"), ("nearest", "int16"), ("nearest", "float32"),
                                           ("nearest", "int64"), ("bilinear", "float32"), ("cubic", "float64"),
                                           ("average", "float32"), ("sum", "float64"), ("min", "float32"),
                                           ("mode", "uint8")])
def test_c_entry_writes_nothing_outside_dst(method, dtype):
    """odd destination shapes: rows that start off a 16-byte boundary, a last vector that would run past the end"""
    from descriptools_amd import _lib, resample
    dt = np.dtype(dtype)
    src = _classes() if dt == np.uint8 else (_dem((130, 257), dtype) if dt.kind == "f" else
                                             (np.arange(130 * 257).reshape(130, 257) % 30000).astype(dt))
    src = np.ascontiguousarray(src)
    code, bits = resample._code(method, dt), int.from_bytes(np.array(0 if dt.kind == "u" else -100, dt).tobytes(), "little")
    L = _lib.lib()
    for m, (Hd, Wd) in (((-0.3, 257 / 71, 0.0, 0.2, 0.0, 130 / 33), (33, 71)), ((-3.5, 0.37, 0.0, 2.25, 0.0, 0.41), (37, 515)),
                        ((0.0, 200.0, 0.0, 0.0, 0.0, 100.0), (2, 2))):
        raw = np.full(2 * GUARD + Hd * Wd * dt.itemsize, 0xA5, np.uint8)
        dst = raw[GUARD:raw.size - GUARD].view(dt).reshape(Hd, Wd)
        mat = (C.c_double * 6)(*m)
        _lib.check(L.dt_resample(src.ctypes.data, code, 130, 257, mat, resample.METHODS.index(method), -1, bits,
                                 dst.ctypes.data, Hd, Wd))
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all()
        R.same(method, dst, R.warp(src, m, (Hd, Wd), method))


def test_align_and_geotransforms():
    from descriptools_amd import resample
    z = _dem((130, 257), "float32")
    s = (500000.0, 30.0, 0.0, 4100000.0, 0.0, -30.0)
    d = (500100.0, 100.0, 0.0, 4099950.0, 0.0, -100.0)
    m = resample.compose(s, d)
    for method in ("nearest", "bilinear", "average", "max"):
        R.same(method, resample.align(z, s, d, (40, 80), method), R.warp(z, m, (40, 80), method))
    R.same("mode", resample.align(_classes(), s, d, (40, 80), "mode"), R.warp(_classes(), m, (40, 80), "mode"))


def test_coarse_simulation_fine_map_recipe():
    from descriptools_amd import inundation, resample
    yy, xx = np.mgrid[0:96, 0:96]
    dem = (5.0 + 0.02 * yy + 0.3 * np.abs(xx - 47.5)).astype(np.float32)             # a valley down the middle
    px = 10.0
    dem_c = resample.aggregate(dem, 4, "average")
    assert dem_c.shape == (24, 24) and dem_c.dtype == np.float32
    R.same("dem_c", dem_c, R.aggregate(dem, 4, "average"))
    depth0 = np.zeros((24, 24))
    depth0[2:6, 11:13] = 2.0
    res = inundation.simulate(dem_c, 4 * px, 600.0, depth=depth0, outputs=("depth", "max_depth"))
    wet = res.max_depth > 0
    assert 8 <= wet.sum() < 24 * 24
    wse_c = np.where(wet, dem_c + res.max_depth, -100.0)
    wse = resample.resize(wse_c, dem.shape, "bilinear")
    R.same("wse", wse, R.resize(wse_c, dem.shape, "bilinear"))
    depth = np.where(wse > -100, np.maximum(wse - dem, 0), 0)
    fine_wet = np.repeat(np.repeat(wet, 4, 0), 4, 1)
    assert (depth[~fine_wet] == 0).all(), "no water outside the coarse wet cells"
    assert (depth[fine_wet] >= 0).all() and (depth > 0).sum() > 16
