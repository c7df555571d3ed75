"""CPU (not gpu): descriptools_amd.resample without a device -- the numpy reference's own properties (identity, exact
block sums, exact ramps, ranges), every refusal of the module docstring (all raised before any library call), compose
against exact rational arithmetic, the geotransform helpers of rasterio_lite through a TIFF, and the plumbing: the
source file in the build list, the two C entries in the header and the binding table, the device entry's NULL-context
answer and the host entry's refusals, which come before it asks for a device."""
import ctypes as C
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _resample_ref as R
from descriptools_amd import _lib, build, rasterio_lite, resample

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IDENTITY = (0.0, 1.0, 0.0, 0.0, 0.0, 1.0)


def _raster(shape=(33, 41), dtype=np.float64, seed=3):
    rng = np.random.default_rng(seed)
    z = rng.uniform(-50.0, 900.0, shape).astype(dtype)
    z[4, 5], z[10, 7], z[20, 30], z[21, 3], z[0, 0] = -100.0, np.nan, np.inf, -np.inf, -250.5
    return z


# ---- the reference's own properties ---------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("method", ["nearest", "bilinear", "cubic", "average", "sum", "min", "max"])
def test_reference_identity(method, dtype):
    z = _raster(dtype=dtype)
    out = R.warp(z, IDENTITY, z.shape, method)
    if method == "nearest":
        R.same(method, out, z)
        return
    ok = R.valid(z.astype(np.float64))
    assert not ok[4, 5] and not ok[10, 7] and not ok[20, 30] and not ok[21, 3] and not ok[0, 0]
    R.same(method, out, np.where(ok, z, dtype(-100)))


def test_reference_mode_identity_and_ties():
    rng = np.random.default_rng(5)
    z = rng.integers(0, 256, (20, 24), dtype=np.uint8)
    R.same("identity", R.warp(z, IDENTITY, z.shape, "mode"), z)
    blk = np.array([[7, 3, 3, 7], [9, 9, 2, 2]], np.uint8)          # 2 x 2 blocks: {7, 3, 9, 9} and {3, 7, 2, 2}
    R.same("mode", R.aggregate(blk, 2, "mode"), np.array([[9, 2]], np.uint8))
    tie = np.array([[200, 5], [5, 200]], np.uint8)                   # an exact tie: the smaller value, not the first
    R.same("tie", R.aggregate(tie, 2, "mode"), np.array([[5]], np.uint8))
    R.same("nodata", R.aggregate(tie, 2, "mode", nodata=5), np.array([[200]], np.uint8))
    R.same("fill", R.aggregate(np.full((2, 2), 5, np.uint8), 2, "mode", nodata=5, fill=77), np.array([[77]], np.uint8))


def test_reference_block_sums_are_exact():
    rng = np.random.default_rng(7)
    z = rng.integers(-90, 1000, (24, 36)).astype(np.float64)
    for fy, fx in ((2, 3), (4, 4), (24, 36)):
        want = z.reshape(24 // fy, fy, 36 // fx, fx).sum(axis=(1, 3))
        R.same("sum", R.aggregate(z, (fy, fx), "sum"), want)
        R.same("average", R.aggregate(z, (fy, fx), "average"), want / (fy * fx))
        assert R.aggregate(z, (fy, fx), "sum").sum() == z.sum()


def test_reference_ramp_is_exact():
    Hs, Ws = 12, 14
    ramp = 3.0 + 2.0 * np.arange(Ws)[None, :] - 5.0 * np.arange(Hs)[:, None]
    for zoom in (2, 4):
        shape = (Hs * zoom, Ws * zoom)
        u, v = R.centres((0.0, 1.0 / zoom, 0.0, 0.0, 0.0, 1.0 / zoom), shape)
        want = 3.0 + 2.0 * (u - 0.5) - 5.0 * (v - 0.5)
        for method, margin in (("bilinear", 0.5), ("cubic", 1.5)):
            out = R.resize(ramp, shape, method)
            inner = (u >= margin) & (u < Ws - margin) & (v >= margin) & (v < Hs - margin)
            assert inner.sum() > 0.4 * inner.size
            assert np.array_equal(out[inner], np.broadcast_to(want, shape)[inner]), (zoom, method)


def test_reference_ranges():
    z = _raster((40, 50), seed=11)
    lo, av, hi = (R.aggregate(z, 3, how) for how in ("min", "average", "max"))
    has = av > -100
    assert has.sum() > 150 and np.array_equal(has, lo > -100) and np.array_equal(has, hi > -100)
    assert (lo[has] <= av[has]).all() and (av[has] <= hi[has]).all()


def test_reference_ranges_on_the_inputs_of_the_gpu_test():
    """what test_gpu_resample.py::test_ranges asks of the library, asked of the reference on the same raster"""
    z = R.range_case()
    R.check_ranges(z, [R.aggregate(z, 3, how) for how in ("min", "average", "max")], R.warp(z, *R.RANGE_ZOOM, "bilinear"))


# ---- refusals: all before any library call (no device here) ---------------------------------------------------------
def test_refusals(monkeypatch):
    def no_library():
        raise AssertionError("the library was called")
    monkeypatch.setattr(_lib, "lib", no_library)
    z = np.ones((8, 9), np.float32)
    u8 = np.ones((8, 9), np.uint8)
    bad = [
        lambda: resample.warp(np.ones(5), IDENTITY, (4, 4)),
        lambda: resample.warp(np.ones((2, 3, 4)), IDENTITY, (4, 4)),
        lambda: resample.warp(np.ones((0, 5)), IDENTITY, (4, 4)),
        lambda: resample.warp(np.broadcast_to(np.uint8(1), (1 << 16, 1 << 15)), IDENTITY, (4, 4)),
        lambda: resample.warp(z, IDENTITY, (0, 4)),
        lambda: resample.warp(z, IDENTITY, (4, -1)),
        lambda: resample.warp(z, IDENTITY, (1 << 16, 1 << 15)),
        lambda: resample.warp(z, IDENTITY, (4.0, 4)),
        lambda: resample.warp(z, IDENTITY, 4),
        lambda: resample.warp(z, (0, 1, 0, 0, 0), (4, 4)),
        lambda: resample.warp(z, (0, 1, 0, 0, 0, math.nan), (4, 4)),
        lambda: resample.warp(z, (0, 1, 0, math.inf, 0, 1), (4, 4)),
        lambda: resample.warp(z, (0, 1, 0, 0, 0, "x"), (4, 4)),
        lambda: resample.warp(z, (0, 1, 2, 0, 2, 4), (4, 4)),                # singular
        lambda: resample.warp(z, (0, 0, 0, 0, 0, 1), (4, 4)),
        lambda: resample.warp(z, IDENTITY, (4, 4), "lanczos"),
        lambda: resample.warp(u8, IDENTITY, (4, 4), "bilinear"),
        lambda: resample.warp(z.astype(np.float16), IDENTITY, (4, 4), "cubic"),
        lambda: resample.warp(z.astype(np.int32), IDENTITY, (4, 4), "average"),
        lambda: resample.warp(z, IDENTITY, (4, 4), "mode"),
        lambda: resample.warp(u8.astype(np.int8), IDENTITY, (4, 4), "mode"),
        lambda: resample.warp(z.astype(np.complex64), IDENTITY, (4, 4)),
        lambda: resample.warp(z, (0, 1, 0.1, 0, 0, 1), (4, 4), "average"),     # rotated
        lambda: resample.warp(z, (0, 1, 0, 0, 0.1, 1), (4, 4), "sum"),
        lambda: resample.warp(z, (8, -1, 0, 0, 0, 1), (4, 4), "min"),          # flipped
        lambda: resample.warp(u8, (0, 1, 0, 8, 0, -1), (4, 4), "mode"),
        lambda: resample.warp(z, (0, 257, 0, 0, 0, 1), (4, 4), "average"),     # the footprint cap
        lambda: resample.warp(z, (0, 1, 0, 0, 0, 256.5), (4, 4), "max"),
        lambda: resample.aggregate(z, 257, "average"),
        lambda: resample.aggregate(z, (1, 257), "sum"),
        lambda: resample.aggregate(z, 0),
        lambda: resample.aggregate(z, 2.0),
        lambda: resample.aggregate(z, 2, "nearest"),
        lambda: resample.warp(u8, IDENTITY, (4, 4), "nearest", fill=256),
        lambda: resample.warp(u8, IDENTITY, (4, 4), "nearest", fill=-100),
        lambda: resample.warp(u8, IDENTITY, (4, 4), "nearest", fill=1.5),
        lambda: resample.warp(u8 > 0, IDENTITY, (4, 4), "nearest", fill=2),
        lambda: resample.warp(z.astype(np.int16), IDENTITY, (4, 4), "nearest", fill=40000),
        lambda: resample.warp(z, IDENTITY, (4, 4), "nearest", fill=1e-3),      # not a float32 value
        lambda: resample.warp(z, IDENTITY, (4, 4), "bilinear", fill=0.0),
        lambda: resample.warp(u8, IDENTITY, (4, 4), "mode", nodata=256),
        lambda: resample.warp(u8, IDENTITY, (4, 4), "mode", nodata=-1),
        lambda: resample.warp(u8, IDENTITY, (4, 4), "mode", fill=300),
        lambda: resample.warp(z, IDENTITY, (4, 4), "average", nodata=0),
        lambda: resample.resize(z, (0, 3)),
        lambda: resample.align(z, (0, 0, 0, 0, 0, 0), (0, 1, 0, 0, 0, -1), (4, 4)),
        lambda: resample.compose((0, 1, 0, 0, 0, -1), (0, 2, 1, 0, 4, 2)),
        lambda: resample.compose((0, 1, 0, 0, 0), (0, 1, 0, 0, 0, -1)),
        lambda: resample.compose((0, 1, 0, 0, math.nan, 1), (0, 1, 0, 0, 0, -1)),
    ]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            pytest.fail("case %d was accepted" % k)


def test_cap_message_says_to_chain():
    with pytest.raises(ValueError, match="chain two calls"):
        resample.aggregate(np.ones((300, 520)), 257, "average")


# ---- compose --------------------------------------------------------------------------------------------------------
def _compose_exact(s, d):
    x0, dx, rx, y0, ry, dy = (Fraction(v) for v in s)
    X0, DX, RX, Y0, RY, DY = (Fraction(v) for v in d)
    det = dx * dy - rx * ry
    ex, ey = X0 - x0, Y0 - y0
    return ((dy * ex - rx * ey) / det, (dy * DX - rx * RY) / det, (dy * RX - rx * DY) / det,
            (dx * ey - ry * ex) / det, (dx * RY - ry * DX) / det, (dx * DY - ry * RX) / det)


@pytest.mark.parametrize("s, d", [
    ((500000.0, 32.0, 0.0, 4100000.0, 0.0, -32.0), (500096.0, 128.0, 0.0, 4099904.0, 0.0, -128.0)),
    ((500000.0, 128.0, 0.0, 4100000.0, 0.0, -128.0), (499990.0, 32.0, 0.0, 4100007.0, 0.0, -32.0)),
    ((-8.0, 0.25, 0.0, 3.0, 0.0, -0.5), (1.0, 3.0, 0.0, -2.0, 0.0, -7.0)),
    ((10.0, 2.0, 2.0, 20.0, 2.0, -2.0), (7.0, 1.0, 3.0, 5.0, -3.0, 1.0)),       # rotated, det = -8
    ((0.0, 0.0, 4.0, 0.0, -4.0, 0.0), (3.0, 1.0, 0.0, 9.0, 0.0, -1.0)),         # a quarter turn
])
def test_compose_is_exact_on_dyadic_transforms(s, d):
    got = resample.compose(s, d)
    want = _compose_exact(s, d)
    assert all(isinstance(g, float) for g in got)
    assert tuple(Fraction(g) for g in got) == want
    # and it is what it says: the source pixel of a destination pixel is the same point on the ground
    for x, y in ((0, 0), (5, 3)):
        u, v = want[0] + want[1] * x + want[2] * y, want[3] + want[4] * x + want[5] * y
        gx, gy = Fraction(d[0]) + Fraction(d[1]) * x + Fraction(d[2]) * y, Fraction(d[3]) + Fraction(d[4]) * x + Fraction(d[5]) * y
        assert Fraction(s[0]) + Fraction(s[1]) * u + Fraction(s[2]) * v == gx
        assert Fraction(s[3]) + Fraction(s[4]) * u + Fraction(s[5]) * v == gy


def test_compose_identity_and_resize_matrix():
    t = (500000.0, 30.0, 0.0, 4100000.0, 0.0, -30.0)
    assert resample.compose(t, t) == IDENTITY


# ---- rasterio_lite --------------------------------------------------------------------------------------------------
def test_geotransform_round_trip(tmp_path):
    a = np.arange(12, dtype=np.float32).reshape(3, 4)
    assert rasterio_lite.geotransform({"tags": {}}) is None
    t = (500012.5, 30.0, 0.0, 4100000.25, 0.0, -30.0)
    meta = rasterio_lite.with_geotransform({"tags": {}, "nodata": None, "pixel": None}, t)
    assert rasterio_lite.geotransform(meta) == t and meta["pixel"] == (30.0, 30.0)
    p = str(tmp_path / "a.tif")
    rasterio_lite.write(p, a, like=meta, nodata=-100.0)
    b, m = rasterio_lite.read(p)
    assert np.array_equal(a, b) and m["nodata"] == -100.0
    assert rasterio_lite.geotransform(m) == t
    # the other tags of a template survive, the template itself is not touched
    t2 = (t[0] + 60.0, 120.0, 0.0, t[3] - 30.0, 0.0, -90.0)
    m2 = rasterio_lite.with_geotransform(m, t2)
    assert rasterio_lite.geotransform(m) == t and rasterio_lite.geotransform(m2) == t2
    assert set(m2["tags"]) == set(m["tags"])
    # a tie point that is not at the raster's corner
    tie = {"tags": {rasterio_lite.MODEL_PIXEL_SCALE: (2.0, 4.0, 0.0),
                    rasterio_lite.MODEL_TIEPOINT: (1.0, 2.0, 0.0, 100.0, 200.0, 0.0)}}
    assert rasterio_lite.geotransform(tie) == (98.0, 2.0, 0.0, 208.0, 0.0, -4.0)
    with pytest.raises(ValueError):
        rasterio_lite.with_geotransform(m, (0.0, 1.0, 0.5, 0.0, 0.0, -1.0))
    with pytest.raises(ValueError):
        rasterio_lite.with_geotransform(m, (0.0, 1.0, 0.0, 0.0, -0.5, -1.0))
    # a positive pixel scale is all a GeoTIFF's tag can hold: south-up, mirrored, degenerate and non-finite are refused
    for bad in ((0.0, 1.0, 0.0, 0.0, 0.0, 1.0), (0.0, -1.0, 0.0, 0.0, 0.0, -1.0), (0.0, 0.0, 0.0, 0.0, 0.0, -1.0),
                (0.0, 1.0, 0.0, 0.0, 0.0, 0.0), (math.nan, 1.0, 0.0, 0.0, 0.0, -1.0), (0.0, math.inf, 0.0, 0.0, 0.0, -1.0)):
        with pytest.raises(ValueError):
            rasterio_lite.with_geotransform(m, bad)


# ---- plumbing -------------------------------------------------------------------------------------------------------
def test_source_header_and_bindings():
    assert "dt_resample.hip" in build.SOURCES
    assert os.path.exists(os.path.join(build.CSRC, "dt_resample.hip"))
    hdr = open(os.path.join(ROOT, "include", "descriptools_hip.h")).read()
    vp, ci, i64 = C.c_void_p, C.c_int, C.c_int64
    tail = [ci, i64, i64, C.POINTER(C.c_double), ci, i64, C.c_uint64, vp, i64, i64]
    for name, args in (("dt_resample", [vp] + tail), ("dt_dev_resample", [vp, vp] + tail)):
        assert re.search(r"\bint %s\(" % name, hdr), name
        res, got = _lib._SIGS[name]
        assert res is ci and got == args, name
        assert hasattr(_lib.lib(), name)


def test_alias_module():
    import descriptools.resample as alias
    for name in ("warp", "compose", "align", "resize", "aggregate"):
        assert getattr(alias, name) is getattr(resample, name)


def test_device_entry_refuses_a_null_context():
    L = _lib.lib()
    m = (C.c_double * 6)(*IDENTITY)
    assert L.dt_dev_resample(None, None, 32, 4, 4, m, 1, -1, 0, None, 4, 4) == -1
    assert L.dt_last_error() == b"invalid argument: ctx is NULL"


def test_host_entry_refuses_before_it_asks_for_a_device():
    L = _lib.lib()
    src = np.zeros(16, np.float64)
    dst = np.zeros(16, np.float64)

    def call(dtype=32, Hs=2, Ws=2, m=IDENTITY, method=1, nodata=-1, Hd=2, Wd=2):
        mat = (C.c_double * 6)(*m)
        return L.dt_resample(src.ctypes.data, dtype, Hs, Ws, mat, method, nodata, 0, dst.ctypes.data, Hd, Wd)

    for kw, word in ((dict(Hs=0), b"empty"), (dict(Wd=0), b"empty"), (dict(Hs=1 << 16, Ws=1 << 15), b"2^31"),
                     (dict(Hd=1 << 16, Wd=1 << 15), b"2^31"), (dict(m=(0, 1, 0, 0, 0, math.nan)), b"finite"),
                     (dict(m=(0, 1, 2, 0, 2, 4)), b"singular"), (dict(method=8), b"method"),
                     (dict(method=-1), b"method"), (dict(dtype=4), b"float32"), (dict(dtype=32, method=0), b"nearest"),
                     (dict(dtype=2, method=7), b"mode"), (dict(method=3, m=(0, 1, 0.5, 0, 0, 1)), b"axis-aligned"),
                     (dict(method=5, m=(0, -1, 0, 0, 0, 1)), b"axis-aligned"),
                     (dict(method=3, m=(0, 257, 0, 0, 0, 1)), b"chain two calls"),
                     (dict(method=4, m=(0, 1, 0, 0, 0, 256.5)), b"chain two calls"),
                     (dict(dtype=1, method=7, nodata=256), b"nodata")):
        assert call(**kw) == -1, kw
        assert word in L.dt_last_error(), (kw, L.dt_last_error())
    assert L.dt_resample(None, 32, 2, 2, (C.c_double * 6)(*IDENTITY), 1, -1, 0, None, 2, 2) == -1
    assert L.dt_last_error() == b"invalid argument: NULL raster"
