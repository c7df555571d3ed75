"""GPU (-m gpu): descriptools_amd.filters against the numpy reference of tests/_filters_ref.py, bit for bit, on both
tiers: the host entries through the Python functions, the dt_dev_filter_* entries on device rasters.

Float outputs are compared as their uint32 views and their NaN positions as masks.  Beside the common small shapes, the
kernels' own sizes, each minus one, exact and plus one on either axis:
  extremes    k_fx_rows walks tiles of 64 x 64 (FX_T) and k_fx_cols takes 256 columns a block: 63 / 64 / 65 and 255 /
              256 / 257.  A segment holds L = 2 R + 1 cells, a k_fx_rows wave walks floor(1024 / L) L columns and a
              k_fx_cols thread floor(128 / L) L rows (at least one segment): per radius R in 1, 2, 7, 64 the sizes
              L - 1, L, L + 1 and both spans - 1, exact, + 1, as 5 x n and n x 5 rasters (test_extremes_at_the_seams).
              L = 3, 5, 15 and 129 divide none of the widths 70, 131 and 2051 but 3 | 131 - 2.
  percentile  k_fr_rank and k_fr_rank_net tile 64 x 16 (FR_TX x FR_TY), a lane takes 4 rows: 63 / 64 / 65 columns, 15 /
              16 / 17 rows.  Radius 1 and 2 take the sorting network, 3 and more the bitwise search: 1, 2, 3, 5 and 16.
  denoise     k_fd_normals tiles 64 x 16 and k_fd_smooth 32 x 32 (FD_T): the above and 31 / 32 / 33 on both axes."""
import ctypes as C
import math

import numpy as np
import pytest

import _filters_ref as R

pytestmark = pytest.mark.gpu

COMMON = [(1, 1), (1, 70), (70, 1), (3, 3), (67, 131)]
EXTREMES_SHAPES = COMMON + [(130, 2051), (2051, 67), (63, 65), (64, 64), (65, 63), (7, 257), (8, 256), (9, 255)]
RANK_TILE_SHAPES = [(15, 63), (16, 64), (17, 65)]
DENOISE_SHAPES = COMMON + RANK_TILE_SHAPES + [(31, 33), (32, 32), (33, 31)]
_CACHE = {}


def _dem(shape, noise=0.02):
    key = (shape, noise)
    if key not in _CACHE:
        d = R.terrain(shape[0], shape[1], seed=shape[0] * 7 + shape[1], holes=shape[0] * shape[1] >= 64, noise=noise)
        d.setflags(write=False)
        _CACHE[key] = d
    return _CACHE[key]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_same(got, want, what):
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), "%s: NaN positions differ at %d cells" % (what, int((gn != wn).sum()))
    diff = (_bits(got) != _bits(want)) & ~gn
    assert not diff.any(), "%s: %d cells differ, first at %s: %r, reference %r" % (
        what, int(diff.sum()), tuple(np.argwhere(diff)[0]), got[diff][0], want[diff][0])


# ---- extremes ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [1, 2, 7, 64, "whole"])
@pytest.mark.parametrize("shape", EXTREMES_SHAPES, ids=lambda s: "%dx%d" % s)
def test_extremes_equal_the_reference_bit_for_bit(shape, radius):
    from descriptools_amd import filters
    dem = _dem(shape)
    r = max(shape) if radius == "whole" else radius
    got = filters.extremes(dem, r, ("min", "max", "range"))
    want = R.extremes(dem, r)
    assert list(got) == ["min", "max", "range"]
    if shape[0] * shape[1] >= 64:
        assert (want["min"] == -100).any()
    for k in got:
        _assert_same(got[k], want[k], "%s at radius %d" % (k, r))


@pytest.mark.parametrize("radius", [1, 2, 7, 64])
def test_extremes_at_the_seams(radius):
    from descriptools_amd import filters
    L = 2 * radius + 1
    span_x, span_y = max(1024 // L, 1) * L, max(128 // L, 1) * L
    sizes = sorted({s + d for s in (L, span_x, span_y) for d in (-1, 0, 1)})
    for n in sizes:
        for shape in ((5, n), (n, 5)):
            dem = R.terrain(shape[0], shape[1], seed=n + radius, holes=True)
            got = filters.extremes(dem, radius, ("min", "max"))
            want = R.extremes(dem, radius)
            for k in got:
                _assert_same(got[k], want[k], "%s of %s at radius %d" % (k, shape, radius))


def test_single_output_forms():
    from descriptools_amd import filters
    dem = _dem((67, 131))
    want = R.extremes(dem, 3)
    _assert_same(filters.minimum(dem, 3), want["min"], "minimum")
    _assert_same(filters.maximum(dem, 3), want["max"], "maximum")
    _assert_same(filters.relief(dem, 3), want["range"], "relief")
    got = filters.extremes(dem, 3, ("range", "min"))
    assert list(got) == ["range", "min"]


@pytest.mark.parametrize("radius", [1, 7, 64])
@pytest.mark.parametrize("shape", [(1, 70), (3, 3), (67, 131), (130, 2051)], ids=lambda s: "%dx%d" % s)
def test_opening_and_closing_equal_the_reference(shape, radius):
    from descriptools_amd import filters
    dem = _dem(shape)
    _assert_same(filters.opening(dem, radius), R.opening(dem, radius), "opening")
    _assert_same(filters.closing(dem, radius), R.closing(dem, radius), "closing")


def test_extremes_of_an_all_invalid_raster():
    from descriptools_amd import filters
    dem = np.full((40, 70), -100, np.float32)
    dem[3, 4], dem[5, 6], dem[7, 8] = np.nan, np.inf, -9999
    for out in list(filters.extremes(dem, 5, ("min", "max", "range")).values()) + [filters.opening(dem, 5),
                                                                                  filters.closing(dem, 5)]:
        assert out.dtype == np.float32 and (out == -100).all()


def test_signed_zeros_are_ordered():
    from descriptools_amd import filters
    dem = np.zeros((6, 9), np.float32)
    dem[2, 3] = -0.0
    got = filters.extremes(dem, 1, ("min", "max"))
    want = R.extremes(dem, 1)
    assert np.signbit(want["min"][2, 2]) and not np.signbit(want["max"][2, 2]) and not np.signbit(want["min"][5, 8])
    for k in got:
        _assert_same(got[k], want[k], k)


# ---- percentile ------------------------------------------------------------------------------------------------------------
QS = (0, 10, 50, 100)


@pytest.mark.parametrize("radius", [1, 2, 5, 16])
@pytest.mark.parametrize("shape", COMMON, ids=lambda s: "%dx%d" % s)
def test_percentile_equals_the_reference_bit_for_bit(shape, radius):
    from descriptools_amd import filters
    dem = _dem(shape)
    for q, want in zip(QS, R.percentiles(dem, radius, QS)):
        _assert_same(filters.percentile(dem, radius, q), want, "q=%r at radius %d" % (q, radius))


@pytest.mark.parametrize("radius", [1, 3])
@pytest.mark.parametrize("shape", RANK_TILE_SHAPES + [(130, 300)], ids=lambda s: "%dx%d" % s)
def test_percentile_at_the_tile_seams(shape, radius):
    from descriptools_amd import filters
    dem = _dem(shape)
    for q, want in zip(QS, R.percentiles(dem, radius, QS)):
        _assert_same(filters.percentile(dem, radius, q), want, "q=%r at radius %d" % (q, radius))


def test_median_is_the_percentile_at_50():
    from descriptools_amd import filters
    dem = _dem((67, 131))
    _assert_same(filters.median(dem, 2), R.percentile(dem, 2, 50.0), "median")


def test_percentile_of_equal_heights():
    from descriptools_amd import filters
    dem = np.full((20, 70), 57.5, np.float32)
    dem[4:6, 10:13] = -100
    for q in QS:
        out = filters.percentile(dem, 3, q)
        _assert_same(out, np.where(R.valid(dem), np.float32(57.5), np.float32(-100)).astype(np.float32), "q=%r" % q)


def test_percentile_of_a_window_of_one():
    from descriptools_amd import filters
    dem = np.full((9, 11), -100, np.float32)
    dem[4, 5] = 12.25
    for r in (1, 2):
        for q in QS:
            _assert_same(filters.percentile(dem, r, q), dem, "radius %d q=%r" % (r, q))


# ---- denoise ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius,iterations,threshold,px", [(1, 1, 5.0, 2.0), (5, 3, 30.0, 2.0), (5, 1, 5.0, 29.7),
                                                            (1, 3, 30.0, 29.7)])
@pytest.mark.parametrize("shape", DENOISE_SHAPES, ids=lambda s: "%dx%d" % s)
def test_denoise_equals_the_reference_bit_for_bit(shape, radius, iterations, threshold, px):
    from descriptools_amd import filters
    dem = _dem(shape, noise=0.002)
    got = filters.denoise(dem, px, radius, threshold, iterations)
    want = R.denoise(dem, px, radius, threshold, iterations)
    _assert_same(got, want, "denoise")
    bad = ~R.valid(dem)
    assert np.array_equal(_bits(got)[bad], _bits(dem)[bad])


def test_denoise_where_max_change_rejects_some_cells():
    from descriptools_amd import filters
    dem = _dem((67, 131), noise=0.002)
    ok = R.valid(dem)
    accepted = []
    want = R.denoise(dem, 2.0, 5, 15.0, 3, 0.05, accepted)
    for acc in accepted:  # the reference itself accepts some valid cells and rejects others
        assert acc[ok].any() and (~acc[ok]).any()
    _assert_same(filters.denoise(dem, 2.0, max_change=0.05), want, "denoise")


def test_denoise_defaults_on_a_noisy_step():
    from descriptools_amd import filters
    _, noisy = R.step_surface(60, 90, 2.0, seed=7, holes=True)
    _assert_same(filters.denoise(noisy, 2.0), R.denoise(noisy, 2.0), "denoise")


# ---- the device tier -------------------------------------------------------------------------------------------------------
def _u16(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


@pytest.mark.parametrize("shape", [(3, 3), (67, 131), (130, 300)], ids=lambda s: "%dx%d" % s)
def test_device_tier_equals_the_reference(shape):
    from descriptools_amd import _lib, filters
    from descriptools_amd.device import Context
    L = _lib.lib()
    dem = _dem(shape, noise=0.002)
    H, W = dem.shape
    ctx = Context()
    try:
        d = ctx.to_device(dem)
        o = [ctx.empty((H, W), np.float32) for _ in range(5)]
        _lib.check(L.dt_dev_filter_extremes(ctx.h, d.ptr, H, W, 7, *[a.ptr for a in o]))
        ctx.sync()
        ext = R.extremes(dem, 7)
        for a, want, what in zip(o, (ext["min"], ext["max"], ext["range"], R.opening(dem, 7), R.closing(dem, 7)),
                                 ("min", "max", "range", "opening", "closing")):
            _assert_same(a.to_host(), want, what)
        # one output alone leaves the others untouched
        o[1].copy_from(np.full((H, W), 7.0, np.float32))
        _lib.check(L.dt_dev_filter_extremes(ctx.h, d.ptr, H, W, 2, None, None, None, o[0].ptr, None))
        ctx.sync()
        _assert_same(o[0].to_host(), R.opening(dem, 2), "opening alone")
        assert (o[1].to_host() == 7.0).all()
        table = filters.rank_table(2, 10.0)
        _lib.check(L.dt_dev_filter_rank(ctx.h, d.ptr, H, W, 2, _u16(table), table.size, o[0].ptr))
        ctx.sync()
        _assert_same(o[0].to_host(), R.percentile(dem, 2, 10.0), "rank")
        t = math.cos(math.radians(15.0))
        for it in (1, 2, 3):  # the last step lands in `out` whatever the parity
            _lib.check(L.dt_dev_filter_denoise(ctx.h, d.ptr, H, W, 29.7, 5, t, it, 0.5, o[0].ptr))
            ctx.sync()
            _assert_same(o[0].to_host(), R.denoise(dem, 29.7, 5, 15.0, it, 0.5), "denoise, %d steps" % it)
        assert ctx.status() == 0
        assert np.array_equal(_bits(d.to_host()), _bits(dem))
        for a in o + [d]:
            a.free()
    finally:
        ctx.close()


def test_device_tier_refusals():
    from descriptools_amd import _lib, filters
    from descriptools_amd.device import Context
    L = _lib.lib()
    ctx = Context()
    try:
        d = ctx.to_device(np.zeros((4, 5), np.float32))
        o = ctx.empty((4, 5), np.float32)
        table = filters.rank_table(1, 50.0)
        bad_table = table.copy()
        bad_table[3] = 3
        t = math.cos(math.radians(15.0))
        ext = lambda r=1, outs=(o.ptr, None, None, None, None), dem=d.ptr, H=4: \
            L.dt_dev_filter_extremes(ctx.h, dem, H, 5, r, *outs)
        rank = lambda r=1, tab=table, n=None, out=o.ptr, dem=d.ptr: \
            L.dt_dev_filter_rank(ctx.h, dem, 4, 5, r, _u16(tab) if tab is not None else None,
                                 (tab.size if tab is not None else 10) if n is None else n, out)
        den = lambda px=2.0, r=5, c=t, it=3, mc=0.5, out=o.ptr, dem=d.ptr: \
            L.dt_dev_filter_denoise(ctx.h, dem, 4, 5, px, r, c, it, mc, out)
        for call, msg in ((lambda: ext(r=0), b"[1, 4096]"), (lambda: ext(r=4097), b"[1, 4096]"),
                          (lambda: ext(outs=(None,) * 5), b"no output raster"), (lambda: ext(dem=None), b"NULL raster"),
                          (lambda: ext(H=-1), b"negative raster shape"),
                          (lambda: rank(r=0), b"[1, 16]"), (lambda: rank(r=17), b"[1, 16]"),
                          (lambda: rank(tab=None), b"rank table"), (lambda: rank(n=9), b"rank table"),
                          (lambda: rank(tab=bad_table), b"k[n] must be below n"), (lambda: rank(out=None), b"no output"),
                          (lambda: rank(dem=None), b"NULL raster"),
                          (lambda: den(px=0.0), b"px must be"), (lambda: den(r=0), b"[1, 16]"), (lambda: den(r=17), b"[1, 16]"),
                          (lambda: den(c=0.0), b"cos_threshold"), (lambda: den(c=1.0), b"cos_threshold"),
                          (lambda: den(c=float("nan")), b"cos_threshold"), (lambda: den(it=0), b"iterations"),
                          (lambda: den(it=33), b"iterations"), (lambda: den(mc=0.0), b"max_change"),
                          (lambda: den(mc=float("inf")), b"max_change"), (lambda: den(out=None), b"no output"),
                          (lambda: den(dem=None), b"NULL raster"), (lambda: den(out=d.ptr), b"must not be dem")):
            assert call() == -1
            assert msg in L.dt_last_error(), L.dt_last_error()
        assert ext(H=0) == 0 and ext() == 0 and rank() == 0 and den() == 0
        ctx.sync()
        assert ctx.status() == 0
        d.free()
        o.free()
    finally:
        ctx.close()


def test_two_runs_agree_byte_for_byte():
    from descriptools_amd import filters
    dem = _dem((130, 2051))
    for f in (lambda: filters.relief(dem, 33), lambda: filters.median(dem, 2), lambda: filters.denoise(dem, 2.0)):
        assert f().tobytes() == f().tobytes()


# ---- the bench tool ----------------------------------------------------------------------------------------------------
def test_bench_tool_prints_one_json_line(tmp_path, capsys, monkeypatch):
    """tools/filters_bench.py under the contract of the op tools (tests/test_gpu_bench_tools.py)"""
    import importlib
    import json
    import os
    monkeypatch.syspath_prepend(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    out = tmp_path / "filters_bench.json"
    importlib.import_module("filters_bench").main(["--size", "512", "--steps", "2", "--warmup", "1", "--out", str(out)])
    line = capsys.readouterr().out.strip()
    res = json.loads(line)
    assert out.read_text() == line + "\n"
    assert res["tool"] == "filters_bench" and res["size"] == [512, 512] and res["steps"] == 2 and res["warmup"] == 1
    assert isinstance(res["timing"], str) and res["timing"]
    want = {"copy_8B_per_cell", "extremes_r4", "extremes_r64", "extremes_r1024", "tpi_r4", "tpi_r64", "tpi_r1024",
            "percentile_r1", "percentile_r2", "percentile_r5", "percentile_r16", "ep_r3", "ep_r6", "ep_r16",
            "denoise_r5_1_step", "denoise_r5_3_steps", "terrain_r5_gradient"}
    assert set(res["ms"]) == want
    for k, v in res["ms"].items():
        assert math.isfinite(v) and v > 0, (k, v)
        assert 0 < res["ms_min_max"][k][0] <= res["ms_min_max"][k][1]
    assert res["status"] == 0
